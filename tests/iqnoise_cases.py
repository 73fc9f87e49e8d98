"""Shared by the Welch and IQ-noise tests (test_welch_host.py, test_iqnoise_host.py, test_gpu_welch.py,
test_gpu_iqnoise.py): the inputs, a numpy restatement of the rules of include/mkidgpu.h
(mkid_welch_psd, mkid_iq_noise), the same rule in long double as the truth, the comparison bar, and
ctypes calls of the host twins with a row stride and pre-filled outputs. Everything here is made once
per process and handed out read-only.

The bar for a spectrum bin, wherever floats are compared and bit-identity is not claimed:
    |P - Pref| <= 2 eta sqrt(Pref S) + eta^2 S,     eta = 4 * 2^-53 * log2(nfft),
S the sum over k of both reference spectra of the pair at that resolution (one series' rounding
reaches the other through the unpacking). An amplitude error of eta sqrt(S) in a transform bin changes
its power by at most that much. ratio() returns |P - Pref| over the bar; units() the eta a difference
needs, in units of 2^-53 log2(nfft) (the bar is 4 of them).
"""
import ctypes
import functools
import math

import numpy as np

from mkids_sdr_amd import _lib, iqnoise

STRIP = _lib.WELCH_STRIP
FS = 200000.0
RES_DT = np.dtype(_lib.IQ_NOISE_DTYPE)
KINDS = ('white', 'dc', 'impulse', 'a_only', 'b_only', 'zeros')
# (nfft, n): one segment, and four segments with an unread tail; at nfft = 8 the second has 34
# segments, so two strips; 4096 is the LDS limit, 8192 the smallest four-step length, 32768 a
# non-square split, 262144 the reference's length (two segments, one channel at a time)
SHAPES = [(8, 8), (8, 143), (64, 64), (64, 163), (4096, 4096), (4096, 10243), (8192, 8192), (8192, 20483),
          (32768, 32768), (32768, 81923), (262144, 3 * 2 ** 17)]


def _ro(a):
    a.setflags(write=False)
    return a


def window(nfft):
    """w and S2 of the rule (S2 correctly rounded: the twin's compensated sum is within an ulp of it)."""
    j = np.arange(nfft, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / (nfft - 1))
    return w, math.fsum(w * w)


def eta(nfft):
    return 4.0 * 2.0 ** -53 * math.log2(nfft)


def ratio(P, Pref, S, nfft):
    """|P - Pref| over the bar, per bin; where the bar is 0 (S == 0) equal values give 0, others inf."""
    e = eta(nfft)
    Pref = np.asarray(Pref, np.float64)
    bar = 2.0 * e * np.sqrt(Pref * S) + e * e * S
    d = np.abs(np.asarray(P, np.float64) - Pref)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(d == 0.0, 0.0, d / bar)


def units(P, Pref, S, nfft):
    """The eta that |P - Pref| needs, in units of 2^-53 log2(nfft): the largest over the bins."""
    if S == 0.0:
        return 0.0
    Pref = np.asarray(Pref, np.float64)
    d = np.abs(np.asarray(P, np.float64) - Pref)
    e = (np.sqrt(Pref * S + d * S) - np.sqrt(Pref * S)) / S
    return float(np.max(e)) / (2.0 ** -53 * math.log2(nfft))


def welch_ref(a, b, nfft, fs, long_double=False):
    """The rule of mkid_welch_psd for one channel with np.fft.fft in float64, or with scipy.fft in long
    double (the truth) -> (pa, pb) [nfft/2+1] float64."""
    dt = np.longdouble if long_double else np.float64
    if long_double:
        import scipy.fft
        fft = scipy.fft.fft
    else:
        fft = np.fft.fft
    w, S2 = window(nfft)
    half = nfft // 2
    nseg = (len(a) - half) // half
    acc = [np.zeros(half + 1, dt), np.zeros(half + 1, dt)]
    for s0 in range(0, nseg, STRIP):
        strip = [np.zeros(half + 1, dt), np.zeros(half + 1, dt)]
        for s in range(s0, min(nseg, s0 + STRIP)):
            for x, st in zip((a, b), strip):
                X = fft((x[s * half:s * half + nfft] * w).astype(dt))[:half + 1]
                st += X.real * X.real + X.imag * X.imag
        for t, st in zip(acc, strip):
            t += st
    out = []
    for t in acc:
        P = (t / dt(nseg)) / dt(fs * S2)
        P[1:half] *= 2
        out.append(np.asarray(P, np.float64))
    return out


def impulse_psd(nfft, n, j0, fs):
    """The closed form for a unit impulse at sample j0: every bin of a segment that holds it is w[l]^2."""
    w, S2 = window(nfft)
    half = nfft // 2
    nseg = (n - half) // half
    tot = sum(w[j0 - s * half] ** 2 for s in range(nseg) if 0 <= j0 - s * half < nfft)
    P = np.full(half + 1, tot / nseg / (fs * S2))
    P[1:half] *= 2
    return P


@functools.lru_cache(maxsize=None)
def welch_inputs(nfft, n):
    """The six input kinds of a shape -> dict kind -> (a, b) float64 [n], read-only."""
    rng = np.random.default_rng(1000 + nfft + n)
    z = np.zeros(n)
    imp_a, imp_b = z.copy(), z.copy()
    ja = (n // 2) | 1                     # odd, and inside every shape's first or second segment
    jb = min(n - 1, (nfft // 4) | 1)
    imp_a[ja], imp_b[jb] = 1.0, 1.0
    d = dict(white=(rng.standard_normal(n), rng.standard_normal(n)),
             dc=(1e-2 * rng.standard_normal(n), 1.0 + 3e-4 * rng.standard_normal(n)),
             impulse=(imp_a, imp_b),
             a_only=(rng.standard_normal(n), z.copy()),
             b_only=(z.copy(), rng.standard_normal(n)),
             zeros=(z.copy(), z.copy()))
    return {k: (_ro(a), _ro(b)) for k, (a, b) in d.items()}, (ja, jb)


def block(rows, ld):
    """Rows [nch][n] -> a [nch][ld] array whose padding is NaN (never read)."""
    rows = np.asarray(rows, np.float64)
    out = np.full((rows.shape[0], ld), np.nan)
    out[:, :rows.shape[1]] = rows
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_psd(a, b, n, nfft, fs=FS, group=0, fill=-7.0, want_b=True):
    """mkid_welch_psd_host on [nch][ld] blocks into pre-filled outputs -> (rc, pa, pb)."""
    nch, ld = a.shape
    nb = max(int(nfft) // 2 + 1, 1) if nfft > 0 else 1
    pa = np.full((nch, nb), fill)
    pb = np.full((nch, nb), fill) if want_b else None
    rc = _lib.load().mkid_welch_psd_host(_p(a), _p(b), int(n), int(ld), int(nch), int(nfft), float(fs), int(group),
                                         _p(pa), _p(pb))
    return rc, pa, pb


@functools.lru_cache(maxsize=None)
def host_kinds(nfft, n):
    """The host twin's spectra of every kind of a shape, each run alone (nch = 1, ld = n)."""
    ins, _ = welch_inputs(nfft, n)
    out = {}
    for k, (a, b) in ins.items():
        rc, pa, pb = host_psd(a[None, :].copy(), b[None, :].copy(), n, nfft)
        assert rc == 0
        out[k] = (_ro(pa[0]), _ro(pb[0]))
    return out


def same_bits(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


# ---- the IQ noise analysis ---------------------------------------------------------------------------
FIXTURE_CFG = dict(nfft_low=8192, nfft_high=128, k_join=2, fit_first=140, fit_count=5, samprate=200000.0,
                   f_eval=25000.0, gain=0.2, full_scale=32767.0)
SECOND_CFG = dict(nfft_low=32768, nfft_high=1024, k_join=4, fit_first=150, fit_count=6, samprate=200000.0,
                  f_eval=1000.0, gain=0.2, full_scale=32767.0)
REFERENCE_CFG = dict(iqnoise.DEFAULTS)


def synth_records(nch, n, seed, sigma=30.0, centre=(3000.0, -2000.0)):
    """int16 noise records about `centre` counts (the shape the bar was measured on)."""
    rng = np.random.default_rng(seed)
    I = np.rint(centre[0] + 40.0 * np.arange(nch)[:, None] + sigma * rng.standard_normal((nch, n)))
    Q = np.rint(centre[1] - 25.0 * np.arange(nch)[:, None] + sigma * rng.standard_normal((nch, n)))
    return _ro(I.astype(np.int16)), _ro(Q.astype(np.int16))


def synth_offsets(nch, seed):
    """Zero points, loop centres (well inside the records' means, in scaled units) and Q per channel."""
    rng = np.random.default_rng(seed)
    return dict(i0=_ro(rng.uniform(-1e-3, 1e-3, nch)), q0=_ro(rng.uniform(-1e-3, 1e-3, nch)),
                icen=_ro(rng.uniform(5e-3, 9e-3, nch)), qcen=_ro(rng.uniform(-5e-3, -2e-3, nch)),
                qfit=_ro(rng.uniform(1.5e4, 4e4, nch)))


def fits_of(off):
    p = np.zeros((len(off['qfit']), 10))
    p[:, 0], p[:, 8], p[:, 9] = off['qfit'], off['icen'], off['qcen']
    return {'p': p}


def line_weights(x, xe):
    """The closed-form line's value at xe as sum c_i y_i -> c."""
    xm = x.mean()
    return 1.0 / len(x) + (xe - xm) * (x - xm) / np.sum((x - xm) ** 2)


def iq_ref(I, Q, off, cfg):
    """The rule of mkid_iq_noise in numpy for every channel -> dict like iqnoise.analyze_noise_host's."""
    c = iqnoise.make_cfg(**cfg)
    nch, n = I.shape
    no = iqnoise.nout(c)
    jn = (c.nfft_low // c.nfft_high) * c.k_join
    out = dict(pn=np.zeros((nch, no)), an=np.zeros((nch, no)), freq=iqnoise.freqs(c))
    for k in iqnoise.RESULT_FIELDS:
        out[k] = np.zeros(nch, RES_DT[k])
    out['S_low'], out['S_high'] = np.zeros(nch), np.zeros(nch)
    f = out['freq'][c.fit_first:c.fit_first + c.fit_count]
    for ch in range(nch):
        i0, q0, icen, qcen, qf = (float(off[k][ch]) for k in ('i0', 'q0', 'icen', 'qcen', 'qfit'))
        SI, SQ = int(I[ch].astype(np.int64).sum()), int(Q[ch].astype(np.int64).sum())
        mI = ((SI / n) * c.gain) / c.full_scale - i0 - icen
        mQ = ((SQ / n) * c.gain) / c.full_scale - q0 - qcen
        ang = math.atan2(mQ, mI)
        cs, sn = math.cos(ang), math.sin(ang)
        rad = mI * cs + mQ * sn
        Ia = ((I[ch].astype(np.float64) * c.gain) / c.full_scale - i0) - icen
        Qa = ((Q[ch].astype(np.float64) * c.gain) / c.full_scale - q0) - qcen
        with np.errstate(all='ignore'):
            nI, nQ = (Ia * cs + Qa * sn) / rad, (Qa * cs - Ia * sn) / rad
            phase, amp = np.arctan2(nQ, nI), np.sqrt(nI * nI + nQ * nQ)
        st = 0
        if not all(math.isfinite(v) for v in (i0, q0, icen, qcen)):
            st |= _lib.IQN_NONFINITE
        if not math.isfinite(rad) or rad == 0.0:
            st |= _lib.IQN_BAD_RAD
        if not math.isfinite(qf) or qf == 0.0:
            st |= _lib.IQN_BAD_Q
        if st & _lib.IQN_BAD_RAD:
            out['pn'][ch], out['an'][ch] = np.nan, np.nan
        else:
            pl, al = welch_ref(phase, amp, c.nfft_low, c.samprate)
            ph, ah = welch_ref(phase, amp, c.nfft_high, c.samprate)
            out['S_low'][ch], out['S_high'][ch] = pl.sum() + al.sum(), ph.sum() + ah.sum()
            out['pn'][ch] = np.concatenate([pl[:jn], ph[c.k_join:c.nfft_high // 2]])
            out['an'][ch] = np.concatenate([al[:jn], ah[c.k_join:c.nfft_high // 2]])
        y = out['pn'][ch][c.fit_first:c.fit_first + c.fit_count]
        v = y.mean() + np.sum((f - f.mean()) * (y - y.mean())) / np.sum((f - f.mean()) ** 2) * (c.f_eval - f.mean())
        with np.errstate(all='ignore'):
            fn = v / (16.0 * (qf * qf)) if not st & (_lib.IQN_BAD_RAD | _lib.IQN_BAD_Q) else np.nan
        for k, val in dict(mean_i=mI, mean_q=mQ, resang=ang, rad=rad, fn1k=fn, sum_i=SI, sum_q=SQ,
                           nseg_low=(n - c.nfft_low // 2) // (c.nfft_low // 2),
                           nseg_high=(n - c.nfft_high // 2) // (c.nfft_high // 2), status=st).items():
            out[k][ch] = val
    return out


def compare_noise(got, ref, cfg, label, exact_ints=True):
    """got against ref (an iq_ref dict, or a host-twin dict with S_low / S_high added) under the rules
    of mkid_iq_noise's tests -> the largest ratio of a spectrum bin to its bar. The integers and the
    status are equal; resang and rad within 1e-12 relative; every stitched bin of pn and an under the bar
    of its resolution; fn1k within 1e-12 max|pn[fit]| / (16 Q^2) plus what the bar allows the line."""
    c = iqnoise.make_cfg(**cfg)
    jn = (c.nfft_low // c.nfft_high) * c.k_join
    if exact_ints:
        for k in ('sum_i', 'sum_q', 'nseg_low', 'nseg_high', 'status'):
            assert np.array_equal(got[k], ref[k]), (label, k, got[k], ref[k])
    worst = 0.0
    for ch in range(len(ref['rad'])):
        for k in ('resang', 'rad'):
            g, r = float(got[k][ch]), float(ref[k][ch])
            if math.isfinite(r):
                assert abs(g - r) <= 1e-12 * abs(r), (label, k, ch, g, r)
            else:
                assert g == r or (math.isnan(g) and math.isnan(r)), (label, k, ch, g, r)
        if ref['status'][ch] & _lib.IQN_BAD_RAD:
            assert np.all(np.isnan(got['pn'][ch])) and np.all(np.isnan(got['an'][ch])) and np.isnan(got['fn1k'][ch])
            continue
        rr = np.zeros(got['pn'].shape[1])
        bar = np.zeros_like(rr)
        for lo, hi, S, nfft in ((0, jn, ref['S_low'][ch], c.nfft_low), (jn, None, ref['S_high'][ch], c.nfft_high)):
            for k in ('pn', 'an'):
                r = ratio(got[k][ch][lo:hi], ref[k][ch][lo:hi], S, nfft)
                print('%s ch %d %s[%s:%s] nfft %d: largest ratio to the bar %.4f' % (label, ch, k, lo, hi, nfft, r.max()))
                assert np.all(r <= 1.0), (label, ch, k, lo, float(r.max()))
                worst = max(worst, float(r.max()))
            e = eta(nfft)
            bar[lo:hi] = 2.0 * e * np.sqrt(ref['pn'][ch][lo:hi] * S) + e * e * S
        if ref['status'][ch] & _lib.IQN_BAD_Q:
            assert np.isnan(got['fn1k'][ch])
            continue
        fit = slice(c.fit_first, c.fit_first + c.fit_count)
        q2 = 16.0 * float(ref['qfit'][ch]) ** 2
        w = np.abs(line_weights(ref['freq'][fit], c.f_eval))
        allow = (1e-12 * np.max(np.abs(ref['pn'][ch][fit])) + np.sum(w * bar[fit])) / q2
        print('%s ch %d fn1k %.6e, reference %.6e, allowed %.3e' % (label, ch, got['fn1k'][ch], ref['fn1k'][ch], allow))
        assert abs(got['fn1k'][ch] - ref['fn1k'][ch]) <= allow, (label, ch, got['fn1k'][ch], ref['fn1k'][ch], allow)
    return worst


def host_noise(I, Q, n, off, cfg, fill=-7.0, nullify=()):
    """mkid_iq_noise_host on [nch][ld] int16 blocks into pre-filled outputs -> (rc, pn, an, res)."""
    c = cfg if isinstance(cfg, _lib.IqNoiseCfg) else iqnoise.make_cfg(**cfg)
    nch, ld = I.shape
    no = 4096
    try:
        no = max(iqnoise.nout(c), 1) if c.nfft_high > 0 else no
    except ZeroDivisionError:
        pass
    pn, an = np.full((nch, max(no, 1)), fill), np.full((nch, max(no, 1)), fill)
    res = np.full(nch * RES_DT.itemsize, 0x5A, np.uint8)
    a = dict(i=I, q=Q, i0=np.ascontiguousarray(off['i0']), q0=np.ascontiguousarray(off['q0']),
             icen=np.ascontiguousarray(off['icen']), qcen=np.ascontiguousarray(off['qcen']),
             qfit=np.ascontiguousarray(off['qfit']), pn=pn, an=an, res=res)
    for k in nullify:
        a[k] = None
    rc = _lib.load().mkid_iq_noise_host(_p(a['i']), _p(a['q']), int(n), int(ld), int(nch), _p(a['i0']), _p(a['q0']),
                                        _p(a['icen']), _p(a['qcen']), _p(a['qfit']),
                                        None if 'cfg' in nullify else ctypes.byref(c), _p(a['pn']), _p(a['an']),
                                        _p(a['res']))
    return rc, pn, an, res


def with_sums(host, ref):
    """A host-twin result as a reference for the device: the restatement's S_low, S_high and qfit ride along."""
    out = dict(host)
    out.update(S_low=ref['S_low'], S_high=ref['S_high'], qfit=ref['qfit'])
    return out


@functools.lru_cache(maxsize=None)
def noise_case(name):
    """'fixture2' (the golden file's shape, other data), 'second' (a four-step nfft_low with a non-square
    split) -> dict(I, Q, off, cfg, ref, host): ref the restatement, host the twin's result."""
    cfg, nch, n, seed = dict(second=(SECOND_CFG, 3, 2 * 32768 + 77, 5), fixture2=(FIXTURE_CFG, 2, 20580, 6))[name]
    I, Q = synth_records(nch, n, seed)
    off = synth_offsets(nch, seed + 100)
    ref = iq_ref(I, Q, off, cfg)
    ref['qfit'] = off['qfit']
    host = iqnoise.analyze_noise_host(I, Q, fits_of(off), i0=off['i0'], q0=off['q0'], **cfg)
    return dict(I=I, Q=Q, off=off, cfg=cfg, ref=ref, host=host)
