"""Resonator loop fits (include/mkidgpu.h mkid_fit_loops): every channel's swept IQ loop fitted with
the reference's ten-parameter model (IQsweep.FitLoopMP, lib/iqsweep.py:141-291) in one device call,
giving Q, f0, the loop centre, Qc, Qi and the dip depth per channel. The model, window, guesses,
bounds, start recipe and derived quantities are the reference's; the solver is the library's own.

Resonator magnitude fits (mkid_fit_mags): IQsweep.FitMagMP (:293-356), the six-parameter fit of
|S21| alone, for every channel in one device call; fit_sweeps chains it into the loop fit on the
device, the magnitude fit's Q seeding the loop fit's starts as the reference does (:227-231).
internal_power is the reference's Pint (:275-276), and load_swp / save_swp read and write the .swp
text files of LoadSWP (:97-139) that carry the attenuator setting Pint needs.
"""
import ctypes

import numpy as np

from . import _lib, roach

PARAMS = ('Q', 'f0', 'aleak', 'ph1', 'da', 'ang1', 'Igain', 'Qgain', 'Ioff', 'Qoff')
FIELDS = ('p', 'chisq', 'qc', 'qi', 'dipdb', 'cidx', 'low', 'high', 'n', 'best_start', 'evals', 'status')


def draws(nch, S, seed):
    """The random numbers of lib/iqsweep.py:236-244 for nch channels and S starts -> float64
    [nch][S][5]: g standard normal, u2, u3, u4 uniform in [0, 1), u5 uniform in [-1, 1)."""
    rng = np.random.default_rng(seed)
    d = np.empty((int(nch), int(S), 5), np.float64)
    d[..., 0] = rng.standard_normal((nch, S))
    d[..., 1:4] = rng.random((nch, S, 3))
    d[..., 4] = rng.uniform(-1.0, 1.0, (nch, S))
    return d


def model(p, x):
    """The loop model at frequencies x for parameters p (PARAMS order) -> complex I + iQ, over
    roach.resdiff."""
    return roach.resdiff(x, *[float(v) for v in p])


def _by_field(fits, chisq_all):
    fits = fits.view(np.dtype(_lib.LOOP_FIT_DTYPE))
    out = {k: fits[k].copy() for k in FIELDS}
    out['chisq_all'] = chisq_all
    return out


def _sweep(freq, I, Q):
    f, i, q = (np.ascontiguousarray(a, np.float64) for a in (freq, I, Q))
    if not (f.ndim == 2 and f.shape == i.shape == q.shape):
        raise ValueError('freq, I, Q must be [nch][fsteps] of one shape')
    return f, i, q


def _inputs(freq, I, Q, isd, qsd, dr, qguess):
    f, i, q = _sweep(freq, I, Q)
    nch, fsteps = f.shape
    d = np.ascontiguousarray(dr, np.float64)
    if d.ndim != 3 or d.shape[0] != nch or d.shape[2] != 5:
        raise ValueError('draws must be [nch][S][5]')
    if (isd is None) != (qsd is None):
        raise ValueError('isd and qsd go together')
    sd = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (isd, qsd)]
    if sd[0] is not None and not (sd[0].shape == sd[1].shape == f.shape):
        raise ValueError('isd, qsd must have the shape of I')
    g = None if qguess is None else np.ascontiguousarray(np.broadcast_to(np.asarray(qguess, np.float64), (nch,)))
    return f, i, q, sd[0], sd[1], d, g, nch, fsteps, d.shape[1]


def _device(dev, arrays, outs, enqueue):
    """A device call: `arrays` uploaded and the result buffers `outs` ((shape, dtype) each) zeroed on
    torch's stream, one synchronisation (the kernels run on the context's stream),
    enqueue(uploads, buffers), one synchronisation -> the buffers as numpy arrays."""
    import torch
    t = [None if a is None else torch.from_numpy(a).to(dev) for a in arrays]
    o = [torch.zeros(shape, dtype=getattr(torch, dt), device=dev) for shape, dt in outs]
    torch.cuda.synchronize(dev)
    enqueue(t, o)
    torch.cuda.synchronize(dev)
    return [b.cpu().numpy() for b in o]


def _loop_call(chan, nch, fsteps, S, max_iter, ftol):
    """-> (the result buffers d_fits, d_chisq_all as (shape, dtype); enqueue(t, d_qguess, buffers), t the
    six device arrays freq .. draws)."""
    outs = [(nch * ctypes.sizeof(_lib.LoopFit), 'uint8'), ((nch, S), 'float64')]
    return outs, lambda t, qg, o: chan.fit_loops_device(*t, qg, nch, fsteps, S, max_iter, ftol, *o)


def fit_loops(chan, freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10):
    """Fit every row of a sweep on the GPU of `chan`: freq (Hz), I, Q float64 [nch][fsteps] (zero point
    subtracted), draws [nch][S][5] (draws()), optional isd, qsd (weights 1 / sd) and qguess [nch].
    One device call on the context's stream, one synchronisation, one copy of the results (144 bytes
    a channel) -> dict of arrays by field (FIELDS), 'p' [nch][10] in PARAMS order, and 'chisq_all'
    [nch][S]."""
    *a, nch, fsteps, S = _inputs(freq, I, Q, isd, qsd, draws, qguess)
    outs, enqueue = _loop_call(chan, nch, fsteps, S, max_iter, ftol)
    return _by_field(*_device(chan.torch_device(), a, outs, lambda t, o: enqueue(t[:6], t[6], o)))


def fit_loops_host(freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10):
    """The same call through the host twin (mkid_fit_loops_host); needs no GPU."""
    L = _lib.load()
    f, i, q, sI, sQ, d, g, nch, fsteps, S = _inputs(freq, I, Q, isd, qsd, draws, qguess)
    fits = np.zeros(nch, np.dtype(_lib.LOOP_FIT_DTYPE))
    call = np.zeros((nch, S), np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.mkid_fit_loops_host(p(f), p(i), p(q), p(sI), p(sQ), p(d), p(g), nch, fsteps, S, int(max_iter),
                                     float(ftol), p(fits), p(call)))
    return _by_field(fits, call)


# ---- magnitude fits (include/mkidgpu.h mkid_fit_mags) -----------------------------------------------
MAG_PARAMS = ('Q', 'f0', 'carrier', 'depth', 'slope', 'curve')
MAG_FIELDS = ('p', 'chisq', 'norm', 'cidx', 'best_start', 'evals', 'status')


def mag_draws(nch, S, seed):
    """The random numbers of lib/iqsweep.py:335 for nch channels and S starts -> float64 [nch][S],
    standard normal."""
    return np.random.default_rng(seed).standard_normal((int(nch), int(S)))


def mag_model(p, x):
    """The magnitude model (MAGDIFF, lib/iqsweep.py:913-917; what `magfit` plots) at frequencies x for
    parameters p (MAG_PARAMS order), in the operation order of include/mkidgpu.h."""
    Qp, f0, carrier, depth, slope, curve = [float(v) for v in p]
    x = np.asarray(x, np.float64)
    with np.errstate(all='ignore'):
        dx = (x - f0) / f0
        t = (2.0 * Qp) * dx
        a = np.abs(t) / np.sqrt(1.0 + t * t)
        return (((a - 1.0) * depth + carrier) + slope * dx) + (curve * dx) * dx


def _mag_by_field(fits, qout, chisq_all):
    fits = fits.view(np.dtype(_lib.MAG_FIT_DTYPE))
    out = {k: fits[k].copy() for k in MAG_FIELDS}
    out['qout'], out['chisq_all'] = qout, chisq_all
    return out


def _mag_inputs(freq, I, Q, dr):
    f, i, q = _sweep(freq, I, Q)
    d = np.ascontiguousarray(dr, np.float64)
    if d.ndim != 2 or d.shape[0] != f.shape[0]:
        raise ValueError('draws must be [nch][S]')
    return f, i, q, d, f.shape[0], f.shape[1], d.shape[1]


def _mag_call(chan, nch, fsteps, S, max_iter, ftol):
    """-> (the result buffers d_fits, d_qout, d_chisq_all as (shape, dtype); enqueue(t, buffers), t the
    four device arrays freq .. draws)."""
    outs = [(nch * ctypes.sizeof(_lib.MagFit), 'uint8'), (nch, 'float64'), ((nch, S), 'float64')]
    return outs, lambda t, o: chan.fit_mags_device(*t, nch, fsteps, S, max_iter, ftol, *o)


def fit_mags(chan, freq, I, Q, draws, max_iter=200, ftol=1e-10):
    """Fit the magnitude of every row of a sweep on the GPU of `chan`: freq (Hz), I, Q float64
    [nch][fsteps] (zero point subtracted), draws [nch][S] (mag_draws()). One device call on the
    context's stream, one synchronisation, one copy of the results (80 bytes a channel) -> dict of
    arrays by field (MAG_FIELDS), 'p' [nch][6] in MAG_PARAMS order, 'qout' [nch] (the fitted Q, 50000
    where there is no fit: a valid qguess of fit_loops) and 'chisq_all' [nch][S]."""
    *a, nch, fsteps, S = _mag_inputs(freq, I, Q, draws)
    outs, enqueue = _mag_call(chan, nch, fsteps, S, max_iter, ftol)
    return _mag_by_field(*_device(chan.torch_device(), a, outs, enqueue))


def fit_mags_host(freq, I, Q, draws, max_iter=200, ftol=1e-10):
    """The same call through the host twin (mkid_fit_mags_host); needs no GPU."""
    L = _lib.load()
    f, i, q, d, nch, fsteps, S = _mag_inputs(freq, I, Q, draws)
    fits = np.zeros(nch, np.dtype(_lib.MAG_FIT_DTYPE))
    qout = np.zeros(nch, np.float64)
    call = np.zeros((nch, S), np.float64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.mkid_fit_mags_host(p(f), p(i), p(q), p(d), nch, fsteps, S, int(max_iter), float(ftol), p(fits),
                                    p(qout), p(call)))
    return _mag_by_field(fits, qout, call)


def fit_sweeps(chan, freq, I, Q, mag_draws, loop_draws, isd=None, qsd=None, max_iter=200, ftol=1e-10):
    """The reference's characterisation order on the device: the magnitude fit first, its Q the
    loop fit's Q guess (lib/iqsweep.py:227-231), without a host round trip. One upload,
    fit_mags_device writing d_qout, fit_loops_device reading that buffer as d_qguess on the same
    stream, one synchronisation -> (mags, loops), the dicts fit_mags and fit_loops return. The loop
    results are those of fit_loops(qguess=mags['qout']) bit for bit."""
    f, i, q, sI, sQ, d, _, nch, fsteps, S = _inputs(freq, I, Q, isd, qsd, loop_draws, None)
    md = _mag_inputs(f, i, q, mag_draws)[3]
    mouts, mags = _mag_call(chan, nch, fsteps, md.shape[1], max_iter, ftol)
    louts, loops = _loop_call(chan, nch, fsteps, S, max_iter, ftol)
    o = _device(chan.torch_device(), (f, i, q, sI, sQ, d, md), mouts + louts,
                lambda t, o: (mags(t[:3] + t[6:], o[:3]), loops(t[:6], o[1], o[3:])))
    return _mag_by_field(*o[:3]), _by_field(*o[3:])


def internal_power(fits, atten1):
    """The reference's Pint (lib/iqsweep.py:275-276) in dB for loop fits (a dict with 'p' and 'qc',
    fit_loops') at input attenuator setting atten1 (dB; a scalar or one per channel):
    10 log10((2 Q^2 / (pi Qc)) 10^((-atten1 - 35) / 10)), in numpy on the host."""
    Qm = np.asarray(fits['p'], np.float64)[..., 0]
    qc = np.asarray(fits['qc'], np.float64)
    with np.errstate(all='ignore'):
        power = 10.0 ** ((-np.asarray(atten1, np.float64) - 35.0) / 10.0)
        return 10.0 * np.log10((2.0 * Qm ** 2 / (np.pi * qc)) * power)


# ---- .swp sweep files (lib/iqsweep.py:97-139 LoadSWP) -------------------------------------------------
# Seven tab-separated header lines,
#   f0_0 span_0 fsteps_0 atten1 / f0_1 span_1 fsteps_1 atten2 / Tstart Tend / Iz0 Iz0sd / Qz0 Qz0sd /
#   Iz1 Iz1sd / Qz1 Qz1sd,
# then one table of five columns, freq (GHz) I Isd Q Qsd: resonator 0 in rows 0 .. fsteps_0 - 1,
# resonator 1 in rows fsteps_0 .. fsteps_0 + fsteps_1 - 1 (LoadSWP's h3 offset).
def _ghz_to_hz(tok):
    """A GHz number as text -> the float64 nearest to its value in Hz (the decimal point moved nine
    places, rounded once; LoadSWP's freq * 1e9 rounds twice and may differ in the last bit)."""
    return float(tok + 'e9') if 'e' not in tok.lower() else float(tok) * 1e9


def _hz_to_ghz(v):
    """The text _ghz_to_hz reads back as exactly v."""
    from decimal import Decimal
    return format(Decimal(repr(float(v))).scaleb(-9), 'f') if np.isfinite(v) else repr(float(v))


def load_swp(path, resnum=0):
    """Read resonator `resnum` (0 or 1) of a .swp text file -> dict: 'freq' in Hz, 'I', 'Q' with the
    zero point subtracted, 'Isd', 'Qsd' (float64 [fsteps]), 'atten1', 'atten2', 'f0', 'span' (the
    header's own numbers, GHz), 'fsteps', 'I0', 'Q0', 'I0sd', 'Q0sd', 'Tstart', 'Tend'."""
    if resnum not in (0, 1):
        raise ValueError('resnum is 0 or 1')
    with open(path) as f:
        lines = f.read().splitlines()
    head = [ln.split() for ln in lines[:7]]
    if len(head) < 7 or [len(h) for h in head] != [4, 4, 2, 2, 2, 2, 2]:
        raise ValueError('%s: not a .swp header' % path)
    hv = [[float(v) for v in h] for h in head]
    rows = [ln.split() for ln in lines[7:] if ln.strip()]
    if any(len(r) != 5 for r in rows):
        raise ValueError('%s: the table has five columns' % path)
    n0, n1 = int(hv[0][2]), int(hv[1][2])
    first, n = (0, n0) if resnum == 0 else (n0, n1)
    if n < 0 or first + n > len(rows):
        raise ValueError('%s: resonator %d needs rows %d .. %d of %d' % (path, resnum, first, first + n - 1, len(rows)))
    tab = rows[first:first + n]
    col = lambda k: np.array([float(r[k]) for r in tab], np.float64)
    I0, I0sd = hv[3 + 2 * resnum]
    Q0, Q0sd = hv[4 + 2 * resnum]
    return dict(freq=np.array([_ghz_to_hz(r[0]) for r in tab], np.float64), I=col(1) - I0, Q=col(3) - Q0, Isd=col(2),
                Qsd=col(4), atten1=hv[0][3], atten2=hv[1][3], f0=hv[resnum][0], span=hv[resnum][1], fsteps=n, I0=I0,
                Q0=Q0, I0sd=I0sd, Q0sd=Q0sd, Tstart=hv[2][0], Tend=hv[2][1])


def save_swp(path, res0, res1=None, atten1=0.0, atten2=0.0, tstart=0.0, tend=0.0):
    """Write a .swp text file load_swp (and LoadSWP) reads. res0, res1 (optional): dicts with 'freq'
    in Hz, 'I', 'Q' with the zero point subtracted, 'Isd', 'Qsd', and optionally 'I0', 'Q0' (the
    zero point, added back into the table; default 0), 'I0sd', 'Q0sd', 'f0', 'span' (header numbers
    in GHz; default the sweep's middle and width). Numbers are written with repr, so load_swp returns
    freq, Isd and Qsd exactly, and I and Q exactly wherever I + I0 is exact (a zero point of 0, or
    integer data)."""
    r = repr
    head, zero, table = [], [], []
    for res, att in ((res0, atten1), (res1, atten2)):
        if res is None:
            head.append([0.0, 0.0, 0, float(att)])
            zero += [[0.0, 0.0], [0.0, 0.0]]
            continue
        a = {k: np.asarray(res[k], np.float64) for k in ('freq', 'I', 'Q', 'Isd', 'Qsd')}
        n = a['freq'].shape[0]
        if a['freq'].ndim != 1 or any(v.shape != (n,) for v in a.values()):
            raise ValueError('freq, I, Q, Isd, Qsd must be [fsteps] of one length')
        I0, Q0 = float(res.get('I0', 0.0)), float(res.get('Q0', 0.0))
        f0 = res.get('f0', float((a['freq'].max() + a['freq'].min()) / 2e9) if n else 0.0)
        span = res.get('span', float((a['freq'].max() - a['freq'].min()) / 1e9) if n else 0.0)
        head.append([float(f0), float(span), n, float(att)])
        zero += [[I0, float(res.get('I0sd', 0.0))], [Q0, float(res.get('Q0sd', 0.0))]]
        for k in range(n):
            table.append([_hz_to_ghz(a['freq'][k]), r(float(a['I'][k] + I0)), r(float(a['Isd'][k])),
                          r(float(a['Q'][k] + Q0)), r(float(a['Qsd'][k]))])
    with open(path, 'w') as f:
        for h in head:
            f.write('\t'.join([r(h[0]), r(h[1]), str(h[2]), r(h[3])]) + '\n')
        f.write('\t'.join([r(float(tstart)), r(float(tend))]) + '\n')
        for z in zero:
            f.write('\t'.join([r(z[0]), r(z[1])]) + '\n')
        for row in table:
            f.write('\t'.join(row) + '\n')
