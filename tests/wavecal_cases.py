"""Shared by tests/test_wavecal_host.py and tests/test_gpu_wavecal.py: the restatement of
mkid_spectrum_lines (include/mkidgpu.h) — the integer part in numpy int64, the float64 part in Python
floats, which are IEEE doubles with one rounding per operation, in the order the header states — the
error bars of the float part derived per fit, the numpy fp32 restatement of mkid_energy_cube, ctypes
wrappers of the host twins, and the case tables.

The bars. Device, host twin and this restatement run the same IEEE operations in the same order and
differ only in log (and exp, for amp). For one fit with used bins b (x_b, W_b, y_b = log n_b) the
solution is a = A^-1 X^T W y, so a 1-ulp error in each y_b moves a_i by at most
    da_i = sum_b |(A^-1 X^T W)_ib| ulp(y_b)                         (first order).
A different last bit in y_b also changes the roundings of every later product and sum; their effect
on the solution is bounded norm-wise by cond_2(A) 2^-52 |a|_2 and is added to every da_i. Both are
carried on by the partial derivatives:
    mu_x = -a1 / (2 a2)            dmu_x = da1 / (2 |a2|) + |a1| da2 / (2 a2^2)
    sigma_x = (-1 / (2 a2))^(1/2)  dsigma_x = sigma_x da2 / (2 |a2|)
    amp = exp(a0 - a1^2 / (4 a2))  damp = amp (da0 + |a1| da1 / (2 |a2|) + a1^2 da2 / (4 a2^2) + 4 * 2^-52)
    mu = lo + (m + 1/2 + mu_x) step, sigma = sigma_x |step|: times |step|, plus 4 ulp of the result
(the last operations round differently once their input has moved). The coefficients c are carried
by the Jacobian dc_i / dmu_p, taken by central differences of the restatement's own calibration
(relative step 1e-6; its truncation error is covered by the factor 1.01), plus 4 ulp of |c_i| +
the Jacobian's largest term; R_p = E_p / (k |d_p| sigma_p) with d_p = c1 + 2 c2 mu_p gets
dR / R = dd / |d| + dsigma / sigma + 4 * 2^-52, dd = dc1 + 2 |mu_p| dc2 + 2 |c2| dmu_p.

Determined fits. Whether a fit fails is itself read from floats: a2 < 0, |mu_x| <= g, and for the
calibration the sign of d_p. Where a window is flat (a plateau: every y_b equal) a2 is rounding noise
and its sign turns with the last bit of log. A fit is called determined when |a2| > da2 and
||mu_x| - g| > dmu_x, a calibration when |d_p| > dd_p at every line; only then can two
implementations with different logs be asked for the same status bits and compared in the floats.
The host twin shares this restatement's log (glibc's) and is compared everywhere; the device is
compared in every integer everywhere, and in the status bits and floats of determined channels.
"""
import ctypes
import math

import numpy as np

from mkids_sdr_amd import _lib

import observe_cases as oc

FWHM = 2.3548200450309493
U = 2.0 ** -52
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
LINE_DT = np.dtype(_lib.LINE_FIT_DTYPE)
CAL_DT = np.dtype(_lib.ENERGY_CAL_DTYPE)


# ---- integer part ---------------------------------------------------------------------------------
def counts_of(row):
    """The nbins counts of a row as int64, each read as uint32."""
    return np.ascontiguousarray(row, np.int32).view(np.uint32).astype(np.int64)


def smooth_ref(n, w):
    k = np.array([w + 1 - abs(i) for i in range(-w, w + 1)], np.int64)
    full = np.convolve(n, k)                  # int64: below 65^2 2^32
    return full[w:w + len(n)]


def select_ref(s, P, min_sep, min_peak):
    sp = np.concatenate([[0], s, [0]])
    cand = np.nonzero((s >= min_peak) & (s > sp[:-2]) & (s >= sp[2:]))[0]
    order = cand[np.lexsort((cand, -s[cand]))]
    chosen = []
    for b in order:
        if len(chosen) == P:
            break
        if all(abs(int(b) - c) >= min_sep for c in chosen):
            chosen.append(int(b))
    return sorted(chosen)


def window_ref(bins, p, g, nbins):
    m = bins[p]
    L = (bins[p - 1] + m) // 2 + 1 if p > 0 else 0
    H = (m + bins[p + 1]) // 2 if p + 1 < len(bins) else nbins - 1
    return max(m - g, L), min(m + g, H)


# ---- float64 part ---------------------------------------------------------------------------------
def solve3_ref(S, T):
    m00 = S[2] * S[4] - S[3] * S[3]
    m01 = S[1] * S[4] - S[3] * S[2]
    m02 = S[1] * S[3] - S[2] * S[2]
    det = (S[0] * m00 - S[1] * m01) + S[2] * m02
    t14 = T[1] * S[4] - S[3] * T[2]
    t13 = T[1] * S[3] - S[2] * T[2]
    t12 = S[1] * T[2] - T[1] * S[2]
    t23 = S[2] * T[2] - T[1] * S[3]
    d0 = (T[0] * m00 - S[1] * t14) + S[2] * t13
    d1 = (S[0] * t14 - T[0] * m01) + S[2] * t12
    d2 = (S[0] * t23 - S[1] * t12) + T[0] * m02
    with np.errstate(all='ignore'):
        return [float(np.float64(d) / np.float64(det)) for d in (d0, d1, d2)]


def _spacing(x):
    return float(np.spacing(abs(np.float64(x)))) if math.isfinite(x) else math.inf


def fit_ref(n, m, b0, b1, g, lo, step):
    """-> dict(nfit, counts, mu, sigma, amp, and the bars dmu, dsigma, damp, with cond and dmu_x)."""
    S, T = [0.0] * 5, [0.0] * 3
    xs, Ws, ys = [], [], []
    counts, nfit = 0, 0
    for b in range(b0, b1 + 1):
        c = int(n[b])
        counts += c
        if c < 1:
            continue
        nfit += 1
        x, y = float(b - m), math.log(float(c))
        w0 = float(c) * float(c)
        w1 = w0 * x
        w2 = w1 * x
        w3 = w2 * x
        w4 = w3 * x
        for k, wk in enumerate((w0, w1, w2, w3, w4)):
            S[k] = S[k] + wk
        T[0] = T[0] + w0 * y
        T[1] = T[1] + w1 * y
        T[2] = T[2] + w2 * y
        xs.append(x), Ws.append(w0), ys.append(y)
    out = dict(nfit=nfit, counts=counts, mu=math.nan, sigma=math.nan, amp=math.nan, dmu=math.nan, dsigma=math.nan,
               damp=math.nan, cond=math.nan, dmu_x=math.nan, determined=True)
    if nfit < 3:
        return out
    a = solve3_ref(S, T)
    out['determined'] = False
    if not all(math.isfinite(v) for v in a):
        return out
    # the bars on a (module docstring)
    A = np.array([[S[0], S[1], S[2]], [S[1], S[2], S[3]], [S[2], S[3], S[4]]])
    X = np.vander(np.array(xs), 3, increasing=True)
    try:
        G = np.linalg.solve(A, X.T * np.array(Ws)[None, :])
    except np.linalg.LinAlgError:      # singular to LAPACK: no finite bar
        G = np.full((3, len(xs)), np.inf)
    cond = float(np.linalg.cond(A))
    with np.errstate(all='ignore'):
        da = np.abs(G) @ np.array([_spacing(y) if y != 0.0 else 0.0 for y in ys]) + cond * U * float(np.linalg.norm(a))
    sign_known = bool(abs(a[2]) > da[2])
    if not a[2] < 0.0:
        out['determined'] = sign_known
        return out
    lo, step = float(np.float32(lo)), float(np.float32(step))
    with np.errstate(all='ignore'):
        mu_x = float(np.float64(-a[1]) / np.float64(2.0 * a[2]))
        sigma_x = math.sqrt(-1.0 / (2.0 * a[2]))
        try:
            amp = math.exp(a[0] - (a[1] * a[1]) / (4.0 * a[2]))
        except OverflowError:
            amp = math.inf
    mu = lo + ((float(m) + 0.5) + mu_x) * step
    sigma = sigma_x * abs(step)
    a2 = abs(a[2])
    with np.errstate(all='ignore'):
        dmu_x = da[1] / (2 * a2) + abs(a[1]) * da[2] / (2 * a2 * a2)
        dsigma_x = sigma_x * da[2] / (2 * a2)
    out['determined'] = sign_known and math.isfinite(mu_x) and bool(abs(abs(mu_x) - float(g)) > dmu_x)
    if not all(math.isfinite(v) for v in (mu_x, sigma_x, amp, mu, sigma)) or abs(mu_x) > float(g):
        return out
    out.update(mu=mu, sigma=sigma, amp=amp, cond=cond, dmu_x=float(dmu_x),
               dmu=float(abs(step) * dmu_x + 4 * _spacing(max(abs(mu), abs(lo)))),
               dsigma=float(abs(step) * dsigma_x + 4 * _spacing(sigma)),
               damp=float(amp * (da[0] + abs(a[1]) * da[1] / (2 * a2) + a[1] * a[1] * da[2] / (4 * a2 * a2) + 4 * U)))
    return out


def poly_ref(E, mu):
    """c0, c1, c2 through (mu_p, E_p) in the header's order; float divisions by zero give inf / NaN."""
    P = len(E)
    f = lambda a, b: float(np.float64(a) / np.float64(b))
    with np.errstate(all='ignore'):
        if P == 1:
            return [0.0, f(E[0], mu[0]), 0.0]
        if P == 2:
            c1 = f(E[1] - E[0], mu[1] - mu[0])
            return [E[0] - c1 * mu[0], c1, 0.0]
        f01, f12 = f(E[1] - E[0], mu[1] - mu[0]), f(E[2] - E[1], mu[2] - mu[1])
        f012 = f(f12 - f01, mu[2] - mu[0])
        return [float((np.float64(E[0]) - np.float64(mu[0]) * f01) + np.float64(f012) * (np.float64(mu[0]) * mu[1])),
                float(np.float64(f01) - np.float64(f012) * (np.float64(mu[0]) + mu[1])), f012]


def calibrate_ref(E, fits, found):
    """-> dict(c, r, n_found, status, cal_f, dc, dr, determined)."""
    P = len(E)
    status = _lib.CAL_FEW_LINES if found < P else 0
    for p in range(found):
        if not math.isfinite(fits[p]['mu']):
            status |= _lib.CAL_FIT_FAILED << p
    nan3 = [math.nan] * 3
    c, r, dc, dr = list(nan3), list(nan3), list(nan3), list(nan3)
    determined = all(fits[p]['determined'] for p in range(found))
    if status == 0:
        mu = [fits[p]['mu'] for p in range(P)]
        c = poly_ref(E, mu)
        with np.errstate(all='ignore'):
            d = [float(np.float64(c[1]) + (np.float64(2.0) * c[2]) * mu[p]) for p in range(P)]
        ok = all(math.isfinite(x) and x != 0.0 for x in d) and math.isfinite(c[0]) and (d[0] > 0.0) == (d[-1] > 0.0)
        dd = [math.inf] * P
        if all(math.isfinite(x) for x in c + d):
            # bars: Jacobian of c in mu by central differences
            J = np.zeros((3, P))
            for p in range(P):
                hstep = 1e-6 * max(abs(mu[p]), abs(mu[-1] - mu[0]) if P > 1 else 0.0)
                up, dn = list(mu), list(mu)
                up[p] += hstep
                dn[p] -= hstep
                with np.errstate(all='ignore'):
                    J[:, p] = (np.array(poly_ref(E, up)) - np.array(poly_ref(E, dn))) / (up[p] - dn[p])
            dmu = np.array([fits[p]['dmu'] for p in range(P)])
            with np.errstate(all='ignore'):
                terms = np.abs(J) * dmu[None, :]
                dc = [float(1.01 * terms[i].sum() + 4 * _spacing(abs(c[i]) + np.abs(J[i] * np.array(mu)).max()))
                      for i in range(3)]
                dd = [dc[1] + 2 * abs(mu[p]) * dc[2] + 2 * abs(c[2]) * dmu[p] for p in range(P)]
        determined = determined and all(abs(d[p]) > dd[p] for p in range(P))
        if not ok:
            status |= _lib.CAL_BAD_SLOPE
            c, dc = list(nan3), list(nan3)
        else:
            for p in range(P):
                r[p] = E[p] / ((FWHM * abs(d[p])) * fits[p]['sigma'])
                dr[p] = float(r[p] * (dd[p] / abs(d[p]) + fits[p]['dsigma'] / fits[p]['sigma'] + 4 * U))
    with np.errstate(all='ignore'):
        cal_f = np.array([c[0], c[1], c[2], 1.0 if status == 0 else 0.0], np.float64).astype(np.float32)
    return dict(c=c, r=r, n_found=found, status=status, cal_f=cal_f, dc=dc, dr=dr, determined=determined)


def lines_ref(row, lo, step, nbins, E, w, min_sep, min_peak, g):
    """One channel -> dict(bins, lines: list of P dicts (bin, nfit, peak_s, counts, mu, sigma, amp and
    bars), cal: calibrate_ref's dict)."""
    P = len(E)
    n = counts_of(row)
    s = smooth_ref(n, w)
    bins = select_ref(s, P, min_sep, min_peak)
    lines = []
    for p in range(P):
        if p < len(bins):
            b0, b1 = window_ref(bins, p, g, nbins)
            f = fit_ref(n, bins[p], b0, b1, g, lo, step)
            f.update(bin=bins[p], peak_s=int(s[bins[p]]))
        else:
            f = dict(bin=-1, nfit=0, peak_s=0, counts=0, mu=math.nan, sigma=math.nan, amp=math.nan, dmu=math.nan,
                     dsigma=math.nan, damp=math.nan, cond=math.nan, dmu_x=math.nan, determined=True)
        lines.append(f)
    return dict(bins=bins, lines=lines, cal=calibrate_ref(list(E), lines, len(bins)))


# ---- the host twin --------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def spectra_of(rows, nbins):
    """Rows of nbins counts -> the table [nch][nbins + 3] with junk in the three columns never read."""
    sp = np.full((len(rows), nbins + 3), -7, np.int32)
    for i, r in enumerate(rows):
        sp[i, 1:nbins + 1] = np.asarray(r, np.int64).astype(np.uint32).view(np.int32)   # counts 0 .. 2^32 - 1
    return sp


def lines_host(spectra, lo, step, nbins, E, w, min_sep, min_peak, g, nch=None, null=()):
    """mkid_spectrum_lines_host -> (rc, lines [nch][P], cal [nch], cal_f [nch][4]); `null`: names of
    pointers passed as NULL."""
    L = _lib.load()
    nch = spectra.shape[0] if nch is None else nch
    n = max(spectra.shape[0], 1)
    E = np.ascontiguousarray(E, np.float64)
    P = len(E)
    lo32 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (n,)))
    st32 = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (n,)))
    lines = np.zeros((n, max(P, 1)), LINE_DT)
    cal = np.zeros(n, CAL_DT)
    cal_f = np.zeros((n, 4), np.float32)
    a = dict(spectra=np.ascontiguousarray(spectra, np.int32), lo=lo32, step=st32, E=E, lines=lines, cal=cal, cal_f=cal_f)
    q = {k: (None if k in null else _p(v)) for k, v in a.items()}
    rc = L.mkid_spectrum_lines_host(q['spectra'], q['lo'], q['step'], nch, nbins, P, q['E'], w, min_sep, min_peak, g,
                                    q['lines'], q['cal'], q['cal_f'])
    return rc, lines[:, :P], cal, cal_f


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_ints(lines, cal, ref, status=True):
    """The integer outputs of one channel against the restatement, exactly; status=False leaves
    out the status bits that are read from floats (a channel that is not determined)."""
    for p, f in enumerate(ref['lines']):
        got = (int(lines[p]['bin']), int(lines[p]['nfit']), int(lines[p]['peak_s']), int(lines[p]['counts']))
        assert got == (f['bin'], f['nfit'], f['peak_s'], f['counts']), (p, got, f)
    assert int(cal['n_found']) == ref['cal']['n_found'], (cal, ref['cal'])
    few = _lib.CAL_FEW_LINES
    assert int(cal['status']) & few == ref['cal']['status'] & few, (cal, ref['cal'])
    if status:
        assert int(cal['status']) == ref['cal']['status'], (cal, ref['cal'])


def float_ratio(lines, cal, cal_f, ref):
    """|value - restatement| / bar, the largest over one channel's float outputs; NaN and inf must
    match exactly. cal_f must be the float32 of the channel's own c."""
    worst = 0.0

    def one(got, want, bar):
        nonlocal worst
        got, want = float(got), float(want)
        if not math.isfinite(want) or not math.isfinite(got):
            assert (math.isnan(got) and math.isnan(want)) or got == want, (got, want)
            return
        if got != want:
            assert bar > 0 and math.isfinite(bar), (got, want, bar)
            worst = max(worst, abs(got - want) / bar)

    for p, f in enumerate(ref['lines']):
        one(lines[p]['mu'], f['mu'], f['dmu'])
        one(lines[p]['sigma'], f['sigma'], f['dsigma'])
        one(lines[p]['amp'], f['amp'], f['damp'])
    for i in range(3):
        one(cal['c'][i], ref['cal']['c'][i], ref['cal']['dc'][i])
        one(cal['r'][i], ref['cal']['r'][i], ref['cal']['dr'][i])
    with np.errstate(all='ignore'):
        want_f = np.append(cal['c'].astype(np.float32), np.float32(1.0 if cal['status'] == 0 else 0.0))
    assert np.array_equal(cal_f, want_f, equal_nan=True), (cal_f, want_f)
    return worst


# ---- spectrum rows --------------------------------------------------------------------------------
def gauss_row(nbins, centres, sigma, amp, rng=None, background=0):
    b = np.arange(nbins) + 0.5
    y = np.zeros(nbins)
    for c in centres:
        y += amp * np.exp(-0.5 * ((b - c) / sigma) ** 2)
    y = rng.poisson(y + background) if rng is not None else np.rint(y + background)
    return y.astype(np.int64)


def rows_for(nbins, seed=5):
    """The spectrum shapes of the case table for one nbins: (name, int64 counts [nbins]) each."""
    rng = np.random.default_rng(seed + nbins)
    z = lambda: np.zeros(nbins, np.int64)
    out = [('empty', z())]
    r = z(); r[nbins // 2] = 500; out.append(('one_bin', r))
    r = z(); r[nbins // 3: nbins // 3 + 4] = 40; r[(2 * nbins) // 3: (2 * nbins) // 3 + 2] = 40; out.append(('plateaus', r))
    r = z(); r[nbins // 4] = 77; r[(3 * nbins) // 4] = 77; out.append(('equal_peaks', r))
    r = z(); r[nbins // 2] = 90; r[min(nbins // 2 + 2, nbins - 1)] = 80; r[min(nbins // 2 + 4, nbins - 1)] = 70; out.append(('close_peaks', r))
    r = z(); r[0] = 60; r[nbins - 1] = 61; out.append(('edges', r))
    r = z(); r[nbins // 2] = 2 ** 31 - 1; r[max(nbins // 2 - 1, 0)] = 2 ** 31 - 5; r[min(nbins // 2 + 1, nbins - 1)] = 2 ** 31 + 9
    out.append(('near_2_31', r))
    r = rng.integers(2 ** 32 - 1000, 2 ** 32, nbins); out.append(('negative_int32', r.astype(np.int64)))
    out.append(('noise', rng.poisson(3.0, nbins).astype(np.int64)))
    if nbins >= 64:
        sg = max(nbins / 64.0, 1.5)
        c3 = [nbins * 0.22, nbins * 0.5, nbins * 0.8]
        out.append(('three_lines', gauss_row(nbins, c3, sg, 3000.0, rng, 2)))
        out.append(('two_lines', gauss_row(nbins, c3[:2], sg, 3000.0, rng, 0)))
        for k, name in enumerate(('spike_first', 'spike_middle', 'spike_last')):
            r = gauss_row(nbins, [c for i, c in enumerate(c3) if i != k], sg, 3000.0)
            r[int(c3[k])] = 10 ** 6
            out.append((name, r))
        out.append(('smooth_lines', gauss_row(nbins, c3, sg, 3000.0)))
    return out


NBINS = [1, 2, 3, 64, 257, 16384]
ENERGIES = {1: [3.06], 2: [1.26, 3.06], 3: [1.26, 1.88, 3.06]}   # eV: 983, 660 and 405 nm lasers


def param_table(nbins):
    """(P, w, g, min_sep, min_peak, E) for every P in 1..3, w in {0, 1, 64}, g in {1, 64}, and two with
    energies that are not monotonic in the bin order."""
    out = []
    for P in (1, 2, 3):
        for w in (0, 1, 64):
            for g in (1, 64):
                out.append((P, w, g, max(1, min(nbins // 8, 40)) if (w + g) % 2 else 1, 10 if w else 1, ENERGIES[P]))
    out.append((3, 1, 64, max(1, nbins // 8), 10, [1.26, 3.06, 1.88]))
    out.append((3, 2, 12, max(1, nbins // 16), 10, [3.06, 1.88, 1.26]))
    return out


# ---- the energy cube ------------------------------------------------------------------------------
def energy_ref(h, cf):
    """e for heights h float32 [n] with per-packet table rows cf float32 [n][4]."""
    h = np.asarray(h, np.float32)
    with np.errstate(all='ignore'):
        t = h * cf[:, 2]
        t = cf[:, 1] + t
        t = h * t
        e = cf[:, 0] + t
        assert e.dtype == np.float32
    bad = (cf[:, 3] == 0) | ~np.isfinite(h) | np.isnan(e)
    return np.where(bad, NAN32, e).astype(np.float32)


def cube_ref(ev, h, j0, j_defer, C, cal_f, mode, hc, vlo, vinv, nb, cube=None, energy=None):
    """-> (cube [C][nb + 3] int32, energy float32 [n]); adds to cube, writes into energy when given."""
    cube = np.zeros((C, nb + 3), np.int32) if cube is None else cube
    h = np.asarray(h, np.float32)
    energy = np.full(len(h), np.float32(-1234.5), np.float32) if energy is None else energy
    ch, jg = oc.decode(ev, j0)
    pix = ch < C
    e = energy_ref(h[pix], cal_f[ch[pix]])
    energy[pix] = e
    keep = ~(~np.isfinite(h[pix]) & (jg[pix] >= j_defer))
    with np.errstate(all='ignore'):
        v = e if mode == _lib.CUBE_ENERGY else np.float32(hc) / e
        assert v.dtype == np.float32
    n = int(keep.sum())
    col = oc.column_ref(v[keep], np.full(n, vlo, np.float32), np.full(n, vinv, np.float32), nb)
    np.add.at(cube, (ch[pix][keep], col), 1)
    return cube, energy


def cube_host(ev, h, j0, j_defer, C, cal_f, mode, hc, vlo, vinv, nb, cube=None, energy=None, n=None, null=(),
              want_energy=True):
    """mkid_energy_cube_host -> (rc, cube, energy)."""
    L = _lib.load()
    ev = None if ev is None else np.ascontiguousarray(ev, np.uint64)
    h = None if h is None else np.ascontiguousarray(h, np.float32)
    cube = np.zeros((max(C, 1), max(nb, 1) + 3), np.int32) if cube is None else cube
    n = (0 if ev is None else len(ev)) if n is None else n
    if energy is None and want_energy:
        energy = np.full(max(n, 1), np.float32(-1234.5), np.float32)
    a = dict(ev=ev, h=h, cal_f=np.ascontiguousarray(cal_f, np.float32), cube=cube, energy=energy)
    q = {k: (None if k in null or v is None else _p(v)) for k, v in a.items()}
    rc = L.mkid_energy_cube_host(q['ev'], q['h'], n, j0, j_defer, C, q['cal_f'], mode, float(hc), float(vlo), float(vinv),
                                 nb, q['cube'], q['energy'])
    return rc, cube, (None if energy is None else energy[:n])


def cube_case(C=64, n=3000, seed=9):
    """About n packets in the device's order for a C-channel context: heights around a calibration
    with positive, negative and zero energies, every special height, channels >= C, stamps on both
    sides of j_defer with non-finite heights on both sides, a channel that is not usable, one whose
    energy is 0 for every height and one with infinite coefficients."""
    rng = np.random.default_rng(seed)
    j0, rows = 5000, 2000
    jd = j0 + rows - 80
    jg = j0 + rng.integers(0, rows, n)
    ch = np.where(rng.random(n) < 0.1, rng.integers(C, 4096, n), rng.integers(0, C, n))
    ev = oc.device_order(oc.pack(ch, jg, rng), j0)
    chs, jgs = oc.decode(ev, j0)
    h = rng.normal(-1.0, 0.6, n).astype(np.float32)
    k = rng.random(n) < 0.1
    h[k] = rng.choice(oc.SPECIALS, int(k.sum()))
    late = jgs >= jd
    h[late & (rng.random(n) < 0.7)] = np.nan
    cal_f = np.zeros((C, 4), np.float32)
    cal_f[:, 0] = rng.normal(0.1, 0.05, C)
    cal_f[:, 1] = rng.normal(-2.0, 0.2, C)       # negative heights, positive energies
    cal_f[:, 2] = rng.normal(0.0, 0.05, C)
    cal_f[:, 3] = 1.0
    cal_f[3] = [np.nan, np.nan, np.nan, 0.0]     # not usable
    cal_f[4] = [1.0, 1.0, 0.0, 0.0]              # finite coefficients, still not usable
    cal_f[5] = [0.0, 0.0, 0.0, 1.0]              # e = 0: 1 / e = inf
    cal_f[6] = [np.inf, -np.inf, 0.0, 1.0]       # inf - inf
    cal_f[7] = [-1.0, 0.0, 0.0, 1.0]             # e < 0
    h[(chs == 8) & (rng.random(n) < 0.5)] = 0.0  # e = c0 exactly
    return dict(C=C, ev=ev, h=h, j0=j0, j_defer=jd, cal_f=cal_f)


HC = np.float32(4.13567E-15 * 3.0E17)
CUBE_MODES = [(_lib.CUBE_ENERGY, np.float32(0.92), np.float32(1) / np.float32((3.18 - 0.92) / 10), 10),
              (_lib.CUBE_WAVELENGTH, np.float32(390.0), np.float32(1) / np.float32(95.8), 10),
              (_lib.CUBE_ENERGY, np.float32(-3.0), np.float32(37.5), 257)]
