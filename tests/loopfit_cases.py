"""The float64 restatement of mkid_fit_loops (include/mkidgpu.h; the rules are csrc/loopfit_common.h)
in numpy, the synthetic loops and the case table of tests/test_loopfit_host.py and
tests/test_gpu_loopfit.py.

The restatement does every operation of the header in the header's order. Elementwise numpy float64
arithmetic is one IEEE operation per element and is never fused, so the per-point terms are arrays
over the window's points; sin, cos and atan2 go through `math` one element at a time (the C
library's, which the host twin calls as well). The 64 lane partials are an array [66][64] to which
round r adds the I terms and then the Q terms of points 64 r + l, and the butterfly is p = p + p[l ^ m].
The Cholesky and the iteration are scalar Python floats. The solver (csrc/lm_common.h: lane_sums_ref,
step_ref, run_start_ref) is restated once, here, for any number of parameters; tests/magfit_cases.py
runs its own model through the same functions.

Trig(rng) moves every sin, cos, atan2 (and log10) result by one ulp up or down at random. The window
weights are not moved: the host entry makes them for device and twin alike. The change this makes
over the case table, per quantity, is the measure of what the device's own sin, cos and atan2 may do;
the device's bars (BARS) are ten times the largest change measured, see measure_bars().
"""
import ctypes
import math

import numpy as np

from mkids_sdr_amd import _lib, roach

PI = 3.141592653589793
NP, LANES = 10, 64
LANE = np.arange(LANES)
FIT_DT = np.dtype(_lib.LOOP_FIT_DTYPE)
INT_FIELDS = ('cidx', 'low', 'high', 'n', 'best_start', 'evals', 'status')
FLOAT_FIELDS = ('p', 'chisq', 'qc', 'qi', 'dipdb')
FAIL_BITS = _lib.LOOP_NONFINITE | _lib.LOOP_FLAT | _lib.LOOP_NO_FIT
NAN = float('nan')


def ix(i, j):
    return i * (i + 1) // 2 + j


class Trig:
    """math's sin, cos, atan2, log10 with C's answers for arguments Python raises on; with an rng
    every result is moved by one ulp, up or down at random."""

    def __init__(self, rng=None):
        self.rng = rng

    def _move(self, v):
        if self.rng is None or not math.isfinite(v):
            return v
        return float(np.nextafter(v, math.inf if self.rng.integers(2) else -math.inf))

    def sin1(self, v):
        return self._move(math.sin(v)) if math.isfinite(v) else NAN

    def cos1(self, v):
        return self._move(math.cos(v)) if math.isfinite(v) else NAN

    def sin(self, a):
        return np.array([self.sin1(v) for v in a.tolist()], np.float64)

    def cos(self, a):
        return np.array([self.cos1(v) for v in a.tolist()], np.float64)

    def atan2(self, y, x):
        return self._move(math.atan2(y, x))

    def log10(self, v):
        if v != v or v < 0.0:
            return NAN
        return -math.inf if v == 0.0 else self._move(math.log10(v))


EXACT = Trig()


# ---- the window -------------------------------------------------------------------------------------
def window_weights():
    w = [0.5 + 0.5 * math.cos((PI * float(2 * j - 9)) / 9.0) for j in range(10)]
    s = 0.0
    for v in w:
        s = s + v
    return np.array([v / s for v in w], np.float64)


WN = window_weights()


def velocities(I, Q):
    with np.errstate(all='ignore'):
        dI, dQ = I[:-1] - I[1:], Q[:-1] - Q[1:]
        return np.sqrt(dI * dI + dQ * dQ)[:len(I) - 2]


def padded(v):
    nv = len(v)
    top = min(10, nv - 1)
    with np.errstate(all='ignore'):
        return np.concatenate([2.0 * v[0] - v[top:1:-1], v, 2.0 * v[nv - 1] - v[nv - 1:nv - 10:-1]])


def smooth_ref(v, wn=WN):
    """The explicit sum: sv[i] = sum_j wn[j] s[i + 13 - j], ascending j from 0.0."""
    s = padded(v)
    nsv = len(s) - 18
    acc = np.zeros(nsv)
    with np.errstate(all='ignore'):
        for j in range(10):
            acc = acc + wn[j] * s[13 - j:13 - j + nsv]
    return acc


def window_ref(I, Q):
    fsteps = len(I)
    sv = smooth_ref(velocities(I, Q)).tolist()
    cidx, best = 0, sv[0]
    for i in range(1, len(sv)):
        if sv[i] > best:
            best, cidx = sv[i], i
    low, high = max(cidx - fsteps // 4, 0), min(cidx + fsteps // 4, fsteps)
    return cidx, low, high, high - low


# ---- guesses, bounds, starts ------------------------------------------------------------------------
def clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def guesses_ref(x, I, Q, wI, wQ, k, trig):
    """-> (status, lo[10], hi[10], base[10]) over the window's arrays."""
    finite = bool(np.all(np.isfinite(x)) and np.all(np.isfinite(I)) and np.all(np.isfinite(Q)) and
                  np.all(np.isfinite(wI)) and np.all(np.isfinite(wQ)))
    if not finite:
        return _lib.LOOP_NONFINITE, None, None, None
    xs = 0.0
    for v in x.tolist():
        xs = xs + v
    xmin, xmax = float(x.min()), float(x.max())
    imin, imax, qmin, qmax = float(I.min()), float(I.max()), float(Q.min()), float(Q.max())
    gI, gQ = imax - imin, qmax - qmin
    icen, qcen = gI / 2.0 + imin, gQ / 2.0 + qmin
    ang = trig.atan2(float(Q[k]) - qcen, float(I[k]) - icen)
    ang = ang - PI / 2.0 if ang >= 0.0 else ang + PI / 2.0
    if gI == 0.0 or gQ == 0.0:
        return _lib.LOOP_FLAT, None, None, None
    alim = 1.1 * PI
    lo = [5e3, xmin, 1e-4, 1.0, -5e3, -alim, gI - 0.5 * gI, gQ - 0.5 * gQ, icen - 0.5 * abs(icen),
          qcen - 0.5 * abs(qcen)]
    hi = [1e6, xmax, 1e2, 4e4, 5e3, alim, gI + 0.5 * gI, gQ + 0.5 * gI, icen + 0.5 * abs(icen),
          qcen + 0.5 * abs(qcen)]
    base = [0.0, xs / float(len(x)), 0.0, 0.0, 0.0, ang, gI, gQ, icen, qcen]
    return 0, lo, hi, base


def start_ref(lo, hi, base, s, d, qg):
    qs = qg if qg is not None else 10000.0 * float(s)
    qt = qs + 20000.0 * d[0]
    p = [5000.0 if qt < 5000.0 else qt, base[1], 1.1e-4 + 90.0 * d[1], 1.0 + 3e4 * d[2], 9000.0 * d[3] - 4500.0,
         base[5] if s <= 5 else PI * d[4], base[6], base[7], base[8], base[9]]
    return [clip(p[i], lo[i], hi[i]) for i in range(NP)]


# ---- the model, the Jacobian, the sums ----------------------------------------------------------------
def terms_ref(p, x, yI, yQ, wI, wQ, trig):
    """-> (mI, mQ, rI, rQ, JI [10][n], JQ [10][n]) in the order of loopfit_common.h point_terms."""
    Qp, f0, al, ph1, da, ang, Ig, Qg, Io, Qo = p
    ca, sa = trig.cos1(ang), trig.sin1(ang)
    with np.errstate(all='ignore'):
        dx = (x - f0) / f0
        twoQ = 2.0 * Qp
        t = twoQ * dx
        t2 = t * t
        den = 1.0 + t2
        ph = dx * ph1
        c, s = trig.cos(ph), trig.sin(ph)
        re = (da * dx + (t2 / den - 0.5)) + al * (1.0 - c)
        im = t / den - al * s
        Ix, Qx = re * Ig, im * Qg
        mI = (Ix * ca + Qx * sa) + Io
        mQ = (Qx * ca - Ix * sa) + Qo
        rI, rQ = (yI - mI) * wI, (yQ - mQ) * wQ
        den2, twodx = den * den, 2.0 * dx
        ddx = (-x) / (f0 * f0)
        a, b = (2.0 * t) / den2, (1.0 - t2) / den2
        as_, ac = al * s, al * c
        zero = np.zeros_like(x)
        dre = [a * twodx, ddx * ((da + twoQ * a) + as_ * ph1), 1.0 - c, as_ * dx, dx]
        dim = [b * twodx, ddx * (twoQ * b - ac * ph1), -s, -(ac * dx), zero]
        JI, JQ = [], []
        for k in range(5):
            u, v = Ig * dre[k], Qg * dim[k]
            JI.append((u * ca + v * sa) * wI)
            JQ.append((v * ca - u * sa) * wQ)
        JI += [(Qx * ca - Ix * sa) * wI, (re * ca) * wI, (im * sa) * wI, wI + zero, zero]
        JQ += [(-(Ix * ca + Qx * sa)) * wQ, (-(re * sa)) * wQ, (im * ca) * wQ, zero, wQ + zero]
    return mI, mQ, rI, rQ, np.array(JI), np.array(JQ)


def model_ref(p, x, trig=EXACT):
    x = np.asarray(x, np.float64)
    one = np.ones_like(x)
    mI, mQ = terms_ref([float(v) for v in p], x, one, one, one, one, trig)[:2]
    return mI + 1j * mQ


def chisq_ref(p, x, yI, yQ, wI, wQ, trig=EXACT):
    """chi^2 at p by the lane partials and the butterfly."""
    return sums_ref(p, x, yI, yQ, wI, wQ, trig)[2]


def sums_ref(p, x, yI, yQ, wI, wQ, trig):
    """-> (A [55], g [10], chi) as Python floats: a point adds its I terms, then its Q terms."""
    _, _, rI, rQ, JI, JQ = terms_ref(p, x, yI, yQ, wI, wQ, trig)
    return lane_sums_ref([(JI, rI), (JQ, rQ)])


# ---- the solver (csrc/lm_common.h), for any number of parameters N ------------------------------------
_TRI = {}


def lane_sums_ref(blocks):
    """blocks: the (J [N][n], r [n]) term blocks a point adds, in their order -> (A [N (N + 1) / 2],
    g [N], chi) as Python floats: 64 lane partials, round r adding every block's terms of points
    64 r + l in turn, then the butterfly."""
    N, n = blocks[0][0].shape
    if N not in _TRI:
        _TRI[N] = (np.array([i for i in range(N) for j in range(i + 1)]),
                   np.array([j for i in range(N) for j in range(i + 1)]))
    iu, ju = _TRI[N]
    NA = len(iu)
    R = (n + LANES - 1) // LANES
    acc = np.zeros((NA + N + 1, LANES))
    with np.errstate(all='ignore'):
        Ts = []
        for J, r in blocks:
            T = np.zeros((NA + N + 1, R * LANES))
            T[:NA, :n], T[NA:NA + N, :n], T[NA + N, :n] = J[iu] * J[ju], J * r, r * r
            Ts.append(T.reshape(NA + N + 1, R, LANES))
        for rd in range(R):
            valid = (rd * LANES + LANE) < n
            for T in Ts:
                acc = np.where(valid, acc + T[:, rd, :], acc)
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, LANE ^ m]
    col = acc[:, 0].tolist()
    return col[:NA], col[NA:NA + N], col[NA + N]


def step_ref(A, g, lam, p, lo, hi):
    """-> (trial or None, nfree): the Cholesky of lm_common.h step at len(p) parameters."""
    N = len(p)
    fr = [hi[i] > lo[i] and A[ix(i, i)] > 0.0 for i in range(N)]
    nf = sum(fr)
    L = [0.0] * len(A)
    for j in range(N):
        ajj = A[ix(j, j)]
        s = ajj + lam * ajj if fr[j] else 1.0
        for k in range(j):
            s = s - L[ix(j, k)] * L[ix(j, k)]
        if not (s > 0.0 and math.isfinite(s)):
            return None, nf
        d = math.sqrt(s)
        L[ix(j, j)] = d
        for i in range(j + 1, N):
            t = A[ix(i, j)] if fr[i] and fr[j] else 0.0
            for k in range(j):
                t = t - L[ix(i, k)] * L[ix(j, k)]
            L[ix(i, j)] = t / d
    y = [0.0] * N
    for i in range(N):
        t = g[i] if fr[i] else 0.0
        for k in range(i):
            t = t - L[ix(i, k)] * y[k]
        y[i] = t / L[ix(i, i)]
    for i in range(N - 1, -1, -1):
        t = y[i]
        for k in range(i + 1, N):
            t = t - L[ix(k, i)] * y[k]
        y[i] = t / L[ix(i, i)]
    return [clip(p[i] + y[i], lo[i], hi[i]) for i in range(N)], nf


def run_start_ref(p, lo, hi, sums, max_iter, ftol):
    """One start from p; sums(p) -> (A, g, chi), the model's combined sums -> (p, chi, evals, hit_max)."""
    A, g, chi = sums(p)
    evals = 1
    if not math.isfinite(chi):
        return p, chi, evals, 0
    lam = 1e-3
    while True:
        if evals >= max_iter:
            return p, chi, evals, 1
        trial, nfree = step_ref(A, g, lam, p, lo, hi)
        if trial is None:
            lam = lam * 10.0
            if lam > 1e12:
                return p, chi, evals, 0
            continue
        if nfree == 0:
            return p, chi, evals, 0
        A2, g2, chi2 = sums(trial)
        evals += 1
        if math.isfinite(chi2) and chi2 < chi:
            rel = (chi - chi2) / chi
            p, chi, A, g = trial, chi2, A2, g2
            lam = max(lam / 10.0, 1e-12)
            if rel <= ftol:
                return p, chi, evals, 0
        else:
            lam = lam * 10.0
            if lam > 1e12:
                return p, chi, evals, 0


def finish_ref(rec, status, best, trig):
    if status == 0 and best is None:
        status = _lib.LOOP_NO_FIT
    if status:
        rec['p'], rec['chisq'], rec['qc'], rec['qi'], rec['dipdb'] = NAN, NAN, NAN, NAN, NAN
        rec['best_start'], rec['evals'], rec['status'] = -1, 0, status
        return
    s, (p, chi, evals, hit) = best
    with np.errstate(all='ignore'):
        f = [np.float64(v) for v in p]
        rad = abs(f[6] + f[7]) / 4.0
        diam = (2.0 * rad) / (np.sqrt(f[8] * f[8] + f[9] * f[9]) + rad)
        rec['p'], rec['chisq'] = p, chi
        rec['qc'], rec['qi'] = f[0] / diam, f[0] / (1.0 - diam)
        rec['dipdb'] = 20.0 * np.float64(trig.log10(float(1.0 - diam)))
    rec['best_start'], rec['evals'], rec['status'] = s, evals, _lib.LOOP_MAX_ITER if hit else 0


def fit_ref(freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10, trig=EXACT):
    """The restatement of mkid_fit_loops -> (fits [nch] of FIT_DT, chisq_all [nch][S])."""
    freq, I, Q = (np.asarray(a, np.float64) for a in (freq, I, Q))
    nch, S = freq.shape[0], draws.shape[1]
    fits = np.zeros(nch, FIT_DT)
    call = np.full((nch, S), NAN)
    for c in range(nch):
        cidx, low, high, n = window_ref(I[c], Q[c])
        rec = fits[c]
        rec['cidx'], rec['low'], rec['high'], rec['n'] = cidx, low, high, n
        sl = slice(low, high)
        with np.errstate(all='ignore'):
            wI = np.ones(n) if isd is None else 1.0 / np.asarray(isd, np.float64)[c, sl]
            wQ = np.ones(n) if qsd is None else 1.0 / np.asarray(qsd, np.float64)[c, sl]
        win = (freq[c, sl], I[c, sl], Q[c, sl], wI, wQ)
        status, lo, hi, base = guesses_ref(*win, cidx - low, trig)
        best = None
        if status == 0:
            qg = None if qguess is None else float(qguess[c])
            for s in range(S):
                r = run_start_ref(start_ref(lo, hi, base, s, draws[c, s].tolist(), qg), lo, hi,
                                  lambda p: sums_ref(p, *win, trig), max_iter, ftol)
                call[c, s] = r[1]
                if math.isfinite(r[1]) and (best is None or r[1] < best[1][1]):
                    best = (s, r)
        finish_ref(rec, status, best, trig)
    return fits, call


# ---- the host twin ------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fit_host(freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10, nch=None, fsteps=None, S=None,
             null=(), want_all=True):
    """mkid_fit_loops_host -> (rc, fits, chisq_all); `null`: names of pointers passed as NULL."""
    L = _lib.load()
    a = {k: None if v is None else np.ascontiguousarray(v, np.float64)
         for k, v in dict(freq=freq, i=I, q=Q, isd=isd, qsd=qsd, draws=draws, qguess=qguess).items()}
    n0, f0 = a['freq'].shape
    nch = n0 if nch is None else nch
    fsteps = f0 if fsteps is None else fsteps
    S = a['draws'].shape[1] if S is None else S
    fits = np.zeros(max(n0, 1), FIT_DT)
    call = np.full((max(n0, 1), a['draws'].shape[1]), -7.0) if want_all else None
    a['fits'], a['call'] = fits, call
    q = {k: (None if k in null else _p(v)) for k, v in a.items()}
    rc = L.mkid_fit_loops_host(q['freq'], q['i'], q['q'], q['isd'], q['qsd'], q['draws'], q['qguess'], nch, fsteps, S,
                               max_iter, ftol, q['fits'], q['call'])
    return rc, fits, call


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def check_equal(got, ref, fields=INT_FIELDS + FLOAT_FIELDS):
    for k in fields:
        if k in FLOAT_FIELDS:
            assert same_bits(got[k], ref[k]), (k, got[k], ref[k])
        else:
            assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


# ---- synthetic loops ----------------------------------------------------------------------------------
def synth_loops(nch, fsteps, seed, noise=0.01, where='mid', sd=False, integer=False):
    """nch loops drawn as the numpy prototype of the solver's rules did: Q 15e3 .. 80e3, the sweep 4 .. 8 linewidths wide
    and offset by up to +-0.1 span (`where`: 'first' / 'last' put the resonance a quarter of the span
    from that end instead, so that the window is cut there), radius R, the centre 2 .. 5 R from the origin on both axes, aleak 0.01 ..
    0.3, ph1 100 .. 2000, da +-500, ang1 +-3, Gaussian noise of `noise` R on I and Q.
    -> dict(freq, I, Q [nch][fsteps], isd, qsd (or None), truth [nch][10], R [nch])."""
    rng = np.random.default_rng(seed)
    freq, I, Q = (np.zeros((nch, fsteps)) for _ in range(3))
    truth, Rs = np.zeros((nch, NP)), np.zeros(nch)
    for c in range(nch):
        Qr = rng.uniform(15e3, 80e3)
        f0 = rng.uniform(4.0e9, 6.0e9)
        span = rng.uniform(4.0, 8.0) * f0 / Qr
        off = rng.uniform(-0.1, 0.1) * span + {'mid': 0.0, 'first': 0.35, 'last': -0.35}[where] * span
        R = rng.uniform(2e3, 2e4)
        cen = rng.uniform(2.0, 5.0, 2) * R * rng.choice([-1.0, 1.0], 2)
        p = [Qr, f0, rng.uniform(0.01, 0.3), rng.uniform(100.0, 2000.0), rng.uniform(-500.0, 500.0),
             rng.uniform(-3.0, 3.0), 2.0 * R, 2.0 * R, cen[0], cen[1]]
        x = f0 + off + np.linspace(-0.5 * span, 0.5 * span, fsteps)
        z = roach.resdiff(x, *p)
        freq[c], truth[c], Rs[c] = x, p, R
        I[c] = z.real + noise * R * rng.standard_normal(fsteps)
        Q[c] = z.imag + noise * R * rng.standard_normal(fsteps)
    if integer:
        I, Q = np.rint(I), np.rint(Q)
    out = dict(freq=freq, I=I, Q=Q, isd=None, qsd=None, truth=truth, R=Rs)
    if sd:
        out['isd'] = noise * Rs[:, None] * rng.uniform(0.5, 2.0, (nch, fsteps))
        out['qsd'] = noise * Rs[:, None] * rng.uniform(0.5, 2.0, (nch, fsteps))
    return out


def draws_for(nch, S, seed):
    from mkids_sdr_amd import loopfit
    return loopfit.draws(nch, S, seed)


def _special(seed):
    """Three channels of 64 steps: a constant sweep, a NaN inside the window, a NaN outside it."""
    d = synth_loops(3, 64, seed)
    d['I'][0], d['Q'][0] = 1234.0, -567.0
    _, low1, high1, _ = window_ref(d['I'][1], d['Q'][1])
    d['freq'][1, (low1 + high1) // 2] = NAN           # frequencies do not move the window
    _, low2, high2, _ = window_ref(d['I'][2], d['Q'][2])
    out = 0 if low2 > 0 else 63
    assert not low2 <= out < high2
    d['freq'][2, out] = NAN
    return d


def _axis(seed):
    """One channel whose window midpoint in I is exactly 0 (integer samples less their half-integer
    midpoint: exact), so that Ioff's bounds coincide and the parameter is held fixed."""
    d = synth_loops(1, 65, seed, integer=True)
    _, low, high, _ = window_ref(d['I'][0], d['Q'][0])
    w = d['I'][0, low:high]
    mid = (w.max() + w.min()) / 2.0
    d['I'][0] = d['I'][0] - mid
    d['truth'][0, 8] -= mid
    w = d['I'][0, low:high]
    assert (w.max() - w.min()) / 2.0 + w.min() == 0.0
    return d


def _nofit(seed):
    """One channel whose frequencies are all 0 Hz: f0 is held at 0, dx = 0 / 0 is not a number, and
    no start reaches a finite chi^2, although every input is finite."""
    d = synth_loops(1, 25, seed)
    d['freq'][0] = 0.0
    return d


# name -> (data builder, S, qguess?, max_iter). Shapes: nch 1, 3, 65; fsteps 12 (the minimum), 13, 64, 65,
# 129, 1024 (ragged lane tails, several points a lane); S 1, 5, 10, 16 (waves with 0, 1, several starts).
CASES = {
    'min12':    (lambda: synth_loops(1, 12, 101), 1, False, 400),
    'odd13sd':  (lambda: synth_loops(3, 13, 102, sd=True), 5, False, 300),
    'first64':  (lambda: synth_loops(3, 64, 103, where='first'), 10, True, 30),
    'last65sd': (lambda: synth_loops(3, 65, 104, where='last', sd=True), 16, True, 30),
    'many24':   (lambda: synth_loops(65, 24, 105), 5, False, 30),
    'mid129':   (lambda: synth_loops(3, 129, 106), 10, False, 60),
    'big1024':  (lambda: synth_loops(1, 1024, 107, noise=0.001), 5, False, 30),
    'special':  (lambda: _special(108), 5, False, 30),
    'axis':     (lambda: _axis(109), 5, False, 300),
    'nofit':    (lambda: _nofit(110), 5, False, 30),
}
FTOL = 1e-10
_cache = {}


def case(name):
    """-> dict(data, draws, qguess, max_iter, ref=(fits, chisq_all), pert=(fits, chisq_all)), made once."""
    if name not in _cache:
        build, S, qg, max_iter = CASES[name]
        d = build()
        nch = d['freq'].shape[0]
        dr = draws_for(nch, S, 7000 + len(name) + nch)
        q = d['truth'][:, 0] * 1.2 if qg else None
        kw = dict(isd=d['isd'], qsd=d['qsd'], qguess=q, max_iter=max_iter, ftol=FTOL)
        ref = fit_ref(d['freq'], d['I'], d['Q'], dr, **kw)
        pert = fit_ref(d['freq'], d['I'], d['Q'], dr, trig=Trig(np.random.default_rng(31)), **kw)
        _cache[name] = dict(data=d, draws=dr, qguess=q, max_iter=max_iter, kw=kw, ref=ref, pert=pert)
    return _cache[name]


def comparable(ref, pert):
    """bool [nch]: channels whose parameters the device is compared in: the perturbed restatement
    keeps best_start, evals and the status."""
    return ((ref['best_start'] == pert['best_start']) & (ref['evals'] == pert['evals']) &
            (ref['status'] == pert['status']))


def chisq_of(fits, c, data, kw, trig=EXACT):
    """chi^2 of channel c's parameters `fits['p'][c]` by the restatement's model over its window."""
    low, high = int(fits['low'][c]), int(fits['high'][c])
    sl = slice(low, high)
    n = high - low
    wI = np.ones(n) if kw['isd'] is None else 1.0 / kw['isd'][c, sl]
    wQ = np.ones(n) if kw['qsd'] is None else 1.0 / kw['qsd'][c, sl]
    return chisq_ref(fits['p'][c].tolist(), data['freq'][c, sl], data['I'][c, sl], data['Q'][c, sl], wI, wQ, trig)


# The largest relative change per quantity between the restatement and its perturbed twin over the
# table (measure_bars(), rounded up to two digits; tests/test_loopfit_host.py holds the table to
# them), and the device's bars: ten times that, for a device function two ulp off and for the
# butterfly's interaction with an accept decision. ph1 (p3) is nearly free wherever aleak is small,
# which is why its figure is so much larger than the others'.
MEASURED = {'chisq': 2.0e-3, 'p0': 5.7e-8, 'p1': 4.3e-14, 'p2': 1.8e-5, 'p3': 0.11, 'p4': 1.7e-6, 'p5': 8.1e-9,
            'p6': 2.9e-8, 'p7': 6.9e-8, 'p8': 1.8e-8, 'p9': 8.6e-9, 'qc': 9.5e-8, 'qi': 3.7e-8, 'dipdb': 5.0e-8}
BARS = {k: 10.0 * v for k, v in MEASURED.items()}
MAX_EXCLUDED = 0.05   # of the table's channels


def rel_change(a, b):
    """max over elements of |a - b| / |b| (0 where both are equal, NaN included)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    with np.errstate(all='ignore'):
        r = np.abs(a - b) / np.abs(b)
    r[(a == b) | (np.isnan(a) & np.isnan(b))] = 0.0
    return float(np.max(r)) if r.size else 0.0


def measure_bars():
    """The largest relative change of every float quantity between the restatement and its perturbed
    twin over the comparable channels of the table -> dict by quantity (chisq over all channels)."""
    out = {k: 0.0 for k in ('chisq',) + tuple('p%d' % i for i in range(NP)) + ('qc', 'qi', 'dipdb')}
    for name in CASES:
        cs = case(name)
        ref, pert = cs['ref'][0], cs['pert'][0]
        ok = comparable(ref, pert) & (ref['status'] & FAIL_BITS == 0)
        fit = (ref['status'] & FAIL_BITS == 0) & (pert['status'] & FAIL_BITS == 0)
        out['chisq'] = max(out['chisq'], rel_change(pert['chisq'][fit], ref['chisq'][fit]))
        for i in range(NP):
            out['p%d' % i] = max(out['p%d' % i], rel_change(pert['p'][ok, i], ref['p'][ok, i]))
        for k in ('qc', 'qi', 'dipdb'):
            out[k] = max(out[k], rel_change(pert[k][ok], ref[k][ok]))
    return out
