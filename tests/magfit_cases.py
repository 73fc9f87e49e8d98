"""The float64 restatement of mkid_fit_mags (include/mkidgpu.h; the rules are csrc/magfit_common.h)
in numpy, the model-generated magnitude sweeps and the case table of tests/test_magfit_host.py and
tests/test_gpu_magfit.py.

The restatement does every operation of the header in the header's order. Elementwise numpy float64
arithmetic (+, -, x, /, sqrt, abs) is one IEEE operation per element and is never fused, so the
per-point terms are arrays over the sweep's points. The 64 lane partials are an array [28][64] (21
rows of A, 6 of g, chi^2) to which round r adds the terms of points 64 r + l, and the butterfly is
p = p + p[l ^ m]. The Cholesky and the iteration are scalar Python floats. The model calls no library
function, so the host twin and the device are held to the restatement bit for bit. The solver
(lane partials and butterfly, step, one start) and the velocity-maximum index are the loop fit's
restatements (loopfit_cases lane_sums_ref, step_ref, run_start_ref, window_ref).
"""
import ctypes
import math

import numpy as np

import loopfit_cases as lc
from mkids_sdr_amd import _lib, loopfit

NP = 6
FIT_DT = np.dtype(_lib.MAG_FIT_DTYPE)
INT_FIELDS = ('cidx', 'best_start', 'evals', 'status')
FLOAT_FIELDS = ('p', 'chisq', 'norm')
FAIL_BITS = _lib.LOOP_NONFINITE | _lib.LOOP_FLAT | _lib.LOOP_NO_FIT
NAN = float('nan')
W = 1.0 / 1e-5
Q_FAIL = 50000.0
clip, same_bits = lc.clip, lc.same_bits


# ---- the data -----------------------------------------------------------------------------------------
def data_ref(x, I, Q):
    """-> (nonfinite, norm, y [fsteps])."""
    nonfinite = not bool(np.all(np.isfinite(x)) and np.all(np.isfinite(I)) and np.all(np.isfinite(Q)))
    with np.errstate(all='ignore'):
        mag = np.sqrt(I * I + Q * Q)
        norm = float(mag[0])
        for v in mag[1:].tolist():
            if v > norm:
                norm = v
        return nonfinite, norm, mag / norm


def problem_ref(x, nonfinite, norm):
    """-> (status, lo[6], hi[6], f0 of the starts)."""
    xs = 0.0
    xmin = xmax = float(x[0])
    for v in x.tolist():
        xs = xs + v
        xmin, xmax = (v if v < xmin else xmin), (v if v > xmax else xmax)
    status = _lib.LOOP_NONFINITE if nonfinite else (_lib.LOOP_FLAT if norm == 0.0 else 0)
    with np.errstate(all='ignore'):
        f0 = float(np.float64(xs) / np.float64(len(x)))
    return status, [5e3, xmin, 1e-4, 0.01, -5e3, -1e8], [1e6, xmax, 1e2, 10.0, 5e3, 1e8], f0


def start_ref(lo, hi, f0, s, g):
    qt = 10000.0 * float(s) + 5000.0 * g
    p = [5000.0 if qt < 5000.0 else qt, f0, 1.0, 0.7, 0.1, -10.0]
    return [clip(p[i], lo[i], hi[i]) for i in range(NP)]


# ---- the model, the Jacobian, the sums ----------------------------------------------------------------
def terms_ref(p, x, y, w=W):
    """-> (m, res, J [6][n]) in the order of magfit_common.h point_terms."""
    Qp, f0, carrier, depth, slope, curve = p
    with np.errstate(all='ignore'):
        dx = (x - f0) / f0
        twoQ = 2.0 * Qp
        t = twoQ * dx
        den = 1.0 + t * t
        r = np.sqrt(den)
        a = np.abs(t) / r
        m = (((a - 1.0) * depth + carrier) + slope * dx) + (curve * dx) * dx
        res = (y - m) * w
        sg = (t > 0.0).astype(np.float64) - (t < 0.0).astype(np.float64)
        k = sg / (den * r)
        ddx = (-x) / (f0 * f0)
        dk = depth * k
        J = [w * (dk * (2.0 * dx)), w * (ddx * ((dk * twoQ + slope) + (2.0 * curve) * dx)), w + np.zeros_like(x),
             w * (a - 1.0), w * dx, w * (dx * dx)]
    return m, res, np.array(J)


def model_ref(p, x):
    x = np.asarray(x, np.float64)
    return terms_ref([float(v) for v in p], x, np.ones_like(x))[0]


def sums_ref(p, x, y):
    """-> (A [21], g [6], chi) as Python floats: a point adds one block of terms."""
    _, res, J = terms_ref(p, x, y)
    return lc.lane_sums_ref([(J, res)])


def fit_ref(freq, I, Q, draws, max_iter=200, ftol=1e-10):
    """The restatement of mkid_fit_mags -> (fits [nch] of FIT_DT, qout [nch], chisq_all [nch][S])."""
    freq, I, Q = (np.asarray(a, np.float64) for a in (freq, I, Q))
    nch, S = freq.shape[0], draws.shape[1]
    fits = np.zeros(nch, FIT_DT)
    qout = np.zeros(nch)
    call = np.full((nch, S), NAN)
    for c in range(nch):
        rec = fits[c]
        rec['cidx'] = lc.window_ref(I[c], Q[c])[0]
        nonfinite, norm, y = data_ref(freq[c], I[c], Q[c])
        rec['norm'] = norm
        status, lo, hi, f0 = problem_ref(freq[c], nonfinite, norm)
        best = None
        if status == 0:
            for s in range(S):
                r = lc.run_start_ref(start_ref(lo, hi, f0, s, float(draws[c, s])), lo, hi,
                                     lambda p: sums_ref(p, freq[c], y), max_iter, ftol)
                call[c, s] = r[1]
                if math.isfinite(r[1]) and (best is None or r[1] < best[1][1]):
                    best = (s, r)
            if best is None:
                status = _lib.LOOP_NO_FIT
        if status:
            rec['p'], rec['chisq'], rec['best_start'], rec['evals'], rec['status'] = NAN, NAN, -1, 0, status
            qout[c] = Q_FAIL
        else:
            s, (p, chi, evals, hit) = best
            rec['p'], rec['chisq'], rec['best_start'], rec['evals'] = p, chi, s, evals
            rec['status'] = _lib.LOOP_MAX_ITER if hit else 0
            qout[c] = p[0]
    return fits, qout, call


# ---- the host twin ------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fit_host(freq, I, Q, draws, max_iter=200, ftol=1e-10, nch=None, fsteps=None, S=None, null=(), want_all=True,
             want_q=True):
    """mkid_fit_mags_host into pre-filled outputs -> (rc, fits, qout, chisq_all); `null`: names of
    pointers passed as NULL."""
    L = _lib.load()
    a = {k: np.ascontiguousarray(v, np.float64) for k, v in dict(freq=freq, i=I, q=Q, draws=draws).items()}
    n0, f0 = a['freq'].shape
    nch = n0 if nch is None else nch
    fsteps = f0 if fsteps is None else fsteps
    S = a['draws'].shape[1] if S is None else S
    fits = np.frombuffer(bytearray(b'\x5a' * (n0 * FIT_DT.itemsize)), FIT_DT)
    qout = np.full(n0, -7.0) if want_q else None
    call = np.full((n0, a['draws'].shape[1]), -7.0) if want_all else None
    a.update(fits=fits, qout=qout, call=call)
    q = {k: (None if k in null else _p(v)) for k, v in a.items()}
    rc = L.mkid_fit_mags_host(q['freq'], q['i'], q['q'], q['draws'], nch, fsteps, S, max_iter, ftol, q['fits'], q['qout'],
                              q['call'])
    return rc, fits, qout, call


def check_equal(got, ref):
    for k in INT_FIELDS:
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in FLOAT_FIELDS:
        assert same_bits(got[k], ref[k]), (k, got[k], ref[k])


# ---- model-generated sweeps -----------------------------------------------------------------------------
def synth_mags(nch, fsteps, seed, noise=0.0, scale=3.0e4):
    """nch magnitude sweeps generated from the model itself, I = scale m (1 + noise gauss), Q = 0: Q
    15e3 .. 80e3, f0 4 .. 6 GHz, the sweep 4 .. 8 linewidths wide and offset by up to +-0.1 span,
    carrier 1, depth 0.3 .. 0.9, slope +-100, curve +-1e5. The fit sees m / max m, which leaves Q and
    f0 as they are. -> dict(freq, I, Q [nch][fsteps], truth [nch][6])."""
    rng = np.random.default_rng(seed)
    freq, I = np.zeros((nch, fsteps)), np.zeros((nch, fsteps))
    truth = np.zeros((nch, NP))
    for c in range(nch):
        Qr = rng.uniform(15e3, 80e3)
        f0 = rng.uniform(4.0e9, 6.0e9)
        span = rng.uniform(4.0, 8.0) * f0 / Qr
        off = rng.uniform(-0.1, 0.1) * span
        p = [Qr, f0, 1.0, rng.uniform(0.3, 0.9), rng.uniform(-100.0, 100.0), rng.uniform(-1e5, 1e5)]
        x = f0 + off + np.linspace(-0.5 * span, 0.5 * span, fsteps)
        freq[c], truth[c] = x, p
        I[c] = scale * model_ref(p, x) * (1.0 + noise * rng.standard_normal(fsteps))
    return dict(freq=freq, I=I, Q=np.zeros((nch, fsteps)), truth=truth)


def _loops(*a, **k):
    d = lc.synth_loops(*a, **k)
    return dict(freq=d['freq'], I=d['I'], Q=d['Q'], truth=None)


def _special(seed):
    """Three channels of 64 steps: an all-zero sweep (flat), a NaN in I (not finite), an ordinary one."""
    d = synth_mags(3, 64, seed)
    d['I'][0] = 0.0
    d['I'][1, 40] = NAN
    return d


def _nofit(seed):
    """All frequencies 0 Hz: f0 is held at 0, dx = 0 / 0 is not a number, and no start reaches a finite
    chi^2, although every input is finite."""
    d = synth_mags(1, 25, seed)
    d['freq'][0] = 0.0
    return d


def _samefreq(seed):
    """All frequencies equal: the bounds of f0 coincide and the parameter is held fixed."""
    d = synth_mags(1, 20, seed)
    d['freq'][0] = 5.0e9
    return d


def _cusp(seed):
    """An odd-length sweep on integer-Hz frequencies symmetric about the middle sample: the sum of x
    and its quotient are exact, so the starts' f0 is the middle sample itself, t = 0 is evaluated
    there and the sg = 0 rule is used."""
    d = synth_mags(1, 65, seed)
    mid = float(np.rint(d['truth'][0, 1]))
    x = mid + 20000.0 * np.arange(-32, 33)
    p = d['truth'][0].copy()
    p[0], p[1] = 4.0e4, mid + 3000.0
    d['freq'][0], d['truth'][0] = x, p
    d['I'][0] = 3.0e4 * model_ref(p, x)
    return d


# name -> (data builder, S, max_iter). Shapes: nch 1, 3, 65; fsteps 12 (the minimum), 13, 64, 65, 129,
# 1024 (ragged lane tails, several points a lane); S 1, 5, 10, 16 (waves with 0, 1, several starts).
# Half of the sets are model-generated (with and without noise), half lc.synth_loops; max_iter 30
# where the max-iter bit is wanted.
CASES = {
    'min12':    (lambda: synth_mags(1, 12, 201), 1, 400),
    'odd13':    (lambda: _loops(3, 13, 202), 5, 300),
    'model64':  (lambda: synth_mags(3, 64, 203, noise=1e-3), 10, 30),
    'loops65':  (lambda: _loops(3, 65, 204), 16, 30),
    'many24':   (lambda: _loops(65, 24, 205), 5, 30),
    'mid129':   (lambda: synth_mags(3, 129, 206), 10, 200),
    'loop1024': (lambda: _loops(1, 1024, 207, noise=0.001), 5, 30),
    'big1024':  (lambda: synth_mags(1, 1024, 208, noise=1e-3), 5, 200),
    'special':  (lambda: _special(209), 5, 200),
    'nofit':    (lambda: _nofit(210), 5, 30),
    'samefreq': (lambda: _samefreq(211), 5, 200),
    'cusp':     (lambda: _cusp(212), 5, 200),
}
FTOL = 1e-10
_cache = {}


def case(name):
    """-> dict(data, draws, max_iter, kw, ref=(fits, qout, chisq_all)), made once."""
    if name not in _cache:
        build, S, max_iter = CASES[name]
        d = build()
        nch = d['freq'].shape[0]
        dr = loopfit.mag_draws(nch, S, 8000 + len(name) + nch)
        kw = dict(max_iter=max_iter, ftol=FTOL)
        _cache[name] = dict(data=d, draws=dr, max_iter=max_iter, kw=kw, ref=fit_ref(d['freq'], d['I'], d['Q'], dr, **kw))
    return _cache[name]
