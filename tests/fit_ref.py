"""Float64 restatement of the pulse-height fit (include/mkidgpu.h mkid_pulse_fit) in plain numpy —
TEST INFRASTRUCTURE, the reference of test_fit_host.py and test_gpu_fit.py.

Per wide packet (channel at bit 52, 28-bit stamp unwrapped into [j0 - 2^27, j0 + 2^27) as
oracle/heights.py does), with r0 = jg - j0 - pre, the lag values
    H[d] = sum_i coeff[ch][i] * phase[r0 + d + i][ch],  d = -L .. L
in float64, the lowest lag that maximises s H, and around an interior lag codecs.peakfit (pinned to
the reference's own vectors) for the height and the vertex formula, applied literally, for dt.
Packets whose rows r0 - L .. r0 + L + ncoeff - 1 are not all inside the rows, or whose channel the
phase does not have, get NaN and INT32_MIN.
"""
import numpy as np

from mkids_sdr_amd import codecs

CH_SHIFT = 52
TS_MASK = (1 << 28) - 1
NO_LAG = np.iinfo(np.int32).min


def pack(ch, ts):
    return np.uint64((int(ch) << CH_SHIFT) | (int(ts) & TS_MASK))


def unwrap(events, j0):
    """(channel, unwrapped stamp jg) of wide packets, int64 each."""
    ev = np.asarray(events, np.uint64)
    ch = ((ev >> np.uint64(CH_SHIFT)) & np.uint64(0xFFF)).astype(np.int64)
    ts = (ev & np.uint64(TS_MASK)).astype(np.int64)
    base = max(int(j0) - (1 << 27), 0)
    return ch, base + ((ts - (base & TS_MASK)) & TS_MASK)


def lag_values(phase, events, coeff, pre, L, j0=0):
    """H float64 [n][2 L + 1] (NaN rows for packets outside) and A [n] = max_d sum_i |coeff_i
    phase[r0 + d + i]|, the magnitude the rounding bars scale with."""
    phase = np.asarray(phase)
    coeff = np.asarray(coeff, np.float64)
    rows, C = phase.shape
    nco = coeff.shape[1]
    ch, jg = unwrap(events, j0)
    H = np.full((ch.size, 2 * L + 1), np.nan)
    A = np.full(ch.size, np.nan)
    for p in range(ch.size):
        r0 = int(jg[p]) - j0 - pre
        if ch[p] >= C or r0 - L < 0 or r0 + L + nco > rows:
            continue
        w = phase[r0 - L:r0 + L + nco, ch[p]].astype(np.float64)
        H[p] = np.correlate(w, coeff[ch[p]], 'valid')
        A[p] = np.correlate(np.abs(w), np.abs(coeff[ch[p]]), 'valid').max()
    return H, A


def fit_lags(H, L, s):
    """(heights, dt, lag, h0) from lag values H [n][2 L + 1]; NaN rows give NaN / NO_LAG."""
    n = H.shape[0]
    heights, dt, h0 = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    lag = np.full(n, NO_LAG, np.int32)
    for p in range(n):
        if np.isnan(H[p, 0]):
            continue
        y = s * H[p]
        k = int(np.argmax(y))                 # the first of equal maxima: the lowest lag
        lag[p], h0[p] = k - L, H[p, L]
        if k == 0 or k == 2 * L:
            heights[p], dt[p] = H[p, k], k - L
            continue
        y1, y2, y3 = y[k - 1], y[k], y[k + 1]
        a, b = y2 - y1, y2 - y3
        c = a + b
        heights[p] = s * codecs.peakfit(y1, y2, y3)
        dt[p] = (k - L) if c == 0 else (k - L) + (a - b) / (2 * c)
    return heights, dt, lag, h0


def pulse_fit(phase, events, coeff, pre, L, s, j0=0):
    """(heights, dt, lag, h0, H, A) of the restatement."""
    H, A = lag_values(phase, events, coeff, pre, L, j0)
    return fit_lags(H, L, s) + (H, A)


def check_against(ref, got, bar, L, s, max_skipped=0.01):
    """The issue's assertions 1-5 on a device (or host) result `got` = (heights, dt, lag, h0) against
    `ref` = pulse_fit(...) with per-packet rounding bars `bar`. Returns (interior, skipped)."""
    rh, rdt, rlag, rh0, H, _ = ref
    gh, gdt, glag, gh0 = (np.asarray(x) for x in got)
    out = np.isnan(rh)
    # 5. the NaN / INT32_MIN pattern
    assert np.array_equal(np.isnan(gh), out) and np.array_equal(np.isnan(gdt), out)
    assert np.array_equal(np.isnan(gh0), out) and np.array_equal(glag == NO_LAG, out)
    ok = np.flatnonzero(~out)
    assert ok.size > 20
    interior = skipped = 0
    for p in ok:
        y = s * H[p]
        k = int(glag[p]) + L
        assert 0 <= k <= 2 * L
        b_ = bar[p]
        assert y[k] >= y.max() - 2 * b_, (p, 'lag not near-maximal')                       # 1
        assert abs(gh0[p] - H[p, L]) <= b_, (p, 'h0')                                      # 2
        if k == 0 or k == 2 * L:                                                          # 3
            assert abs(gh[p] - H[p, k]) <= b_, (p, 'edge height')
            assert gdt[p] == glag[p], (p, 'edge dt')
            continue
        interior += 1                                                                     # 4
        assert abs(gdt[p] - glag[p]) <= 0.5, (p, 'dt outside the half row')
        a, b = y[k] - y[k - 1], y[k] - y[k + 1]
        c64 = a + b
        if c64 >= 16 * b_:
            h64 = s * codecs.peakfit(y[k - 1], y[k], y[k + 1])
            dt64 = (k - L) + (a - b) / (2 * c64)
            assert abs(gh[p] - h64) <= 4 * b_, (p, 'height', gh[p], h64, b_)
            assert abs(gdt[p] - dt64) <= 4 * b_ / c64 + 1e-6, (p, 'dt', gdt[p], dt64)
        else:
            skipped += 1
            assert abs(gh[p] - H[p, k]) <= c64 / 8 + 2 * b_, (p, 'flat-top height')
    assert skipped <= max_skipped * max(interior, 1), (skipped, interior)
    return interior, skipped


# ---- shared inputs of test_fit_host.py and test_gpu_fit.py ---------------------------------------
# (ncoeff, pre, L): 2 L + 1 in {1, 3, 5, 7, 17, 63} covers lane groups that divide the wave and
# groups that do not; ncoeff sits around multiples of 64 and of G = 64 // (2 L + 1)
CASES = [(1, 0, 1), (5, 1, 2), (63, 12, 3), (64, 12, 0), (65, 13, 3), (100, 20, 3), (128, 20, 31), (800, 100, 8),
         (4096, 20, 2)]
C_TEST = 64
_inputs = {}


def inputs(ncoeff, pre, L, n=3000):
    """(phase float32 [rows][64], coeff float32 [64][ncoeff], events uint64 [n]) of a case, made
    once: normal phase and coefficients, packets at random channels and stamps over all the rows (so
    some search windows leave the rows at either end) and a few on channels the context lacks."""
    key = (ncoeff, pre, L)
    if key not in _inputs:
        rng = np.random.default_rng(1000 + 7 * ncoeff + L)
        rows = max(3 * ncoeff, 600) + 200
        phase = rng.normal(size=(rows, C_TEST)).astype(np.float32)
        coeff = rng.normal(size=(C_TEST, ncoeff)).astype(np.float32)
        ch = rng.integers(0, C_TEST, n)
        ch[::500] = C_TEST + rng.integers(0, 100, ch[::500].size)
        ts = rng.integers(0, rows, n)
        ts[1:40:2] = rng.integers(0, pre + L + 2, ts[1:40:2].size)              # around the first rows
        ts[2:40:2] = rows - rng.integers(0, ncoeff - min(pre, ncoeff) + L + 2, ts[2:40:2].size) - 1
        ev = np.array([pack(c, t) for c, t in zip(ch, ts)], np.uint64)
        _inputs[key] = (phase, coeff, ev)
    return _inputs[key]


_refs = {}


def reference(ncoeff, pre, L, s):
    """pulse_fit of a case's inputs, computed once and shared (treat as read-only)."""
    key = (ncoeff, pre, L, s)
    if key not in _refs:
        phase, coeff, ev = inputs(ncoeff, pre, L)
        hk = (ncoeff, pre, L, 'H')
        if hk not in _refs:
            _refs[hk] = lag_values(phase, ev, coeff.astype(np.float64), pre, L)
        H, A = _refs[hk]
        _refs[key] = fit_lags(H, L, s) + (H, A)
    return _refs[key]


def bar32(A, ncoeff):
    """fp32 accumulation of ncoeff products in any order is within ncoeff 2^-24 sum |c x| of the
    exact sum; 1e-5 is the project's bar for at most 128 products (test_heights.py)."""
    return max(1e-5, ncoeff * 2.0 ** -24) * A + 1e-6


def bar64(A, ncoeff):
    return ncoeff * 2.0 ** -53 * A + 1e-12


def exact_case():
    """Integer-valued phase and small integer coefficients: every sum is exact in fp32 and float64.
    Returns (phase [rows][4], coeff [4][5], events, pre, L). Channel 0 is random small integers (lags
    tie often), channel 1 a constant (all lags tie), channel 2 zero but for a flat top of two rows
    under a one-tap filter, channel 3 random again."""
    rng = np.random.default_rng(77)
    rows, nco, pre, L = 120, 5, 2, 3
    phase = rng.integers(-3, 4, size=(rows, 4)).astype(np.float32)
    phase[:, 1] = 2.0
    phase[:, 2] = 0.0
    phase[60:62, 2] = 5.0
    coeff = rng.integers(-2, 3, size=(4, nco)).astype(np.float32)
    coeff[2] = (0, 0, 1, 0, 0)      # H[d] = phase[ts + d] on channel 2
    ev = [pack(c, t) for c in (0, 3) for t in range(0, rows)]
    ev += [pack(1, t) for t in (10, 50, 90)]
    ev += [pack(2, t) for t in range(52, 70)]
    return phase, coeff, np.array(ev, np.uint64), pre, L
