"""The pulse-height fit on the CPU (include/mkidgpu.h mkid_pulse_fit; no GPU): tests/fit_ref.py, the
float64 numpy restatement, against a plain double loop; mkid_pulse_fit_host, which runs the
definitions of csrc/fit_common.h that the kernel runs, against the restatement over the case table
at both polarities; an exact integer case with tied lags; every MKID_E_ARG case; and the science
check on the CPU chain.

Science check (test_fit_beats_plain_on_cpu_chain): noise-free 60 degree pulses at uniform sub-row
offsets through the float64 oracle chain and the oracle trigger, per-channel filters from the mean
of the channel's own pulse windows. Only isolated pulses with exactly one packet count (a second
pulse inside the window changes the height for either estimator). The trigger stamps a pulse about
33 rows after its start, so the window is placed by mkid_optimal_filter's rule, 10 rows before the
peak of the average pulse, which gives pre = 31. Measured on the CPU, 64 channels, 2^22 samples,
957 packets, ncoeff 100, L 3, none at the edge of the search (DESIGN.md has the same numbers):
    spread of h0 / channel median     5.27e-03       spread of the fitted height   1.45e-03
    std of jg - start / N (rows)      0.2815         std of jg + dt - start / N    0.0761
"""
import ctypes

import numpy as np
import pytest

import fit_ref
import signals
from mkids_sdr_amd import _lib, codecs
from oracle import trigger as otrig


def _loop(phase, events, coeff, pre, L, s, j0):
    """The rule of the issue as a plain double loop, without numpy reductions."""
    out = []
    for w in events.tolist():
        ch, ts = w >> 52, w & fit_ref.TS_MASK
        base = max(j0 - (1 << 27), 0)
        jg = base + ((ts - (base & fit_ref.TS_MASK)) & fit_ref.TS_MASK)
        r0 = jg - j0 - pre
        nco = coeff.shape[1]
        if ch >= phase.shape[1] or r0 - L < 0 or r0 + L + nco > phase.shape[0]:
            out.append((np.nan, np.nan, fit_ref.NO_LAG, np.nan))
            continue
        H = [sum(float(coeff[ch, i]) * float(phase[r0 + d + i, ch]) for i in range(nco)) for d in range(-L, L + 1)]
        k = 0
        for i in range(1, 2 * L + 1):
            if s * H[i] > s * H[k]:
                k = i
        if k in (0, 2 * L):
            out.append((H[k], float(k - L), k - L, H[L]))
            continue
        y1, y2, y3 = s * H[k - 1], s * H[k], s * H[k + 1]
        a, b = y2 - y1, y2 - y3
        c = a + b
        if c == 0:
            out.append((H[k], float(k - L), k - L, H[L]))
        else:
            out.append((s * (y2 + (a - b) ** 2 / (8 * c)), k - L + (a - b) / (2 * c), k - L, H[L]))
    return [np.array(x) for x in zip(*out)]


@pytest.mark.parametrize('j0', [0, 1000, (1 << 28) - 7, 3 << 28])
def test_fit_ref_matches_loop(j0):
    rng = np.random.default_rng(5)
    rows, C, nco, pre, L = 300, 8, 20, 6, 2
    phase = rng.normal(size=(rows, C)).astype(np.float32)
    coeff = rng.normal(size=(C, nco))
    ts = j0 + np.array([0, 7, 8, 9, 50, 200, 283, 284, 285, 299, 320] + list(range(100, 140)))
    ch = rng.integers(0, C, ts.size)
    ch[5] = C + 3
    ev = np.array([fit_ref.pack(c, t) for c, t in zip(ch, ts)], np.uint64)
    for s in (1, -1):
        want = _loop(phase, ev, coeff, pre, L, s, j0)
        got = fit_ref.pulse_fit(phase, ev, coeff, pre, L, s, j0)[:4]
        nan = np.isnan(want[0])
        # windows that start before row 0 (ts 0, 7), end past the rows (285, 299, 320), channel >= C
        assert nan.sum() == 6
        assert np.array_equal(want[2], got[2])
        for a, b in zip(want, got):
            assert np.array_equal(np.isnan(a.astype(float)), nan) or a.dtype.kind == 'i'
            assert np.allclose(a[~nan], b[~nan], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('s', [1, -1])
@pytest.mark.parametrize('ncoeff,pre,L', fit_ref.CASES)
def test_host_call_matches_restatement(ncoeff, pre, L, s):
    phase, coeff, ev = fit_ref.inputs(ncoeff, pre, L)
    ref = fit_ref.reference(ncoeff, pre, L, s)
    got = codecs.pulse_fit_host(phase, ev, coeff, pre, search=L, polarity=s)
    H, A = ref[4], ref[5]
    bar = fit_ref.bar64(A, ncoeff)
    fit_ref.check_against(ref, got, bar, L, s)
    # where the best lag leads the second best by more than the rounding, the lags are equal
    ok = np.flatnonzero(~np.isnan(ref[0]))
    if L > 0:
        y = np.sort(s * H[ok], axis=1)
        clear = y[:, -1] - y[:, -2] > 2 * bar[ok]
        assert clear.mean() > 0.99
        assert np.array_equal(got[2][ok][clear], ref[2][ok][clear])
    else:
        assert np.all(got[2][ok] == 0)


def test_exact_ties():
    """Integer inputs, every sum exact: the host call equals the restatement bit for bit, the lowest
    of tied lags is chosen, an all-equal search ends at its edge, and L = 0 is the plain height.
    (With the lowest lag chosen, y1 < y2 at an interior lag, so c = 0 needs a non-finite value.)"""
    phase, coeff, ev, pre, L = fit_ref.exact_case()
    for s in (1, -1):
        ref = fit_ref.pulse_fit(phase, ev, coeff, pre, L, s)
        got = codecs.pulse_fit_host(phase, ev, coeff, pre, search=L, polarity=s)
        for a, b in zip(ref[:4], got):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
        H = ref[4]
        ok = ~np.isnan(ref[0])
        y = s * H[ok]
        ties = (y == y.max(axis=1, keepdims=True)).sum(axis=1) > 1
        assert ties.sum() > 20
        assert np.array_equal(got[2][ok], np.argmax(y, axis=1) - L)     # argmax: the first maximum
    h, dt, lag, h0 = codecs.pulse_fit_host(phase, ev, coeff, pre, search=L, polarity=1)
    ch, jg = fit_ref.unwrap(ev, 0)
    const = ch == 1                      # constant phase: every lag ties, the lowest is the edge
    assert np.all(lag[const] == -L) and np.all(dt[const] == -L) and np.all(h[const] == h0[const])
    flat = (ch == 2) & (jg == 61)        # H = 0 0 5 5 0 0 0 around the second row of the flat top
    assert lag[flat] == -1 and h0[flat] == 5 and h[flat] == 5 + 25 / 40 and dt[flat] == -0.5
    h, dt, lag, h0 = codecs.pulse_fit_host(phase, ev, coeff, pre, search=0, polarity=-1)
    ok = ~np.isnan(h)
    assert ok.sum() > 100 and np.all(lag[ok] == 0) and np.all(dt[ok] == 0) and np.array_equal(h[ok], h0[ok])
    plain = fit_ref.pulse_fit(phase, ev, coeff, pre, 0, -1)
    assert np.array_equal(h, plain[0], equal_nan=True)


def test_host_call_argument_errors():
    L = _lib.load()
    ph = np.zeros((50, 4), np.float32)
    cf = np.ones((4, 5), np.float32)
    ev = np.array([fit_ref.pack(1, 20)], np.uint64)
    h, dt, h0 = np.zeros(1), np.zeros(1), np.zeros(1)
    lag = np.zeros(1, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(phase=ph, rows=50, C=4, j0=0, events=ev, n=1, coeff=cf, ncoeff=5, pre=2, search=3, polarity=-1,
             heights=h, dt_=dt, lag_=lag, h0_=h0):
        return L.mkid_pulse_fit_host(p(phase), rows, C, j0, p(events), n, p(coeff), ncoeff, pre, search, polarity,
                                     p(heights), p(dt_), p(lag_), p(h0_))

    assert call() == _lib.MKID_OK and h[0] == 5 * 0.0 and lag[0] == -3
    assert call(dt_=None, lag_=None, h0_=None) == _lib.MKID_OK          # the nullable outputs
    assert call(rows=0, phase=None) == _lib.MKID_OK and np.isnan(h[0])  # no rows: nothing is inside
    assert call(n=0, events=None, heights=None) == _lib.MKID_OK
    bad = [dict(phase=None), dict(events=None), dict(heights=None), dict(coeff=None), dict(rows=-1), dict(j0=-1),
           dict(n=-1), dict(C=0), dict(C=4097), dict(ncoeff=0), dict(ncoeff=4097), dict(pre=-1), dict(search=-1),
           dict(search=32), dict(polarity=0), dict(polarity=2)]
    for kw in bad:
        assert call(**kw) == _lib.MKID_E_ARG, kw


def _chain_packets(C, S, seed):
    """Noise-free pulses through the oracle chain with the loops rotated to phase 0, thresholds at a
    tenth of the pulse amplitude: (case, phase [J][C], packets)."""
    kw = dict(seed=seed, noise=0, amp_deg=(60.0, 60.0))
    quiet = signals.make_case(C, S // 4, pulses_per_ch=0, **kw)
    y = signals.oracle_chain(quiet).process(quiet.iq)['y']
    phi = np.angle(y[64:].mean(axis=0))
    case = signals.make_case(C, S, pulses_per_ch=40.0, dds_phase=phi, **kw)
    out = signals.oracle_chain(case).process(case.iq)
    thr = np.full(C, -int(np.deg2rad(6.0) * 8192), np.int64)
    ev, _, _ = otrig.Trigger(C, case.fir12, thr).run(out['raw'].astype(np.int64))
    return case, out['phase'].astype(np.float32), np.asarray(ev, np.uint64)


def test_fit_beats_plain_on_cpu_chain():
    C, S, nco, L = 64, 1 << 22, 100, 3
    case, phase, ev = _chain_packets(C, S, seed=31)
    N, rows = case.N, phase.shape[0]
    m = signals.match_pulses(ev, case.pulses, N)
    assert m['isolated'] > 500 and m['exactly_one'] >= 0.95 * m['isolated'], m
    # per packet: the isolated pulse it matches (match_pulses' window and isolation), if any
    ch, jg = fit_ref.unwrap(ev, 0)
    starts = {}
    for s0, c, _ in case.pulses:
        starts.setdefault(int(c), []).append(int(s0))
    keep, start = [], []
    for c, st in starts.items():
        st = np.sort(np.array(st))
        r = st // N
        iso = np.ones(r.size, bool)
        iso[1:] &= np.diff(r) >= 400
        iso[:-1] &= np.diff(r) >= 400
        mine = np.flatnonzero(ch == c)
        for k in np.flatnonzero(iso):
            hit = mine[(jg[mine] >= r[k] - 2) & (jg[mine] <= r[k] + 60)]
            if hit.size == 1 and 200 <= jg[hit[0]] < rows - 200:
                keep.append(hit[0])
                start.append(st[k])
    keep, start = np.array(keep), np.array(start, np.float64)
    assert keep.size > 500
    # The trigger stamps a pulse well after its rise (the delay of the low-pass and the matched
    # filter), so the window is placed by the library's own rule (mkid_optimal_filter): the weights
    # start 10 rows before the peak of the average pulse.
    back = 100
    mean_pulse = np.mean([phase[jg[i] - back:jg[i] + 50, ch[i]].astype(np.float64) for i in keep], axis=0)
    pre = back - int(np.argmin(mean_pulse)) + 10
    assert 10 < pre < back
    # each channel's filter: the mean window of its own pulses, mean removed, sign-flipped to the
    # positive template of template.matched_fir_taps' convention, unit response to the mean window
    coeff = np.zeros((C, nco), np.float32)
    for c in range(C):
        k = keep[ch[keep] == c]
        assert k.size >= 3
        avg = np.mean([phase[jg[i] - pre:jg[i] - pre + nco, c].astype(np.float64) for i in k], axis=0)
        t = -(avg - avg.mean())
        coeff[c] = t / np.dot(t, t)
    h, dt, lag, h0 = codecs.pulse_fit_host(phase, ev[keep], coeff, pre, search=L, polarity=-1)
    assert np.all(np.isfinite(h))
    med = lambda x: np.array([np.median(x[ch[keep] == c]) for c in range(C)])[ch[keep]]
    spread_plain, spread_fit = np.std(h0 / med(h0)), np.std(h / med(h))
    arrival = start / N
    t_plain, t_fit = np.std(jg[keep] - arrival), np.std(jg[keep] + dt - arrival)
    print('pre %d; spread plain %.4e fitted %.4e; arrival std plain %.4f fitted %.4f rows; %d packets, '
          '%d at the edge of the search' % (pre, spread_plain, spread_fit, t_plain, t_fit, keep.size,
                                            int(np.sum(np.abs(lag) == L))))
    assert spread_fit < spread_plain
    assert t_fit < t_plain
