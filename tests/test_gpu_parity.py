"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs.

Bars: phase within 1e-5 rad of the float64 oracle on every tone channel at every
sample where |y - c| >= the IQ floor F = IQ_TOL_REL / PHASE_TOL * |y|max (|y|max: the feedline's
strongest tone); below it the phase of y - c is ill-conditioned in any precision (the stream's
start-up, where y ramps from 0 through the loop centre; noise on a small loop), and the device is
held to the absolute IQ bar |dphi| |y - c| <= IQ_TOL_REL |y|max instead; Fix16_13 phase within 1 LSB (rounding-boundary flips only, rare); photon packets bit-exact —
both the full chain vs the oracle chain, and the device trigger vs the oracle trigger fed the
device's own Fix16_13 phase.
"""
import numpy as np
import pytest

import signals
from oracle import trigger as otrig

pytestmark = pytest.mark.gpu

PHASE_TOL = 1e-5
# absolute IQ error bar below the IQ floor, relative to the feedline's strongest tone |y| (the
# comb's full-scale level). Measured (rounds 5-6): the device's y - c differs from the
# float64 oracle's by <= 5e-8 |y|max on weak channels (the FFT's comb-level rounding), so the bar
# leaves a 2x margin and puts the floor at F = IQ_TOL_REL / PHASE_TOL |y|max = 0.01 |y|max.
IQ_TOL_REL = 1e-7
# rows after a reset until every tap of the chain sees stream samples: frame k is complete from
# k = 2T - 1 = 7, output row j reads frames 2j + 1 - 25 .. 2j + 1, so j >= 16 (reporting only)
SETTLE_ROWS = 16


def configure(ch, case, thr, mode=1):
    ch.set_pfb(case.pfb)
    ch.set_bins(case.bins)
    ch.set_dds(case.lut_i, case.lut_q)
    ch.set_lpf(case.lpf12)
    ch.set_fir(case.fir12)
    ch.set_centers(case.ic, case.qc)
    ch.set_thresholds(thr)
    ch.set_baseline(mode, 41, 82, 93623, 8192)


def quiet_thresholds(C, S, seed):
    q = signals.make_case(C, S, seed=seed, pulses_per_ch=0)
    r = signals.oracle_chain(q).process(q.iq)
    return signals.thresholds_from_quiet(q, r['raw'])


def sort_events(ev):
    ev = np.asarray(ev, np.uint64)
    key = (ev >> np.uint64(52)) * np.uint64(1 << 28) + (ev & np.uint64((1 << 28) - 1))
    return ev[np.argsort(key, kind='stable')]


def split_by_channel(ev):
    out = {}
    for w in sort_events(ev):
        out.setdefault(int(w) >> 52, []).append(int(w))
    return out


def run_gpu(case, thr, splits, mode=1, max_chunk=None, dead=32, front='auto', acc=True):
    """acc: arm the avgIQ accumulator (the front ends' accumulating variants: k_front5<true>, the
    y-sum stores of k_front / k_front3) and return its means; False runs the streaming variants
    bench.py times and returns None for the means."""
    from mkids_sdr_amd.channelizer import Channelizer
    S = case.iq.shape[0]
    ch = Channelizer(case.C, max_chunk=max_chunk or S, dead_time=dead, front=front)
    try:
        configure(ch, case, thr, mode)
        if acc:
            ch.set_accumulator(True)
        phases, evs = [], []
        for a, b in zip(splits[:-1], splits[1:]):
            ph, ev = ch.process(case.iq[a:b])
            phases.append(ph)
            evs.append(ev)
        means = ch.avg_iq() if acc else None
    finally:
        ch.close()
    return np.concatenate(phases), np.concatenate(evs), means


_CASES, _ORACLE = {}, {}


def cached_case(C, S, seed, pulses_per_ch):
    """make_case + quiet thresholds, shared by the parametrisations that differ only in the
    front end (the host-side case and oracle dominate the suite's time at 1024/2048 channels)."""
    key = (C, S, seed, pulses_per_ch)
    if key not in _CASES:
        while len(_CASES) >= 3:                 # keep the last few cases (tens of MB each)
            old = _CASES.pop(next(iter(_CASES)))
            _ORACLE.pop(id(old[0]), None)
        _CASES[key] = (signals.make_case(C, S, seed=seed, pulses_per_ch=pulses_per_ch),
                       quiet_thresholds(C, min(S, 2 * C * 2048), seed))
    return _CASES[key]


def oracle_of(case):
    if id(case) not in _ORACLE:
        if not any(c[0] is case for c in _CASES.values()):
            return signals.oracle_chain(case).process(case.iq)   # uncached case
        _ORACLE[id(case)] = (case, signals.oracle_chain(case).process(case.iq))
    return _ORACLE[id(case)][1]


def compare(case, thr, splits, mode=1, max_chunk=None, dead=32, expect_events=True, front='auto',
            phase_tol=None, report=None, acc=True):
    """phase_tol: per-channel phase bar [C] (default PHASE_TOL everywhere); report: a dict that
    receives the per-channel max phase error ('err') and Fix16_13 flip counts ('flips')."""
    r = oracle_of(case)
    tr = otrig.Trigger(case.C, case.fir12, thr, mode=mode, dead=dead)
    ev_o, n_o, _ = tr.run(r['raw'])
    ph_g, ev_g, _ = run_gpu(case, thr, splits, mode, max_chunk, dead, front, acc)

    assert ph_g.shape == r['phase'].shape
    tones = slice(0, case.n_tones)
    err = np.abs(signals.wrap(ph_g[:, tones].astype(np.float64) - r['phase'][:, tones]))
    raw_g = np.clip(np.rint(ph_g * np.float32(8192)), -25736, 25736).astype(np.int64)
    draw = np.abs(raw_g[:, tones] - r['raw'][:, tones].astype(np.int64))
    y_o = r['y'][:, tones]
    ymc = np.abs(y_o - (case.ic[tones].astype(np.float64) + 1j * case.qc[tones].astype(np.float64)))
    ymax = float(np.median(np.abs(y_o[SETTLE_ROWS:]), axis=0).max())
    iq_tol = IQ_TOL_REL * ymax
    if report is not None:
        report.update(err=err.max(axis=0), flips=(draw > 0).sum(axis=0), rows=err.shape[0], err_rows=err,
                      ymc=ymc, ymax=ymax)
    held = ymc >= iq_tol / PHASE_TOL                      # above the IQ floor
    tol = PHASE_TOL if phase_tol is None else np.asarray(phase_tol, np.float64)[tones][None, :]
    bad = held & (err >= tol)
    assert not bad.any(), 'phase error %.3g rad (%d channels over the bar)' % (
        err[held].max(), bad.any(axis=0).sum())
    low = ~held & (err >= tol)                              # below it: the absolute IQ bar
    assert not (low & (err * ymc > iq_tol)).any(), 'IQ error %.3g of |y|max below the floor' % (
        (err * ymc)[low].max() / ymax)

    assert draw.max() <= 1
    assert (draw > 0).mean() < 5e-3

    # device trigger == oracle trigger on the device's own Fix16_13 phase (exact integer path)
    tr2 = otrig.Trigger(case.C, case.fir12, thr, mode=mode, dead=dead)
    ev_same, _, _ = tr2.run(raw_g.astype(np.int16))
    assert np.array_equal(sort_events(ev_g), sort_events(ev_same))
    # full chain: GPU packets == oracle-chain packets, channel by channel. The only admissible
    # difference is downstream of a Fix16_13 rounding-boundary flip (fp32 vs float64 phase that
    # straddles a half-LSB): a channel may differ only at or after its first flipped sample.
    g_by, o_by = split_by_channel(ev_g), split_by_channel(ev_o)
    n_diff_ch = 0
    for c in range(case.C):
        a, b = g_by.get(c, []), o_by.get(c, [])
        if a == b:
            continue
        n_diff_ch += 1
        flips = np.nonzero(raw_g[:, c] != r['raw'][:, c].astype(np.int64))[0]
        assert flips.size, 'channel %d packets differ with identical Fix16_13 phase' % c
        first_diff = next(i for i in range(min(len(a), len(b)) + 1)
                          if i >= len(a) or i >= len(b) or a[i] != b[i])
        t_diff = min([(w & ((1 << 28) - 1)) for w in (a[first_diff:first_diff + 1] +
                                                     b[first_diff:first_diff + 1])])
        assert t_diff + 1 >= flips[0], 'channel %d differs before its first phase flip' % c
    # statistical sanity bound only: every differing channel was checked above to differ
    # downstream of its own Fix16_13 rounding flip
    assert n_diff_ch <= max(2, case.C // 100)
    if expect_events:
        assert n_o > 0
    return ph_g, ev_g, r


@pytest.mark.parametrize('C,S,splits,seed,front', [
    (64, 2 ** 16, None, 1, 'auto'),                 # config 1 geometry (64 ch, 2^16 samples)
    (128, 2 ** 17, [0, 2 ** 15, 2 ** 17], 2, 'auto'),
    (256, 2 ** 18, [0, 2 ** 16 + 512, 2 ** 17, 2 ** 18], 3, 'auto'),   # config 2, streamed
    (256, 2 ** 18, [0, 2 ** 16 + 512, 2 ** 17, 2 ** 18], 3, 'split'),
    (512, 2 ** 18, None, 4, 'auto'),
    (512, 2 ** 19, [0, 2 ** 17 + 1024, 2 ** 19], 7, 'auto'),   # N = 1024 streamed (k_front3<1024>)
    (1024, 2 ** 20, [0, 2 ** 19, 2 ** 20], 5, 'auto'),    # config 3 geometry
    (1024, 2 ** 20, [0, 2 ** 19, 2 ** 20], 5, 'split'),
    (2048, 2 ** 20, [0, 3 * 2 ** 17 + 4096, 2 ** 20], 6, 'auto'),   # config 5 geometry (k_front5)
    (2048, 2 ** 20, None, 6, 'split'),
    (1024, 2 ** 20, [0, 2 ** 19, 2 ** 20], 5, 'auto-noacc'),   # the streaming variants bench times
    (2048, 2 ** 20, [0, 3 * 2 ** 17 + 4096, 2 ** 20], 6, 'auto-noacc'),
])
def test_chain_parity(gpu, C, S, splits, seed, front):
    """Full chain vs the oracle. 'auto' runs the fused front end (k_front3 for N = 512 / 1024 / 2048,
    k_front5 for N = 4096, k_front for N = 128); 'split' runs k_channelize + k_lpf_phase with z staged
    in HBM; 'auto-noacc' runs the fused front end with the avgIQ accumulator off (k_front5<false>,
    no y-sum stores), the variant every streaming call and bench.py run."""
    case, thr = cached_case(C, S, seed, max(1.0, S / (2 * C) / 400))
    acc = not front.endswith('-noacc')
    compare(case, thr, splits or [0, S], front=front.replace('-noacc', ''), acc=acc)


@pytest.mark.parametrize('acc', [True, False])
@pytest.mark.parametrize('C,S,seed', [
    # test_chain_parity's geometries, the ones its case cache still holds first
    (2048, 2 ** 20, 6), (1024, 2 ** 20, 5), (512, 2 ** 19, 7), (64, 2 ** 16, 1), (128, 2 ** 17, 2), (256, 2 ** 18, 3),
])
def test_fused_short_calls_and_run_tails(gpu, C, S, seed, acc):
    """The fused front ends' shared run geometry and hop loader at their smallest shapes: calls of
    2, 6 and 66 frames, then the rest. A 2-frame call is shorter than one iteration at N = 512 / 1024
    (4 frames per iteration) and reads everything but its own hops from the carried ADC history; a
    66-frame call is one full 64-frame run plus a 2-frame tail run at every geometry."""
    N = 2 * C
    case, thr = cached_case(C, S, seed, max(1.0, S / N / 400))
    compare(case, thr, [0, N, 4 * N, 37 * N, S], acc=acc)


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_baseline_modes(gpu, mode):
    C, S = 256, 2 ** 18
    case = signals.make_case(C, S, seed=11, pulses_per_ch=2.0)
    thr = quiet_thresholds(C, S, 11)
    if mode == 0:  # absolute threshold: below the tone's mean filtered phase
        o = signals.oracle_chain(case)
        raw = o.process(case.iq)['raw'].astype(np.int64)
        thr = (np.median(raw, axis=0) * 1.38 - 1500).astype(np.int64)
    compare(case, thr, [0, 2 ** 17, S], mode=mode)


def test_internal_subchunks_and_tiny_calls(gpu):
    """max_chunk < call size (internal sub-chunking) and calls of exactly N samples."""
    C, S = 64, 2 ** 15
    case = signals.make_case(C, S, seed=21, pulses_per_ch=2.0)
    thr = quiet_thresholds(C, S, 21)
    compare(case, thr, [0, S], max_chunk=8 * 2 * C)
    compare(case, thr, [0, S], max_chunk=8 * 2 * C, front='split')
    splits = list(range(0, 40 * 2 * C, 2 * C)) + [S]
    compare(case, thr, splits)
    compare(case, thr, splits, front='split')


def test_pipelined_subchunks(gpu):
    """max_chunk >= 512 N, the size from which the split front end once cut a call into four
    pipelined pieces (the test's name dates from then): a call is one piece on either front end,
    with z staged for the whole call on the split one. Ragged calls: one that ends five rows past
    an old piece boundary, a one-row call, one just short of a piece and one a row short of
    max_chunk; then the SVF baseline on two calls of max_chunk samples."""
    C = 64
    N = 2 * C
    S = 2 ** 19
    case = signals.make_case(C, S, seed=23, pulses_per_ch=6.0)
    thr = quiet_thresholds(C, 2 ** 18, 23)
    G = 2 ** 18 // 4
    splits = [0, 3 * G + 5 * N, 3 * G + 6 * N, 2 ** 18 + N, S]
    compare(case, thr, splits, max_chunk=2 ** 18, front='split')
    compare(case, thr, [0, S], mode=2, max_chunk=2 ** 18, front='split')
    compare(case, thr, splits, max_chunk=2 ** 18)  # fused


def test_deleted_channels_and_dead_time(gpu):
    C, S = 128, 2 ** 17
    case = signals.make_case(C, S, seed=31, pulses_per_ch=3.0)
    thr = quiet_thresholds(C, S, 31)
    case.fir12[::2] = 0  # zero taps delete a channel (ROACH_Pulses.py:64-67)
    _, ev, _ = compare(case, thr, [0, S], dead=0)
    chans = (np.asarray(ev, np.uint64) >> np.uint64(52)).astype(np.int64)
    assert np.all(chans % 2 == 1)
    compare(case, thr, [0, S], dead=200)


@pytest.mark.parametrize('noise,rate,seed,slots', [
    (30.0, 1 / 300.0, 51, None),   # noisy phase: speculation mostly right, pulses straddle segments
    (0.0, 1 / 200.0, 52, None),    # noiseless: EMA dead band -> speculation fails -> exact fix-up
    (30.0, 1 / 60.0, 53, None),    # pile-up: pulses every ~60 samples
    (30.0, 1 / 300.0, 54, 3),      # occupancy-sized segments: 3 of 5462 samples (ragged tails)
    (0.0, 1 / 200.0, 55, 3),
])
def test_speculative_trigger_exact(gpu, monkeypatch, noise, rate, seed, slots):
    """Calls long enough (J > 2048 phase samples) to take the parallel speculative-segment
    trigger; packets must equal the sequential oracle's bit for bit. `slots` pretends the GPU
    holds that many trigger waves, which stretches the segments beyond the 2048-sample minimum
    (the path a 2^30-sample call takes on the real chip)."""
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 64, 2 ** 21
    J = S // (2 * C)
    case = signals.make_case(C, S, seed=seed, noise=noise, pulses_per_ch=J * rate)
    thr = quiet_thresholds(C, 2 ** 18, seed) if noise > 0 else np.full(C, -1200)
    if slots is not None:
        monkeypatch.setenv('MKID_TRIG_WAVE_SLOTS', str(slots))
    ch = Channelizer(C, max_chunk=S)
    try:
        configure(ch, case, thr)
        ph, ev = ch.process(case.iq)
        reruns = ch.trigger_reruns()
    finally:
        ch.close()
    raw_g = np.clip(np.rint(ph * np.float32(8192)), -25736, 25736).astype(np.int16)
    ev_o, _, _ = otrig.Trigger(C, case.fir12, thr).run(raw_g)
    assert len(ev_o) > 100
    assert np.array_equal(sort_events(ev), sort_events(ev_o))
    if noise == 0.0:
        assert reruns > 0   # the fix-up path was exercised


def test_avg_iq_matches_oracle(gpu):
    C, S = 256, 2 ** 17
    case = signals.make_case(C, S, seed=41)
    thr = np.full(C, -(1 << 30))
    _, _, (mi, mq) = run_gpu(case, thr, [0, S])
    y = signals.oracle_chain(case).process(case.iq)['y']
    np.testing.assert_allclose(mi, y.real.mean(0), rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(mq, y.imag.mean(0), rtol=1e-4, atol=1e-2)


def test_errors_are_loud(gpu):
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(64)
    try:
        with pytest.raises(_lib.MkidError):
            ch.process(np.zeros((100, 2), np.int16))          # not a multiple of N
        with pytest.raises(_lib.MkidError):
            ch.set_fir(np.full((64, 26), 5000, np.int16))     # outside 12-bit
        with pytest.raises(_lib.MkidError):
            ch.set_bins(np.zeros(3, np.int32))                # wrong length
    finally:
        ch.close()
    with pytest.raises(_lib.MkidError):
        Channelizer(100)                                      # N = 200 unsupported


@pytest.mark.parametrize('front', ['auto', 'split'])
def test_iq_snapshot_tap_matches_oracle(gpu, front):
    """mkid_set_iq_tap: the tapped channel's low-pass output equals the oracle's y, rounded."""
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 256, 2 ** 17
    case = signals.make_case(C, S, seed=41, pulses_per_ch=1.0)
    y = signals.oracle_chain(case).process(case.iq)['y']
    ch = Channelizer(C, max_chunk=S, front=front)
    try:
        configure(ch, case, np.full(C, -(1 << 30), np.int64))
        tone = int(np.argmax(np.abs(y).mean(0)))
        ch.set_iq_tap(tone)
        ch.process(case.iq)
        iq = ch.iq_tap().astype(np.int64)
        exp = np.stack([np.rint(y[:, tone].real), np.rint(y[:, tone].imag)], 1)
        exp = np.clip(exp, -32768, 32767).astype(np.int64)
        assert iq.shape == exp.shape
        d = np.abs(iq - exp)
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
        assert np.abs(exp).max() > 100                      # a live tone, not zeros
        ch.set_iq_tap(-1)
        ch.process(case.iq[:2 * C * 8])
        assert ch.iq_tap().shape == (0, 2)
    finally:
        ch.close()


@pytest.mark.parametrize('C,S,splits,seed,mode,deleted', [
    (64, 2 ** 16, None, 31, 1, False),
    (256, 2 ** 18, [0, 2 ** 17 + 512, 2 ** 18], 32, 1, True),
    (256, 2 ** 18, None, 33, 0, False),
    (1024, 2 ** 20, [0, 2 ** 19, 2 ** 20], 34, 1, True),       # fused N = 2048, deleted channels
])
def test_fused_deleted_channels_and_modes(gpu, C, S, splits, seed, mode, deleted):
    """The fused front end + trigger against the oracle with uniform matched-filter taps whose
    zero rows are deleted channels (the reference zeroes a deleted channel's LUT,
    ROACH_Pulses.py:59-111), EMA and no-baseline modes, streamed calls. (Round 2 ran these cases
    through an opt-in two-stream pipeline with a register-lean trigger; both were removed in round
    3 as measured not to pay)"""
    case = signals.make_case(C, S, seed=seed, pulses_per_ch=max(2.0, S / (2 * C) / 400))
    if deleted:
        case.fir12[1::3] = 0
    thr = quiet_thresholds(C, min(S, 2 * C * 2048), seed)
    if mode == 0:
        o = signals.oracle_chain(case)
        raw = o.process(case.iq)['raw'].astype(np.int64)
        thr = (np.median(raw, axis=0) * 1.38 - 1500).astype(np.int64)
    compare(case, thr, splits or [0, S], mode=mode)
