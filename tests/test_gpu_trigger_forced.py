"""Fix-up re-runs forced at every segment boundary, in every baseline mode.

The other trigger tests meet fix-ups by chance (noiseless phase, a short warm-up). Here every
(channel, boundary b) gets one pulse `back` rows before b, with dead_time = 700: the oracle emits its
packet in [b - dead + 8, b - W - 8], so the true state at b is DEAD with a count the speculative walk
cannot have (it starts W rows before b in REARM, after the packet). That precondition is asserted
from the oracle's packets alone, on the CPU, for every pair; the device then has to re-run every
boundary of every channel, splice the lists and hand the right state to the next call."""
import functools
import os

import numpy as np
import pytest

from oracle import trigger as otrig
from mkids_sdr_amd import codecs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C, DEAD, NEXT = 64, 700, 500
L_EMA = 1040                                   # round26(kSegL) with MKID_TRIG_WAVE_SLOTS=64
# name: (mode, J, boundaries, W, back, environment, rearm_q8, seed)
CASES = {
    'none': (0, 4 * L_EMA + 17, [L_EMA * s for s in range(1, 5)], 260, 480, {}, 0, 7),
    'ema': (1, 4 * L_EMA + 17, [L_EMA * s for s in range(1, 5)], 260, 480, {}, 0, 8),
    # three segments of 4134 = 26 * 159 rows, the last one 4132: ragged 26-row and 64-row tails
    'svf': (2, 12400, [4134, 8268], 520, 620, {'MKID_SVF_WARMUP': 520}, 0, 9),
    'svf_rearm': (2, 12400, [4134, 8268], 520, 620, {'MKID_SVF_WARMUP': 520}, 192, 9),
}


def forced_rows(J, bounds, back, seed):
    """Fix16_13 rows [J + NEXT][C] as tests/test_gpu_svf.synth_raw makes them (offset U(-4000, 4000),
    noise sigma 300), with one pulse of 60-100 degrees per channel starting back +- 20 rows before
    each boundary. The NEXT rows of the following call carry one more pulse per channel, 60 +- 20
    rows in: whether and where it fires depends on the state the first call hands over (in modes 0
    and 1 the true state is still DEAD there, the speculative one is not)."""
    rng = np.random.default_rng(seed)
    ph = rng.normal(0.0, 300.0, (J + NEXT, C)) + rng.uniform(-4000, 4000, C)
    t = np.arange(400, dtype=np.float64)
    shape = (1 - np.exp(-t / 0.1)) * np.exp(-t / 65.0)
    starts = [[b - back + int(rng.integers(-20, 21)) for b in bounds] for _ in range(C)]
    for c in range(C):
        for s0 in starts[c] + [J + 60 + int(rng.integers(-20, 21))]:
            ph[s0:s0 + 400, c] -= np.deg2rad(rng.uniform(60, 100)) * 8192 * shape
    return np.clip(np.rint(ph), -25736, 25736).astype(np.int16)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's rows, taps, thresholds and the oracle's packets of both calls (computed once)."""
    from test_gpu_svf import synth_raw
    mode, J, bounds, W, back, env, rearm_q8, seed = CASES[name]
    raw = forced_rows(J, bounds, back, seed)
    mf = codecs.fir_quantise(np.loadtxt(os.path.join(GOLD, 'fir', 'matched_30us.txt')))
    taps = np.tile(mf, (C, 1))
    if mode == 0:   # no baseline: the level is absolute
        thr = (np.median(raw, axis=0) - 3000).astype(np.int32)
    else:
        quiet = synth_raw(C, 20000, 99, pulse_rate=0)
        thr = np.array([codecs.threshold_from_phase(quiet[:, c])[0] for c in range(C)], np.int32)
    tr = otrig.Trigger(C, taps, thr, mode=mode, dead=DEAD, rearm_q8=rearm_q8)
    exp = [tr.run(raw[:J])[0], tr.run(raw[J:])[0]]
    for a in (raw, taps, thr, *exp):
        a.setflags(write=False)
    return raw, taps, thr, exp


def pairs_left_out(name):
    """(channel, boundary) pairs without an oracle packet stamped in [b - dead + 8, b - W - 8]."""
    _, J, bounds, W, _, _, _, _ = CASES[name]
    ev = codecs.unpack_wide(case(name)[3][0])
    out = []
    for c in range(C):
        ts = ev['ts'][ev['ch'] == c]
        out += [(c, b) for b in bounds if not np.any((ts >= b - DEAD + 8) & (ts <= b - W - 8))]
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_forced_precondition(name):
    """A condition, not a tolerance: no pair may be left out."""
    assert pairs_left_out(name) == []


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_forced_boundary_mismatch(gpu, monkeypatch, name):
    from mkids_sdr_amd.channelizer import Channelizer
    mode, J, bounds, W, back, env, rearm_q8, seed = CASES[name]
    raw, taps, thr, exp = case(name)
    assert pairs_left_out(name) == []
    monkeypatch.setenv('MKID_TRIG_WAVE_SLOTS', '64')   # L = 1040 on any device
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ch = Channelizer(C, max_chunk=J * 2 * C, dead_time=DEAD)
    try:
        ch.set_fir(taps)
        ch.set_thresholds(thr)
        ch.set_baseline(mode, 41, 82, 93623, 8192)
        if rearm_q8:
            ch.set_rearm(rearm_q8)
        got = ch.trigger_phase(raw[:J].copy())   # the shared rows stay read-only
        reruns = ch.trigger_reruns()
        nxt = ch.trigger_phase(raw[J:].copy())   # one segment: pins st_out of the override / not-truth exits
    finally:
        ch.close()
    print('%s: %d packets, %d reruns (%d boundaries x %d channels), next call %d packets'
          % (name, len(got), reruns, len(bounds), C, len(nxt)))
    assert np.array_equal(got, exp[0])   # unsorted, as produced
    assert reruns >= C * len(bounds)
    assert np.array_equal(nxt, exp[1])
