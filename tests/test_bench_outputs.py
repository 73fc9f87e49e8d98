"""bench.py's plain run and `--dump-outputs DIR`: the last timed step's outputs as float32 / float64
.npy files (`dump_outputs`: counts, packets by field in word order, config-5 heights in the same
order, the phase stream or its fixed seeded positions), and the result line of a plain run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _words(rng, n):
    ch = rng.integers(0, 1 << 12, n).astype(np.uint64)
    peak = rng.integers(0, 1 << 12, n).astype(np.uint64)
    base = rng.integers(0, 1 << 12, n).astype(np.uint64)
    us = rng.integers(0, 1 << 28, n).astype(np.uint64)
    w = (ch << np.uint64(52)) | (peak << np.uint64(40)) | (base << np.uint64(28)) | us
    return w, np.stack([ch, peak, base, us], axis=1)


def test_dump_outputs_small_stream(tmp_path):
    """Packets come out by field, sorted by word, heights follow them (NaN kept), entries past the
    written count are left out, and a short phase stream is written whole."""
    import torch
    rng = np.random.default_rng(3)
    n, cap = 1000, 1500
    w, fields = _words(rng, n)
    ev = np.zeros(cap, np.uint64)
    ev[:n] = w
    ev[n:] = np.uint64((1 << 64) - 1)
    h = rng.standard_normal(cap).astype(np.float32)
    h[7] = np.nan
    phase = torch.from_numpy(rng.standard_normal(4096).astype(np.float32))
    d = str(tmp_path / 'out')
    bench.dump_outputs(d, phase, torch.from_numpy(ev.view(np.int64)), np.array([n + 5, n]), torch.from_numpy(h))
    assert sorted(os.listdir(d)) == ['counts.npy', 'heights.npy', 'packets.npy', 'phase.npy', 'phase_index.npy']
    o = np.argsort(w, kind='stable')
    got = np.load(os.path.join(d, 'packets.npy'))
    assert got.dtype == np.float64 and got.shape == (n, 4)
    assert np.array_equal(got, fields[o].astype(np.float64))
    gh = np.load(os.path.join(d, 'heights.npy'))
    assert gh.dtype == np.float32 and np.array_equal(gh, h[:n][o], equal_nan=True)
    assert np.array_equal(np.load(os.path.join(d, 'counts.npy')), np.array([n + 5.0, n]))
    gp = np.load(os.path.join(d, 'phase.npy'))
    assert gp.dtype == np.float32 and np.array_equal(gp, phase.numpy())
    assert np.array_equal(np.load(os.path.join(d, 'phase_index.npy')), np.arange(4096.0))


def test_dump_outputs_samples_a_long_stream(tmp_path):
    """Past 2^22 values the phase stream is sampled at fixed positions: both ends and seeded ones
    in between, the same from call to call; no heights file without heights."""
    import torch
    total = (1 << 22) + 12345
    phase = torch.arange(total, dtype=torch.float32)         # exact below 2^24: value == position
    ev = torch.zeros(8, dtype=torch.int64)
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    bench.dump_outputs(a, phase, ev, np.array([0, 0]), None)
    bench.dump_outputs(b, phase, ev, np.array([0, 0]), None)
    assert 'heights.npy' not in os.listdir(a)
    idx = np.load(os.path.join(a, 'phase_index.npy'))
    val = np.load(os.path.join(a, 'phase.npy'))
    assert idx.dtype == np.float64 and val.dtype == np.float32
    assert np.array_equal(idx, np.load(os.path.join(b, 'phase_index.npy')))
    assert np.array_equal(val.astype(np.float64), idx)
    assert np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == total - 1
    edge = bench.DUMP_PHASE_EDGE
    assert np.array_equal(idx[:edge], np.arange(edge)) and np.array_equal(idx[-edge:], total - edge + np.arange(edge))
    assert 2 * edge + bench.DUMP_PHASE_RANDOM // 2 < len(idx) <= 2 * edge + bench.DUMP_PHASE_RANDOM
    assert np.load(os.path.join(a, 'packets.npy')).shape == (0, 4)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) < 64e6


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], cwd=ROOT,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeat(gpu, tmp_path):
    """A plain run (config 3 at 2^24 samples, 3 timed steps) carries the headline keys and none of
    the `--full` legs (those run in test_gpu_bench_multi.py), and two runs with the same arguments
    dump identical arrays."""
    common = ['--gpus', '1', '--config', '3', '--log2-samples', '24', '--steps', '3', '--warmup', '2']
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    out = _bench(common + ['--dump-outputs', a])
    _bench(common + ['--dump-outputs', b])
    assert all(k in out for k in HEADLINE)
    assert out['steps'] == 3 and out['warmup'] == 2 and out['ms_per_step'] > 0
    # both figures come from the same interval; ms_per_step is rounded to 1 us, value to 0.1 MS/s
    ms = out['ms_per_step']
    assert abs(out['value'] - (1 << 24) / ms / 1e3) <= out['value'] * 0.0006 / ms + 0.1
    assert out['detector'] is None and 'cpu_baseline' not in out and 'parity' not in out
    assert out['roofline']['stream_copy_GBps'] is None and out['roofline']['achieved'] > 0
    names = sorted(os.listdir(a))
    assert names == ['counts.npy', 'packets.npy', 'phase.npy', 'phase_index.npy'] == sorted(os.listdir(b))
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y, equal_nan=True), f
    counts = np.load(os.path.join(a, 'counts.npy'))
    assert counts[0] == counts[1] == out['packets_per_step_rank0'] > 100
    assert len(np.load(os.path.join(a, 'packets.npy'))) == counts[1]
    phase = np.load(os.path.join(a, 'phase.npy'))
    index = np.load(os.path.join(a, 'phase_index.npy'))
    assert len(phase) == len(index) > (1 << 21) and index[-1] == (1 << 23) - 1
    assert np.all(np.abs(phase) <= np.pi + 1e-6) and phase.std() > 0
