"""mkid_phase_thresholds on the device against its CPU statement mkid_phase_thresholds_host and
against the host rule codecs.thresholds_from_phase_block on the same block, through the C ABI, the
Channelizer front end and the register shim. Everything is exact equality: thresholds, lo and hi as
integers, med and p05 bitwise (the rule has integer counts and a fixed sequence of IEEE float64
operations only)."""
import numpy as np
import pytest

import signals
import thr_cases
from mkids_sdr_amd import _lib, codecs

pytestmark = pytest.mark.gpu

STATS = np.dtype([('med', '<f8'), ('p05', '<f8'), ('lo', '<i4'), ('hi', '<i4')])
GUARD = 8   # output elements past nch that must stay as they were


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(64, max_chunk=1 << 16)
    yield ch
    ch.close()


def device_call(ch, raw, nch, nsigma=2.5, stats=True):
    """One device call on columns 0..nch-1 of the host block raw [rows][ld]. Returns (thr bytes,
    stats bytes or None) of channels 0..nch-1 after checking that the block and the output
    elements past nch are untouched."""
    import torch
    dev = ch.torch_device()
    rows, ld = raw.shape
    d_raw = torch.from_numpy(raw).to(dev)
    d_thr = torch.full((nch + GUARD,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    d_st = torch.full(((nch + GUARD) * STATS.itemsize,), 0xa5, dtype=torch.uint8, device=dev) if stats else None
    torch.cuda.synchronize(dev)
    ch.phase_thresholds_device(d_raw, rows, ld, nch, nsigma, d_thr, d_st)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_raw.cpu().numpy(), raw), 'the block was written'
    thr = d_thr.cpu().numpy()
    assert (thr[nch:] == 0x5a5a5a5a).all(), 'd_thr written past nch'
    st = None
    if stats:
        st = d_st.cpu().numpy()
        assert (st[nch * STATS.itemsize:] == 0xa5).all(), 'd_stats written past nch'
        st = st[:nch * STATS.itemsize].tobytes()
    return thr[:nch].tobytes(), st


def host_call(raw, nch, nsigma=2.5):
    thr, _, st = codecs.phase_thresholds_host(raw, nsigma, nch=nch, want_stats=True)
    assert st.dtype == STATS
    return thr.tobytes(), st.tobytes()


def mixed_block(seed, rows, nch, ld=None):
    """Every channel kind, cycling, so that neighbouring lanes hold a constant channel, a full-range
    one and a narrow one; wider blocks repeat a 192-column pattern."""
    rng = np.random.default_rng(seed)
    ld = nch if ld is None else ld
    base, _ = thr_cases.block(rng, rows, min(nch, 192))
    raw = np.empty((rows, ld), np.int16)
    raw[:, nch:] = rng.integers(-32768, 32768, (rows, ld - nch))   # junk beside the channels
    raw[:, :nch] = np.resize(base.T, (nch, rows)).T
    return raw


@pytest.mark.parametrize('rows,nch,ld', [(1, 1, 1), (7, 3, 3), (100, 65, 80), (1000, 64, 64), (10240, 256, 256)])
def test_device_equals_host_rule(ctx, rows, nch, ld):
    raw = mixed_block(rows + nch, rows, nch, ld)
    for nsigma in (2.5, 0.0, 6.0):
        thr, st = device_call(ctx, raw, nch, nsigma)
        assert (thr, st) == host_call(raw, nch, nsigma)
        ref = codecs.thresholds_from_phase_block(raw[:, :nch], nsigma)
        assert np.array_equal(np.frombuffer(thr, np.int32), ref)
    # two runs give identical bytes; without the stats the thresholds are the same
    assert device_call(ctx, raw, nch, 6.0) == (thr, st)
    assert device_call(ctx, raw, nch, 6.0, stats=False) == (thr, None)
    med = np.frombuffer(st, STATS)['med']
    for c in range(min(nch, 24)):
        assert med[c].tobytes() == np.float64(codecs.threshold_from_phase(raw[:, c], 6.0)[1]).tobytes()


def _row_block_lengths(ch):
    """Every row-block length the plan function returns, ascending: what it gives for a wide block
    (500 strips) of 1 .. longest + 1 rows, from the shortest (a block of one row) to the longest (the
    largest block the call accepts)."""
    b_min = ch.phase_thresholds_block_rows(1, 1, 1)
    b_max = ch.phase_thresholds_block_rows(2 ** 31 - 1, 1 << 20, 1 << 20)
    nch = 64 * 500
    got = {ch.phase_thresholds_block_rows(r, nch, nch) for r in range(1, b_max + 2)} | {b_min, b_max}
    assert min(got) == b_min and max(got) == b_max and len(got) > 2
    return sorted(got)


def _shape_for_block_rows(ch, B):
    """nch (= ld) at which blocks of B - 1, B and B + 1 rows are all worked on in row blocks of B rows,
    found with the plan function."""
    for strips in range(1, 4096):
        nch = 64 * strips
        if all(ch.phase_thresholds_block_rows(r, nch, nch) == B for r in (B - 1, B, B + 1)):
            return nch
    raise AssertionError('no shape gives row blocks of %d rows' % B)


def _spread(nch, n=48):
    """Channels of the first strip, the last strip and some between."""
    return sorted(set(range(min(n, nch))) | set(range(max(nch - n, 0), nch)) | set(range(0, nch, max(nch // n, 1))))


N_SHARES = 10


@pytest.mark.parametrize('share', range(N_SHARES))
def test_blocks_around_every_row_block_length(ctx, share):
    """Blocks of B - 1, B and B + 1 rows (one row block not full, one exactly full, a second of one
    row) for EVERY row-block length B the plan function returns, the lengths dealt out over the
    cases of this test (each case takes every N_SHARES-th length, whatever their number). The shapes
    are wide (the plan needs about two strips per compute unit to choose a B above the shortest), so
    every channel is checked against the CPU statement, and the independent numpy rule on channels of
    the first and the last strip and a spread between."""
    lengths = _row_block_lengths(ctx)
    assert len(lengths) >= N_SHARES
    for B in lengths[share::N_SHARES]:
        nch = _shape_for_block_rows(ctx, B)
        for rows in (B - 1, B, B + 1):
            assert ctx.phase_thresholds_block_rows(rows, nch, nch) == B
            raw = mixed_block(B + rows, rows, nch)
            thr, st = device_call(ctx, raw, nch)
            assert (thr, st) == host_call(raw, nch)
            cols = _spread(nch)
            ref = codecs.thresholds_from_phase_block(raw[:, cols])
            assert np.array_equal(np.frombuffer(thr, np.int32)[cols], ref)


@pytest.mark.parametrize('offset,ld', [(1, 80), (0, 79), (1, 79), (0, 80)])
def test_unaligned_blocks_and_odd_pitches(ctx, offset, ld):
    """A block that starts `offset` int16 past a 16-byte boundary and / or whose ld is no multiple
    of 8 runs one channel per thread; (0, 80) is the 16-byte path with a tail of 75 mod 8 channels.
    Rows around the row-block length of that very call (alignment included)."""
    import torch
    dev = ctx.torch_device()
    nch = 75
    B = ctx.phase_thresholds_block_rows(1, ld, nch, offset == 0)
    for rows in (B - 1, B, B + 1):
        assert ctx.phase_thresholds_block_rows(rows, ld, nch, offset == 0) == B
        wide = mixed_block(7 + rows, rows + 1, ld, ld).reshape(-1)      # a row of slack for the offset
        d_wide = torch.from_numpy(wide).to(dev)
        assert d_wide.data_ptr() % 16 == 0
        d_thr = torch.zeros(nch, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.phase_thresholds_device(d_wide.data_ptr() + 2 * offset, rows, ld, nch, 2.5, d_thr)
        torch.cuda.synchronize(dev)
        sub = np.ascontiguousarray(wide[offset:offset + rows * ld].reshape(rows, ld))
        got = d_thr.cpu().numpy()
        assert np.array_equal(got, codecs.phase_thresholds_host(sub, 2.5, nch=nch)[0])
        assert np.array_equal(got, codecs.thresholds_from_phase_block(sub[:, :nch]))
        assert np.array_equal(d_wide.cpu().numpy(), wide)


def test_shared_workspace_regrown_between_calls(ctx):
    """A call of another nch (a larger workspace, grown in between) does not change a call's bytes."""
    a = mixed_block(1, 300, 40, 48)
    b = mixed_block(2, 130, 1000)
    first = device_call(ctx, a, 40)
    other = device_call(ctx, b, 1000)
    assert device_call(ctx, a, 40) == first == host_call(a, 40)
    assert device_call(ctx, b, 1000) == other == host_call(b, 1000)


def test_argument_errors_leave_the_outputs(ctx):
    import torch
    dev = ctx.torch_device()
    raw = torch.zeros((4, 6), dtype=torch.int16, device=dev)
    thr = torch.full((6,), 77, dtype=torch.int32, device=dev)
    st = torch.zeros(6 * STATS.itemsize, dtype=torch.uint8, device=dev)
    ok = dict(d_raw=raw, rows=4, ld=6, nch=6, nsigma=2.5, d_thr=thr, d_stats=st)
    bad = [dict(d_raw=None), dict(d_thr=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(nch=0),
           dict(nch=-3), dict(nch=7), dict(nsigma=-0.5), dict(nsigma=float('inf')), dict(nsigma=float('nan'))]
    for kw in bad:
        with pytest.raises(_lib.MkidError) as e:
            ctx.phase_thresholds_device(**dict(ok, **kw))
        assert e.value.code == _lib.MKID_E_ARG, kw
        torch.cuda.synchronize(dev)
        assert (thr == 77).all() and not st.any(), kw
    ctx.phase_thresholds_device(**ok)
    torch.cuda.synchronize(dev)
    assert not thr.any()


def test_load_thresholds_end_to_end(gpu):
    """A 256-channel context on a quiet synthetic stream: load_thresholds() equals the host rule on
    the call's raw phase, and the trigger run with the thresholds it loaded gives the packets it
    gives with the host-computed ones."""
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 256, 1 << 19
    quiet = signals.make_case(C, S, seed=21, pulses_per_ch=0)
    case = signals.make_case(C, S, seed=21, pulses_per_ch=2.0)
    ch = Channelizer(C, max_chunk=S)
    try:
        ch.set_pfb(quiet.pfb)
        ch.set_bins(quiet.bins)
        ch.set_dds(quiet.lut_i, quiet.lut_q)
        ch.set_lpf(quiet.lpf12)
        ch.set_fir(quiet.fir12)
        ch.set_centers(quiet.ic, quiet.qc)
        ch.set_thresholds(np.full(C, -(1 << 30), np.int64))
        ch.set_baseline(1, 41, 82, 93623, 8192)
        ch.process(quiet.iq, want_phase=False)      # the start-up transient, which would set the range
        ch.process(quiet.iq, want_phase=False)      # a settled stretch (the source repeats every 2^16)
        raw = ch.raw_phase()
        thr, med = ch.load_thresholds()
        ref = codecs.thresholds_from_phase_block(raw)
        assert thr.dtype == np.int32 and np.array_equal(thr, ref)
        assert (ref <= 0).all() and (ref >= -25736).all() and (ref < 0).mean() > 0.5
        assert med.tobytes() == np.array([codecs.threshold_from_phase(raw[:, c])[1] for c in range(C)]).tobytes()
        thr6, _ = ch.phase_thresholds(raw, nsigma=6.0)      # the upload path
        assert np.array_equal(thr6, codecs.thresholds_from_phase_block(raw, 6.0))
        ch.reset()
        _, ev_dev = ch.process(case.iq, want_phase=False)   # with the thresholds load_thresholds set
        ch.reset()
        ch.set_thresholds(ref)
        _, ev_host = ch.process(case.iq, want_phase=False)
    finally:
        ch.close()
    assert len(ev_dev) > 0 and np.array_equal(ev_dev, ev_host)


def test_shim_load_thresholds_block(gpu):
    """RoachPulses.loadThresholdsBlock on a 256-channel FpgaClient: the thresholds of one block of
    the running stream equal the host rule on that call's raw rows, a customThresholds entry is
    honoured, and a following loadSingleThreshold changes only its channel."""
    from mkids_sdr_amd.roach import FpgaClient, RoachPulses, RoachSetup
    C, nf = 256, 16
    roach = FpgaClient(n_channels=C, noise_sigma=40.0, seed=3)
    roach.progdev('pulse_trigger_2022_Jan_24_1322.bof')
    rng = np.random.default_rng(9)
    freqs = list(4.0e9 + rng.choice(np.arange(-250, 250), nf, replace=False) * 1e6 + 15625.0)
    rs = RoachSetup(roach, freqs, 4.0e9, n_channels=C)
    rs.define_LUTs()
    rs.toggleDAC()
    rs.rotateLoopsReady()
    rp = RoachPulses(roach, nf, None, n_channels=C)
    rp.customThresholds[5] = -10.0
    custom = max(int(-10.0 / rp.scale_to_angle), -25736)
    seen = []
    run = roach.run
    roach.run = lambda n: seen.append(run(n)) or seen[-1]
    for steps, one_piece in ((2, True), (3, False)):     # 2048 rows: one device call; 3072: two pieces
        loaded = rp.loadThresholdsBlock(steps=steps, L=1024)
        phase = seen[-1][0]
        assert phase.shape == (steps * 1024, C)
        raw = np.clip(np.rint(phase * np.float32(8192)), -25736, 25736).astype(np.int16)
        if one_piece:
            assert np.array_equal(raw, roach.channelizer().raw_phase())
        ref = codecs.thresholds_from_phase_block(raw[:, :nf])
        want = [int(t) for t in ref]
        want[5] = custom
        assert loaded == want and all(-25736 <= t < 0 for t in want)
        assert np.array_equal(roach.cfg.thr[:nf], want) and 'thr' in roach.cfg.dirty
        assert (roach.cfg.thr[nf:] == -(1 << 30)).all()
        assert np.array_equal(rp.thresholds[:nf], rp.scale_to_angle * ref)
        meds = np.array([codecs.threshold_from_phase(raw[:, c])[1] for c in range(nf)])
        assert np.array_equal(rp.medians[:nf], rp.scale_to_angle * meds)
        assert not rp.thresholds[nf:].any() and not rp.medians[nf:].any()
    roach.run = run
    before = roach.cfg.thr.copy()
    t3 = rp.loadSingleThreshold(3)
    changed = np.flatnonzero(roach.cfg.thr != before)
    assert set(changed) <= {3} and roach.cfg.thr[3] == t3
    roach.run(64)                                         # the composed table reaches the device
    assert 'thr' not in roach.cfg.dirty
