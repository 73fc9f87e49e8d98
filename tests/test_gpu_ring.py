"""The ring forms of the photon list and fill, mkid_pack_second and mkid_clear_second on the device
(k_photons.hip, k_pack.hip) against the host twins, which tests/test_ring_host.py holds against the
unbounded tables, PacketMaster and the numpy restatement. Everything is an integer or a float copied
bit for bit, and every comparison is exact, the poison of every slot and entry that must not be
written included. Then a streamed run through observe.Observation(photon_rows=..., ring=R) with a
drain after every step against the same run without a ring.
"""
import numpy as np
import pytest

import observe_cases as oc
import photon_cases as pc
import ring_cases as rc_
from mkids_sdr_amd import _lib, observe, packets

pytestmark = pytest.mark.gpu
C = 64
N = 2 * C
SLICE = 2048                        # csrc/pkt_common.h kObsSlice
FIELDS = ('image', 'outside', 'words', 'stamps', 'dropped', 'height', 'dt', 'fill')


@pytest.fixture(scope='module')
def ctxs(gpu):
    """Contexts by sample clock: it is part of a context's configuration."""
    from mkids_sdr_amd.channelizer import Channelizer
    made = {}

    def get(fs=oc.FS):
        if fs not in made:
            made[fs] = Channelizer(C, max_chunk=2 ** 14, sample_rate=fs)
        return made[fs]

    yield get
    for ch in made.values():
        ch.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    torch.cuda.synchronize()        # torch's stream made it, the context's stream reads it
    return t


def _host(t, like):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint64) if like.dtype == np.uint64 else a


class DevTables:
    """A ring_cases.RingTables on the device."""

    def __init__(self, t):
        self.like = t
        for k in FIELDS:
            setattr(self, k, _dev(getattr(t, k)))

    def host(self):
        t = rc_.RingTables(self.like.n_seconds, self.like.C, self.like.K)
        for k in FIELDS:
            setattr(t, k, _host(getattr(self, k), getattr(self.like, k)))
        return t


def _copy(t):
    c = rc_.RingTables(t.n_seconds, t.C, t.K)
    for k in FIELDS:
        setattr(c, k, getattr(t, k).copy())
    return c


def _equal(a, b):
    """Every table of a and b bit for bit (the heights as 32-bit patterns) -> names that differ."""
    bits = lambda t, k: getattr(t, k).view(np.uint32) if k in ('height', 'dt') else getattr(t, k)
    return [k for k in FIELDS if not np.array_equal(bits(a, k), bits(b, k))]


def dev_list(ctx, ev, j0, win, K, layout, d, count=None, cap=None):
    sec0, R, sec_end = win
    d_ev = _dev(ev) if len(ev) else None
    rest = (j0, sec0, R, sec_end, K, layout, d.image, d.outside, d.words, d.stamps, d.dropped)
    if count is None:
        ctx.list_photons_ring_device(d_ev, len(ev), *rest)
    else:
        ctx.list_photons_ring_counted(d_ev, _dev(np.array([count], np.int64)), cap, *rest)


def dev_fill(ctx, ev, h, dt, j0, jd, win, K, d, row_dt=True, count=None, cap=None):
    sec0, R, sec_end = win
    d_ev, d_h = (_dev(ev), _dev(np.asarray(h, np.float32))) if len(ev) else (None, None)
    d_dt = None if dt is None or not len(ev) else _dev(np.asarray(dt, np.float32))
    rest = (j0, jd, sec0, R, sec_end, K, d.image, d.stamps, d.height, d.dt if row_dt else None, d.fill)
    if count is None:
        ctx.fill_photon_heights_ring_device(d_ev, d_h, d_dt, len(ev), *rest)
    else:
        ctx.fill_photon_heights_ring_counted(d_ev, d_h, d_dt, _dev(np.array([count], np.int64)), cap, *rest)


def dev_pack(ctx, d, sec, cap_out=None, size=None, stamps=True, dt=True):
    """mkid_pack_second of DevTables d into poisoned buffers -> ring_cases.Packed on the host."""
    t = d.like
    cap_out = t.C * t.K if cap_out is None else cap_out
    p = rc_.Packed(t.C, cap_out if size is None else size)
    dp = {k: _dev(getattr(p, k)) for k in rc_.Packed.NAMES}
    ctx.pack_second(sec, t.n_seconds, t.K, d.image, d.words, d.stamps if stamps else None, d.height,
                    d.dt if dt else None, cap_out, dp['counts'], dp['offsets'], dp['words'],
                    dp['stamps'] if stamps else None, dp['height'], dp['dt'] if dt else None, dp['total'])
    for k in rc_.Packed.NAMES:
        setattr(p, k, _host(dp[k], getattr(p, k)))
    return p


def dev_clear(ctx, d, sec, dt=True):
    ctx.clear_second(sec, d.like.n_seconds, d.like.K, d.image, d.height, d.dt if dt else None)


def _parity(ctx, ev, h, j0, jd, fs, win, K, layout, t=None, count=None, cap=None, distinct=False):
    """Device list and fill against the twins, both continuing RingTables t -> the tables. With
    `distinct` the fill gets the first packet of every (channel, stamp) only: two packets of one
    stamp would write the same slot, in no order on the device."""
    t = rc_.RingTables(win[1], C, K) if t is None else t
    m = len(ev) if count is None else max(min(count, cap), 0)
    d = DevTables(t)
    dev_list(ctx, ev, j0, win, K, layout, d, count, cap)
    want = _copy(t)
    assert rc_.list_ring_host(ev[:m], j0, N, fs, C, win, K, layout, want)[0] == 0
    if distinct:
        first = np.sort(np.unique(ev & ~np.uint64(0xFFFFFF << 28), return_index=True)[1])
        ev, h, m = ev[first], h[first], len(first)
    dev_fill(ctx, ev, h, h, j0, jd, win, K, d, count=count, cap=cap)
    assert rc_.fill_ring_host(ev[:m], h[:m], h[:m], j0, jd, N, fs, C, win, want) == 0
    got = d.host()
    assert _equal(got, want) == [], (_equal(got, want), len(ev), K, layout, win, count, cap)
    return got, d


CASES = pc.cases(C, N)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_parity_case_table(ctxs, c):
    """photon_cases' table through the ring forms with sec0 > 0 where the case has a second to leave
    out, R = 2, then every slot packed. The shuffled list is not in the device's order: its counters."""
    ctx = ctxs(c['fs'])
    sec0 = min(1, c['n_seconds'] - 1)
    win = (sec0, 2, c['n_seconds'])
    jd = c['j0'] + 200
    for K in c['Ks']:
        for layout in pc.LAYOUTS:
            if c['name'] == 'shuffled':
                d = DevTables(rc_.RingTables(2, C, K))
                dev_list(ctx, c['ev'], c['j0'], win, K, layout, d)
                _, want = rc_.list_ring_host(c['ev'], c['j0'], N, c['fs'], C, win, K, layout)
                assert d.host().same(want, ('image', 'outside', 'dropped')) == [] and want.outside[2:].min() > 0
                continue
            got, d = _parity(ctx, c['ev'], c['h'], c['j0'], jd, c['fs'], win, K, layout, distinct=True)
            assert got.image.sum() + got.outside.sum() == len(c['ev'])
            for s in range(sec0, min(sec0 + 2, c['n_seconds'])):
                assert dev_pack(ctx, d, s).differs(rc_.pack_host(got, s)[1]) == [], (K, layout, s)


class DevRing(rc_.HostRing):
    """ring_cases.HostRing's four calls on the device, the tables kept there between the calls."""

    def __init__(self, ctx, st, K, layout):
        super().__init__(st, K, layout)
        self.ctx = ctx

    def tables(self, R):
        return DevTables(rc_.RingTables(R, self.st['C'], self.K))

    def list(self, ev, j0, win, d):
        dev_list(self.ctx, ev, j0, win, self.K, self.layout, d)

    def fill(self, ev, h, dt, j0, jd, win, d):
        dev_fill(self.ctx, ev, h, dt, j0, jd, win, self.K, d)

    def pack(self, d, sec):
        return dev_pack(self.ctx, d, sec)

    def clear(self, d, sec):
        dev_clear(self.ctx, d, sec)

    def host(self, d):
        return d.host()


@pytest.mark.parametrize('K,R', [(1, 1), (3, 2), (3, 3), (2000, 4)])
def test_stream_with_drains(ctxs, K, R):
    """The multi-second stream in random calls, a drain at every legal moment and at random ones:
    every drained second and the tables left behind equal the twins' run, bit for bit."""
    st = rc_.stream(C=C, N=N, n=3000)
    ctx = ctxs(st['fs'])
    for mode in ('always', 'random'):
        rng = np.random.default_rng(10 * R + K)
        calls = rc_.cut_calls(st['rows'], rng)
        picks = rng.random(len(calls)) < 0.5
        drain = (lambda k: True) if mode == 'always' else (lambda k: bool(picks[k]))
        want = rc_.run_stream(st, calls, K, pc.WIDE, R=R, drain=drain)
        got = rc_.run_stream(st, calls, K, pc.WIDE, R=R, drain=drain, ops=DevRing(ctx, st, K, pc.WIDE))
        assert sorted(got['seconds']) == list(range(rc_.SECONDS))
        for s in got['seconds']:
            assert got['seconds'][s].differs(want['seconds'][s]) == [], (mode, s)
        assert _equal(got['t'], want['t']) == [] and want['kinds'][rc_.EARLY] == 0
        assert want['kinds'][rc_.OVERRUN] > 0 if R == 1 else (want['kinds'][rc_.OVERRUN] == 0 or R < 3 or mode == 'random')
        assert want['t'].dropped[0] > 0 or K == 2000


def _long_list(n, seed):
    """n packets in the device's order over seconds 0 .. 2 and a little of the third, channels >= C
    among them, and their heights."""
    rng = np.random.default_rng(seed)
    tb = packets.Timebase(oc.FS, N)
    ch = np.where(rng.random(n) < 0.02, rng.integers(C, 4096, n), rng.integers(0, C, n))
    ev = oc.device_order(pc.unique_packets(ch, rng.integers(0, tb.first_row(3) + 50, n), rng), 0)
    return ev, oc.heights_for(len(ev), rng), tb.first_row(2) + 300


@pytest.mark.parametrize('n', [0, 1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 300])
def test_list_lengths(ctxs, n):
    """Seconds 1 and 2 of an exposure of 3 in a ring of 2 (second 0 is early, second 3 late)."""
    ev, h, jd = _long_list(n, 160 + n)
    for K, layout in ((3, pc.WIDE), (100, pc.REFERENCE)):
        got, _ = _parity(ctxs(), ev, h, 0, jd, oc.FS, (1, 2, 3), K, layout)
        assert n < SLICE or (got.outside[:3].min() > 0 and got.fill.min() > 0 and (K == 3) == (got.dropped[0] > 0))
    if n >= SLICE:                                        # and the overrun kind: a ring of 1
        got, _ = _parity(ctxs(), ev, h, 0, jd, oc.FS, (1, 1, 3), 3, pc.WIDE)
        assert got.outside.min() > 0


def test_counted_forms(ctxs):
    """*d_count below, at and above cap, negative and 0, for the list and the fill."""
    ev, h, jd = _long_list(3000, 164)
    n = len(ev)
    for count, cap in ((n // 2, n), (n + 50, n - 7), (0, n), (1, n), (n, n), (-4, n), (2100, 2100)):
        for K in (2, 30):
            got, _ = _parity(ctxs(), ev, h, 0, jd, oc.FS, (1, 2, 3), K, pc.REFERENCE, count=count, cap=cap)
            assert got.image.sum() + got.outside.sum() == max(min(count, cap), 0)


def _random_tables(R, K, fill, seed):
    """Tables with random words, stamps, heights and dt in every slot (so that a wrong source index
    shows) and the row counts fill(rng) -> int32 [R][C]."""
    rng = np.random.default_rng(seed)
    t = rc_.RingTables(R, C, K)
    t.image[:] = fill(rng)
    shape = (R, C, K)
    t.words[:] = rng.integers(0, 1 << 63, shape, dtype=np.int64).view(np.uint64)
    t.stamps[:] = rng.integers(0, 1 << 40, shape)
    t.height.view(np.uint32)[:] = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)   # NaN payloads among them
    t.dt.view(np.uint32)[:] = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    return t


def _pack_parity(ctx, t, sec, **kw):
    d = DevTables(t)
    got = dev_pack(ctx, d, sec, **kw)
    want = rc_.pack_host(t, sec, **kw)[1]
    assert got.differs(want) == [], (got.differs(want), sec, kw)
    assert _equal(d.host(), t) == []                      # pack writes none of the tables
    return got, d


@pytest.mark.parametrize('K', [1, 7, 300])
def test_pack_and_clear(ctxs, K):
    """Rows from empty to overflowing (K = 300: more than one tile of 256 slots) in a ring of 3; cap_out
    at the edges and inside a row; no stamps, no dt; twice the same bits; clear, then the slot
    refilled by the list."""
    ctx = ctxs()
    t = _random_tables(3, K, lambda r: r.integers(0, 2 * K + 2, (3, C)).astype(np.int32), 170 + K)
    t.image[1, 5], t.image[1, 9] = -3, 0                  # a count that wrapped past 2^31: a full row
    got, d = _pack_parity(ctx, t, 1 + 3 * 11)
    total = int(got.total[0])
    assert total > C * K // 3 and got.counts[5] == -3
    inside = int(got.offsets[7]) + max(K // 2, 0)         # cuts row 7 (or ends at its start for K = 1)
    for cap in (0, 1, total - 1, total, total + 1, inside):
        p, _ = _pack_parity(ctx, t, 1, cap_out=cap, size=total + 4)
        assert list(p.total) == [total, min(total, cap)] and np.all(p.words[min(total, cap):] == pc.POISON_W)
    bare, _ = _pack_parity(ctx, t, 1, stamps=False, dt=False)
    assert np.all(bare.stamps == pc.POISON_S) and np.all(bare.dt.view(np.uint32) == rc_.POISON_F)
    assert dev_pack(ctx, d, 1).differs(got) == []         # run twice: the same bits
    for dt in (True, False):                              # clear: the device against the twin, whole tables
        d2, want = DevTables(t), _copy(t)
        dev_clear(ctx, d2, 4, dt)
        assert rc_.clear_host(want, 4, dt) == 0 and _equal(d2.host(), want) == []
        assert not want.image[1].any() and want.image[0].any()
    # refill: slot 1, cleared, takes second 4 from the list (seconds 5 and 6 join what slots 2 and 0
    # hold, second 7 finds no slot); its packed rows equal the twin's
    dev_clear(ctx, d, 1)
    cleared = d.host()
    assert not cleared.image[1].any() and cleared.image[0].any()
    ev, _, _ = _long_list(3000, 171)
    j0 = packets.Timebase(oc.FS, N).first_row(4)          # the same stamps from second 4 on
    ch, jg = oc.decode(ev, 0)
    rng = np.random.default_rng(172)
    ev = oc.device_order(oc.pack(ch, jg + j0, rng), j0)
    refilled, d3 = _parity(ctx, ev, oc.heights_for(len(ev), rng), j0, j0 + 20000, oc.FS, (4, 3, 9), K, pc.WIDE, cleared)
    assert dev_pack(ctx, d3, 4).differs(rc_.pack_host(refilled, 4)[1]) == []
    assert refilled.image[1].sum() > 100 and refilled.outside[3] > 0


def test_pack_extremes(ctxs):
    """K = 65536 with two long rows only (one full, one ending inside a tile), every row empty, and one
    row holding everything."""
    ctx = ctxs()
    K = 65536

    def two_long(r):
        image = np.zeros((1, C), np.int32)
        image[0, 3], image[0, 40] = K + 5, 40000 + 77
        return image

    t = _random_tables(1, K, two_long, 180)
    total = K + 40077
    got, _ = _pack_parity(ctx, t, 0, cap_out=total + 3)
    assert list(got.total) == [total, total] and got.offsets[4] == K and got.offsets[41] == total
    _pack_parity(ctx, t, 0, cap_out=K + 1000)             # the cut inside the second long row
    d, want = DevTables(t), _copy(t)
    dev_clear(ctx, d, 0)
    assert rc_.clear_host(want, 0) == 0 and _equal(d.host(), want) == []
    for K2 in (1, 7):
        empty = _random_tables(2, K2, lambda r: np.zeros((2, C), np.int32), 181)
        got, _ = _pack_parity(ctx, empty, 1)
        assert not got.total.any() and not got.offsets.any() and np.all(got.words == pc.POISON_W)
        one = _random_tables(2, K2, lambda r: np.zeros((2, C), np.int32), 182)
        one.image[1, C - 1] = K2
        got, _ = _pack_parity(ctx, one, 1)
        assert list(got.total) == [K2, K2] and np.array_equal(got.words[:K2], one.words[1, C - 1])


def _code(fn):
    with pytest.raises(_lib.MkidError) as e:
        fn()
    return e.value.code


def test_argument_errors(ctxs):
    """Every MKID_E_ARG case of the six device calls fails before any launch."""
    ctx = ctxs()
    ev, h, jd = _long_list(300, 190)
    t = _random_tables(2, 4, lambda r: r.integers(0, 6, (2, C)).astype(np.int32), 191)
    d = DevTables(t)
    d_ev, d_h, d_cnt = _dev(ev), _dev(h), _dev(np.array([len(ev)], np.int64))
    p = rc_.Packed(C, 8)
    dp = {k: _dev(getattr(p, k)) for k in rc_.Packed.NAMES}

    def lst(**kw):
        a = dict(ev=d_ev, n=len(ev), j0=0, sec0=0, R=2, end=5, K=4, layout=pc.WIDE, image=d.image, out=d.outside,
                 words=d.words, stamps=d.stamps, dropped=d.dropped)
        a.update(kw)
        rest = (a['j0'], a['sec0'], a['R'], a['end'], a['K'], a['layout'], a['image'], a['out'], a['words'], a['stamps'],
                a['dropped'])
        if 'cnt' in a:
            return ctx.list_photons_ring_counted(a['ev'], a['cnt'], a['n'], *rest)
        return ctx.list_photons_ring_device(a['ev'], a['n'], *rest)

    def fill(**kw):
        a = dict(ev=d_ev, h=d_h, dt=d_h, n=len(ev), j0=0, jd=jd, sec0=0, R=2, end=5, K=4, image=d.image, stamps=d.stamps,
                 height=d.height, rdt=d.dt, fill=d.fill)
        a.update(kw)
        rest = (a['j0'], a['jd'], a['sec0'], a['R'], a['end'], a['K'], a['image'], a['stamps'], a['height'], a['rdt'],
                a['fill'])
        if 'cnt' in a:
            return ctx.fill_photon_heights_ring_counted(a['ev'], a['h'], a['dt'], a['cnt'], a['n'], *rest)
        return ctx.fill_photon_heights_ring_device(a['ev'], a['h'], a['dt'], a['n'], *rest)

    def pack(**kw):
        a = dict(sec=0, R=2, K=4, image=d.image, words=d.words, stamps=d.stamps, height=d.height, rdt=d.dt, cap=8,
                 counts=dp['counts'], offsets=dp['offsets'], ow=dp['words'], os=dp['stamps'], oh=dp['height'], odt=dp['dt'],
                 total=dp['total'])
        a.update(kw)
        return ctx.pack_second(a['sec'], a['R'], a['K'], a['image'], a['words'], a['stamps'], a['height'], a['rdt'], a['cap'],
                               a['counts'], a['offsets'], a['ow'], a['os'], a['oh'], a['odt'], a['total'])

    def clear(**kw):
        a = dict(sec=0, R=2, K=4, image=d.image, height=d.height, rdt=d.dt)
        a.update(kw)
        return ctx.clear_second(a['sec'], a['R'], a['K'], a['image'], a['height'], a['rdt'])

    common = (dict(R=0), dict(R=(1 << 20) + 1), dict(sec0=-1), dict(sec0=6), dict(end=(1 << 63) // oc.FS), dict(ev=None),
              dict(image=None), dict(stamps=None), dict(n=-1), dict(j0=-1), dict(j0=1 << 62), dict(K=0), dict(K=65537),
              dict(cnt=None), dict(cnt=d_cnt, n=-1))
    for kw in common + (dict(out=None), dict(words=None), dict(dropped=None), dict(layout=2), dict(layout=-1)):
        assert _code(lambda: lst(**kw)) == _lib.MKID_E_ARG, kw
    for kw in common + (dict(h=None), dict(height=None), dict(fill=None)):
        assert _code(lambda: fill(**kw)) == _lib.MKID_E_ARG, kw
    slot = (dict(sec=-1), dict(R=0), dict(R=(1 << 20) + 1), dict(K=0), dict(K=65537), dict(image=None), dict(height=None))
    for kw in slot + (dict(words=None), dict(counts=None), dict(offsets=None), dict(total=None), dict(cap=-1), dict(ow=None),
                      dict(oh=None), dict(stamps=None), dict(rdt=None)):
        assert _code(lambda: pack(**kw)) == _lib.MKID_E_ARG, kw
    for kw in slot:
        assert _code(lambda: clear(**kw)) == _lib.MKID_E_ARG, kw
    L = ctx._L
    assert L.mkid_pack_second(None, 0, 1, 1, *([None] * 5), 0, *([None] * 7)) == _lib.MKID_E_ARG
    assert L.mkid_clear_second(None, 0, 1, 1, None, None, None) == _lib.MKID_E_ARG
    assert _equal(d.host(), t) == [] and all(np.array_equal(_host(dp[k], getattr(p, k)), getattr(p, k)) for k in ('words', 'total'))
    lst(n=0, ev=None)                                     # the valid edges
    fill(n=0, ev=None, h=None, dt=None)
    pack(cap=0, ow=None, os=None, oh=None, odt=None)
    assert _equal(d.host(), t) == []


_SIGNAL = []


def _signal(S, K):
    """The input of test_gpu_photon_rows.test_observation_end_to_end, made once."""
    import signals
    if not _SIGNAL:
        case = signals.make_case(C, K * S, seed=7, pulses_per_ch=24.0)
        quiet = signals.make_case(C, S, seed=7, pulses_per_ch=0)
        _SIGNAL.append((case, signals.thresholds_from_quiet(quiet, signals.oracle_chain(quiet).process(quiet.iq)['raw'])))
    return _SIGNAL[0]


def _run_observation(ring, n_seconds, R):
    """The four-call run of test_gpu_photon_rows.test_observation_end_to_end at 200 rows per second
    (six seconds in 1024 rows) with the fit and photon_rows = R."""
    import torch
    from mkids_sdr_amd.channelizer import Channelizer
    S, K, ncoeff, pre, nbins, L = 2 ** 15, 4, 40, 10, 32, 3
    J = S // (2 * C)
    fs = 2 * C * 200
    case, thr = _signal(S, K)
    coeff = np.random.default_rng(41).normal(size=(C, ncoeff)).astype(np.float32)
    x = torch.from_numpy(case.iq.reshape(-1)).to('cuda')
    cap = J * C
    ch = Channelizer(C, max_chunk=S, sample_rate=fs)
    try:
        ch.set_pfb(case.pfb)
        ch.set_bins(case.bins)
        ch.set_dds(case.lut_i, case.lut_q)
        ch.set_lpf(case.lpf12)
        ch.set_fir(case.fir12)
        ch.set_centers(case.ic, case.qc)
        ch.set_thresholds(thr)
        ch.set_pulse_filter(coeff, pre)
        ch.set_pulse_fit(L, -1)
        obs = observe.Observation(ch, n_seconds, nbins, -20.0, 40.0 / nbins, cap, cap, fit=True, photon_rows=R,
                                  row_layout=pc.REFERENCE, ring=ring)
        syncs = []
        sync0 = obs._sync
        obs._sync = lambda: (syncs.append(1), sync0())[1]
        bufs = [(torch.empty((J, C), dtype=torch.float32, device='cuda'), torch.empty(cap, dtype=torch.int64, device='cuda'),
                 torch.zeros(2, dtype=torch.int64, device='cuda')) for _ in range(K)]
        torch.cuda.synchronize()
        seconds, plan = [], []
        for k, (d_ph, d_ev, d_cnt) in enumerate(bufs):
            ch.process_device(x[2 * k * S:2 * (k + 1) * S], S, d_ph, d_ev, cap, d_cnt)
            before = len(syncs)
            obs.step(d_ph, J, k * J, d_ev, d_cnt)
            assert len(syncs) == before                  # a step makes no synchronisation
            if ring:
                plan.append((obs.sec0, obs.ready()))
                got = obs.drain()
                assert [s.sec for s in got] == plan[-1][1] and len(syncs) - before == len(got)   # one each
                seconds += got
        r = dict(spectra=obs.spectra(), evs=None, fs=fs, J=J, K=R)
        if ring:
            seconds += obs.drain(final=True)
            r.update(seconds=seconds, plan=plan, overrun=obs.overrun(), early=obs.early(), outside=obs.outside())
            for name in ('image', 'rows', 'photons'):
                with pytest.raises(ValueError, match='Second'):
                    getattr(obs, name)(*((0,) if name == 'rows' else (0, 0) if name == 'photons' else ()))
        else:
            r.update(image=obs.image(), rows=[obs.rows(s) for s in range(n_seconds)], outside=obs.outside(),
                     photons={(s, p): obs.photons(s, p) for s in range(n_seconds) for p in range(C)},
                     packed=[obs.packed(s) for s in range(n_seconds)])
            with pytest.raises(ValueError):
                obs.drain()
        torch.cuda.synchronize()
        r['evs'] = [d_ev[:int(d_cnt[1].item())].cpu().numpy().view(np.uint64) for _, d_ev, d_cnt in bufs]
        return r
    finally:
        ch.close()


def _same_second(sec, rows, photons, K):
    """A drained Second against rows(sec) / photons(sec, p) of the run without a ring: words, stamps,
    us, and the finite heights (and their dt) bit for bit, NaN where the other is NaN."""
    got_rows = sec.rows()
    assert len(got_rows) == C and np.array_equal(np.diff(sec.offsets), np.minimum(sec.counts, K))
    for p in range(C):
        ph, mine = photons[(sec.sec, p)], sec.row(p)
        assert np.array_equal(got_rows[p], rows[sec.sec][p]) and np.array_equal(mine['word'], ph['word']), (sec.sec, p)
        assert np.array_equal(mine['stamp'], ph['stamp']) and np.array_equal(mine['us'], ph['us'])
        for f in ('height', 'dt'):
            assert np.array_equal(np.isnan(mine[f]), np.isnan(ph[f])), (sec.sec, p, f)
            fin = ~np.isnan(ph[f])
            assert np.array_equal(mine[f][fin].view(np.uint32), ph[f][fin].view(np.uint32)), (sec.sec, p, f)


@pytest.mark.parametrize('photon_rows', [16, 2])
def test_observation_end_to_end(gpu, photon_rows):
    """photon_rows = 16 is the run as it was set. Its densest pixel-second holds 3 packets (324
    packets in 1024 rows of 64 channels), so no row of 16 slots overflows; the same run with
    photon_rows = 2 is here for that witness."""
    plain = _run_observation(None, 6, photon_rows)
    # the witnesses: at least four seconds hold packets, and at least one row overflows K
    print('packets per second', plain['image'].sum(axis=1), 'densest cell', plain['image'].max())
    assert (plain['image'].sum(axis=1) > 0).sum() >= 4
    assert photon_rows == 16 or (plain['image'] > photon_rows).any()
    for s, pk in enumerate(plain['packed']):              # packed(sec): the same readout of the unbounded tables
        _same_second(pk, plain['rows'], plain['photons'], plain['K'])
        assert pk.sec == s and np.array_equal(pk.counts, plain['image'][s])
    # ring = 3: long enough for this run drained after every step
    a = _run_observation(3, 6, photon_rows)
    assert a['overrun'] == 0 and a['early'] == 0 and [s.sec for s in a['seconds']] == list(range(6))
    for sec in a['seconds']:
        _same_second(sec, plain['rows'], plain['photons'], plain['K'])
        assert np.array_equal(sec.counts, plain['image'][sec.sec])
    assert np.array_equal(a['spectra'], plain['spectra']) and np.array_equal(a['outside'][:2], plain['outside'])
    assert all(np.array_equal(x, y) for x, y in zip(a['evs'], plain['evs']))
    # ring = 2: the packets whose second had no slot are counted, and every drained second is still exact
    b = _run_observation(2, 6, photon_rows)
    tb = packets.Timebase(b['fs'], N)
    missed, lost = 0, {}
    for k, ev in enumerate(b['evs']):
        sec0 = b['plan'][k][0]
        kind, sec, ch = rc_.ring_kind(ev, k * b['J'], N, b['fs'], C, (sec0, 2, 6))
        missed += int((kind == rc_.OVERRUN).sum())
        for s, p in zip(sec[kind == rc_.OVERRUN].tolist(), ch[kind == rc_.OVERRUN].tolist()):
            lost[(s, p)] = lost.get((s, p), 0) + 1
    assert b['overrun'] == missed > 0 and b['early'] == 0 and [s.sec for s in b['seconds']] == list(range(6))
    assert np.array_equal(b['spectra'], plain['spectra'])
    for sec in b['seconds']:
        if not any(s == sec.sec for s, _ in lost):
            _same_second(sec, plain['rows'], plain['photons'], plain['K'])
            continue
        # a second that lost packets: the restatement over the packets that found their slot
        cells = {}
        for k, ev in enumerate(b['evs']):
            keep = rc_.ring_kind(ev, k * b['J'], N, b['fs'], C, (b['plan'][k][0], 2, 6))[0] == rc_.IN
            pc.rows_ref(ev[keep], k * b['J'], N, b['fs'], C, 6, b['K'], pc.REFERENCE, cells)
        for p in range(C):
            lst = cells.get((sec.sec, p), [])
            assert sec.counts[p] == len(lst) == plain['image'][sec.sec, p] - lost.get((sec.sec, p), 0)
            assert np.array_equal(sec.row(p)['word'], np.array([w for w, _ in lst[:b['K']]], np.uint64))
            assert np.array_equal(sec.row(p)['stamp'], np.array([j for _, j in lst[:b['K']]], np.int64))
            known = {j: h for j, h in zip(plain['photons'][(sec.sec, p)]['stamp'].tolist(), plain['photons'][(sec.sec, p)]['height'])}
            for j, h in zip(sec.row(p)['stamp'].tolist(), sec.row(p)['height']):
                if j in known and np.isfinite(known[j]):
                    assert h.tobytes() == known[j].tobytes()
