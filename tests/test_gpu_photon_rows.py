"""mkid_list_photons and mkid_fill_photon_heights on the device (k_photons.hip) against the host
twins, which tests/test_photon_rows_host.py holds against the numpy restatement and the
WireStream -> PacketMaster path. Everything is an integer or a float copied bit for bit, and every
comparison is exact: the five outputs with d_image and d_outside, the poison of every slot that must
not be written, both fill counters. Then the kernels' own edges (tiny lists, one slice, the slice
cap of the grid, a run over several slices, a cell change at every packet, device-side counts, a
row that fills inside a call and at a call boundary, a list in another order) and a streamed run
through observe.Observation(photon_rows=...) with no host synchronisation between calls.
"""
import numpy as np
import pytest

import observe_cases as oc
import photon_cases as pc
from mkids_sdr_amd import _lib, observe, packets

pytestmark = pytest.mark.gpu
C = 64
N = 2 * C
SLICE, MAX_BLOCKS = 2048, 1024      # csrc/pkt_common.h kObsSlice, kObsMaxBlocks


@pytest.fixture(scope='module')
def ctxs(gpu):
    """Contexts by (C, fs): the sample clock is part of a context's configuration."""
    from mkids_sdr_amd.channelizer import Channelizer
    made = {}

    def get(nch=C, fs=oc.FS):
        if (nch, fs) not in made:
            made[(nch, fs)] = Channelizer(nch, max_chunk=2 ** 14, sample_rate=fs)
        return made[(nch, fs)]

    yield get
    for ch in made.values():
        ch.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    torch.cuda.synchronize()     # torch's stream made it, the context's stream reads it
    return t


def _host(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


FIELDS = ('image', 'outside', 'words', 'stamps', 'dropped', 'height', 'dt', 'fill')


class DevTables:
    """A photon_cases.Tables on the device."""

    def __init__(self, t):
        self.shape = (t.n_seconds, t.C, t.K)
        for k in FIELDS:
            setattr(self, k, _dev(getattr(t, k)))

    def host(self):
        t = pc.Tables(*self.shape)
        for k, a in zip(FIELDS, _host(*(getattr(self, k) for k in FIELDS))):
            setattr(t, k, a.view(np.uint64) if k == 'words' else a)
        return t


def dev_list(ctx, ev, j0, n_seconds, K, layout, t=None, count=None, cap=None):
    """Device list into a copy of Tables t (a fresh one when None) -> Tables on the host."""
    d = DevTables(pc.Tables(n_seconds, ctx.C, K) if t is None else t)
    d_ev = _dev(ev) if len(ev) else None
    rest = (j0, n_seconds, K, layout, d.image, d.outside, d.words, d.stamps, d.dropped)
    if count is None:
        ctx.list_photons_device(d_ev, len(ev), *rest)
    else:
        ctx.list_photons_counted(d_ev, _dev(np.array([count], np.int64)), cap, *rest)
    return d.host()


def dev_fill(ctx, ev, h, dt, j0, j_defer, t, row_dt=True, count=None, cap=None):
    """Device fill into a copy of Tables t -> Tables on the host."""
    d = DevTables(t)
    d_ev, d_h = (_dev(ev), _dev(np.asarray(h, np.float32))) if len(ev) else (None, None)
    d_dt = None if dt is None or not len(ev) else _dev(np.asarray(dt, np.float32))
    rest = (j0, j_defer, t.n_seconds, t.K, d.image, d.stamps, d.height, d.dt if row_dt else None, d.fill)
    if count is None:
        ctx.fill_photon_heights_device(d_ev, d_h, d_dt, len(ev), *rest)
    else:
        ctx.fill_photon_heights_counted(d_ev, d_h, d_dt, _dev(np.array([count], np.int64)), cap, *rest)
    return d.host()


def _bits(t):
    return [getattr(t, k).view(np.uint32) if k in ('height', 'dt') else getattr(t, k) for k in FIELDS]


def _equal(a, b):
    """Every table of a and b bit for bit (the heights as 32-bit patterns) -> names that differ."""
    return [k for k, x, y in zip(FIELDS, _bits(a), _bits(b)) if not np.array_equal(x, y)]


def _parity(ctx, ev, j0, fs, n_seconds, K, layout, t=None, count=None, cap=None):
    """Device against the host twin, both continuing Tables t."""
    m = len(ev) if count is None else max(min(count, cap), 0)
    got = dev_list(ctx, ev, j0, n_seconds, K, layout, t, count, cap)
    want = pc.Tables(n_seconds, ctx.C, K) if t is None else t
    want = _copy(want)
    assert pc.list_host(ev[:m], j0, ctx.N, fs, ctx.C, n_seconds, K, layout, want)[0] == 0
    assert _equal(got, want) == [], (_equal(got, want), len(ev), K, layout, count, cap)
    return got


def _copy(t):
    c = pc.Tables(t.n_seconds, t.C, t.K)
    for k in FIELDS:
        setattr(c, k, getattr(t, k).copy())
    return c


CASES = pc.cases(C, N)


@pytest.mark.parametrize('layout', pc.LAYOUTS)
@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_parity_case_table(ctxs, c, layout):
    ctx = ctxs(C, c['fs'])
    for K in c['Ks']:
        if c['name'] == 'shuffled':      # not the device's order: the counters, and with room the rows as sets
            for K2 in (K, 64):
                t = dev_list(ctx, c['ev'], c['j0'], c['n_seconds'], K2, layout)
                _, want = pc.list_host(c['ev'], c['j0'], N, c['fs'], C, c['n_seconds'], K2, layout)
                assert t.same(want, ('image', 'outside', 'dropped')) == []
            assert t.dropped[0] == 0 and all(t.pairs(s, p) == want.pairs(s, p) for s in range(4) for p in range(C))
        else:
            t = _parity(ctx, c['ev'], c['j0'], c['fs'], c['n_seconds'], K, layout)
        d_image, d_out = _dev(np.zeros((c['n_seconds'], C), np.int32)), _dev(np.zeros(2, np.int64))
        ctx.count_photons_device(_dev(c['ev']) if len(c['ev']) else None, len(c['ev']), c['j0'], c['n_seconds'], d_image,
                                 d_out)                                           # mkid_count_photons, same list
        image, outside = _host(d_image, d_out)
        assert np.array_equal(t.image, image) and np.array_equal(t.outside, outside)
        assert t.image.sum() + t.outside.sum() == len(c['ev'])


def _long_list(n, seed, nch=C):
    """n packets in the device's order over two seconds and a little of the third, channels >= nch
    among them."""
    rng = np.random.default_rng(seed)
    tb = packets.Timebase(oc.FS, 2 * nch)
    ch = np.where(rng.random(n) < 0.02, rng.integers(nch, 4096, n), rng.integers(0, nch, n))
    return oc.device_order(oc.pack(ch, rng.integers(0, tb.first_row(2) + 50, n), rng), 0)


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 256, 257, SLICE - 1, SLICE, SLICE + 5, 2 * SLICE + 300])
def test_list_lengths(ctxs, n):
    ev = _long_list(n, 60 + n)
    for K, layout in ((3, pc.WIDE), (100, pc.REFERENCE)):    # about n / 128 packets a cell, 34 at the most
        t = _parity(ctxs(), ev, 0, oc.FS, 2, K, layout)
        assert n < SLICE or (K == 3) == (t.dropped[0] > 0)


def test_past_the_slice_cap(ctxs):
    """More packets than kObsMaxBlocks slices of kObsSlice: the slices grow. Two runs, the same bits."""
    ev = _long_list(MAX_BLOCKS * SLICE + 300, 61)
    a = _parity(ctxs(), ev, 0, oc.FS, 2, 9, pc.WIDE)
    assert a.dropped[0] > len(ev) // 2 and a.image.min() > 9
    assert _equal(dev_list(ctxs(), ev, 0, 2, 9, pc.WIDE), a) == []


@pytest.mark.parametrize('K', [4, 3 * SLICE + 100])
def test_one_run_over_several_slices(ctxs, K):
    """One cell's run of 3 SLICE + 100 packets, behind and before short runs of other channels: its
    head lies three slices back. K small drops most of it, K = its length none."""
    rng = np.random.default_rng(62)
    n = 3 * SLICE + 100
    assert packets.Timebase(oc.FS, N).second(n + 10) == 0
    ev = np.concatenate([oc.pack(np.full(7, 2), np.arange(7), rng), oc.pack(np.full(n, 5), 3 + np.arange(n), rng),
                         oc.pack(np.full(9, 6), np.arange(9), rng)])
    t = _parity(ctxs(), ev, 0, oc.FS, 1, K, pc.WIDE)
    assert t.image[0, 5] == n and t.dropped[0] == max(n - K, 0) + (3 + 5 if K == 4 else 0)


def test_every_packet_changes_cell(ctxs):
    """Channels cycling with every packet, stamps ascending: 3 SLICE runs of length one. Each cell's
    packets come in ascending stamp, but as runs of their own, so its row is compared as a set."""
    rng = np.random.default_rng(63)
    n = 3 * SLICE
    ev = oc.pack(np.arange(n) % C, np.arange(n), rng)
    K = n // C + 1
    got = dev_list(ctxs(), ev, 0, 1, K, pc.WIDE)
    _, want = pc.list_host(ev, 0, N, oc.FS, C, 1, K, pc.WIDE)
    assert got.same(want, ('image', 'outside', 'dropped')) == [] and got.image.min() == n // C
    for p in range(C):
        assert got.pairs(0, p) == want.pairs(0, p)
    assert np.all(got.words[0, :, K - 1] == pc.POISON_W) and np.all(got.stamps[0, :, K - 1] == pc.POISON_S)
    # and in runs of one the small-K outputs that stay exact
    small = dev_list(ctxs(), ev, 0, 1, 5, pc.WIDE)
    _, hsmall = pc.list_host(ev, 0, N, oc.FS, C, 1, 5, pc.WIDE)
    assert small.same(hsmall, ('image', 'outside', 'dropped')) == [] and small.dropped[0] == n - 5 * C


def test_counted_forms(ctxs):
    """*d_count below, at and above cap, negative and 0; the entries past the count are packets of
    pixels, the one right after the last valid packet of its cell among them, and are never read;
    the slots past min(count, K) keep their poison (the tables are compared whole)."""
    ctx = ctxs()
    ev = _long_list(3000, 64)
    ch, jg = oc.decode(ev, 0)
    sec = packets.Timebase(oc.FS, ctx.N).second(jg)
    same = np.flatnonzero((ch[1:] == ch[:-1]) & (sec[1:] == sec[:-1]) & (ch[1:] < C)) + 1
    assert same.size > 100
    for count, cap in ((int(same[same.size // 2]), 3000), (int(same[5]), 2900), (5000, 2000), (0, 3000), (1, 3000),
                       (3000, 3000), (-4, 3000), (2100, 2100)):
        for K in (2, 30):
            t = _parity(ctx, ev, 0, oc.FS, 2, K, pc.REFERENCE, count=count, cap=cap)
            assert t.image.sum() + t.outside.sum() == max(min(count, cap), 0)


def test_prefix_contribution(ctxs):
    """A stream in several calls equals one call, the tables continued on the device: pixel 5 fills
    its K = 10 slots inside the second call of one cut and exactly at the end of the first call of
    the other."""
    ctx = ctxs()
    rng = np.random.default_rng(65)
    K = 10
    mine = oc.pack(np.full(30, 5), np.arange(100, 130), rng)
    others = oc.pack(rng.integers(6, C, 300), rng.integers(100, 130, 300), rng)
    full = oc.device_order(np.concatenate([mine, others]), 0)
    one = _parity(ctx, full, 0, oc.FS, 1, K, pc.WIDE)
    assert one.image[0, 5] == 30 and np.array_equal(one.stamps[0, 5], np.arange(100, 110))
    for cuts in ((110, 117), (104, 115), (101, 102, 103, 110, 111)):
        t = pc.Tables(1, C, K)
        edges = [0] + list(cuts) + [1 << 20]
        for a, b in zip(edges[:-1], edges[1:]):
            jg = oc.decode(full, 0)[1]
            t = _parity(ctx, full[(jg >= a) & (jg < b)], a, oc.FS, 1, K, pc.WIDE, t)
        assert _equal(t, one) == [], cuts


def test_unordered_list(ctxs):
    """The same packets by ascending stamp, channels mixed: image, outside and dropped are exact
    for any K; with K large enough that nothing drops, every row holds the same (stamp, word) pairs."""
    ctx = ctxs()
    rng = np.random.default_rng(66)
    ev = _long_list(6000, 67)
    by_stamp = ev[np.argsort(oc.decode(ev, 0)[1], kind='stable')]
    by_stamp = np.concatenate([by_stamp[:3000], rng.permutation(by_stamp[3000:])])
    for layout in pc.LAYOUTS:
        for K in (4, 200):
            want = _parity(ctx, ev, 0, oc.FS, 2, K, layout)
            got = dev_list(ctx, by_stamp, 0, 2, K, layout)
            assert got.same(want, ('image', 'outside', 'dropped')) == []
            assert (K == 4) == (want.dropped[0] > 0)
            if K == 200:
                for s in range(2):
                    for p in range(C):
                        assert got.pairs(s, p) == want.pairs(s, p), (s, p)
                assert np.array_equal(got.words == pc.POISON_W, want.words == pc.POISON_W)


def _fill_case(seed, n=3000, K=6):
    """Tables listed on the host from a device-order list of distinct (ch, stamp), and heights with
    every special value on both sides of j_defer."""
    rng = np.random.default_rng(seed)
    tb = packets.Timebase(oc.FS, N)
    ch = np.where(rng.random(n) < 0.05, rng.integers(C, 4096, n), rng.integers(0, C, n))
    ev = oc.device_order(pc.unique_packets(ch, rng.integers(0, tb.first_row(2) + 400, n), rng), 0)
    rc, t = pc.list_host(ev, 0, N, oc.FS, C, 2, K, pc.WIDE)
    assert rc == 0 and t.dropped[0] > 0 and t.outside.min() > 0
    h = oc.heights_for(len(ev), rng)
    h[::11] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]          # a NaN with a payload
    dt = rng.normal(size=len(ev)).astype(np.float32)
    dt[::13] = np.nan
    return ev, h, dt, t, tb.first_row(1) + 200


@pytest.mark.parametrize('with_dt', [True, False])
def test_fill_parity(ctxs, with_dt):
    ev, h, dt, t, jd = _fill_case(68)
    ch, jg = oc.decode(ev, 0)
    assert ((jg >= jd) & ~np.isfinite(h) & (ch < C)).sum() > 50 and ((jg < jd) & ~np.isfinite(h) & (ch < C)).sum() > 50
    want = _copy(t)
    assert pc.fill_host(ev, h, dt if with_dt else None, 0, jd, N, oc.FS, C, want) == 0
    got = dev_fill(ctxs(), ev, h, dt if with_dt else None, 0, jd, t, row_dt=with_dt)
    assert _equal(got, want) == []
    assert got.fill[1] >= t.dropped[0] // 2 and got.fill[0] > 400 and (np.isnan(got.dt).all() != with_dt)
    assert (got.height.view(np.uint32) == 0x7FC12345).any() and np.isinf(got.height).any()
    again = dev_fill(ctxs(), ev, h, dt if with_dt else None, 0, jd, t, row_dt=with_dt)      # the same bits
    assert _equal(again, got) == []
    rng = np.random.default_rng(69)
    p = rng.permutation(len(ev))                                                 # any list order
    assert _equal(dev_fill(ctxs(), ev[p], h[p], dt[p] if with_dt else None, 0, jd, t, row_dt=with_dt), got) == []
    # a dt list without a dt table, and the reverse, write no dt
    assert _equal(dev_fill(ctxs(), ev, h, dt, 0, jd, t, row_dt=False), dev_fill(ctxs(), ev, h, None, 0, jd, t)) == []


def test_fill_counted_and_lengths(ctxs):
    ev, h, dt, t, jd = _fill_case(70)
    for count, cap in ((1000, len(ev)), (len(ev) + 50, len(ev) - 7), (0, len(ev)), (-1, len(ev)), (257, 300)):
        m = max(min(count, cap), 0)
        want = _copy(t)
        assert pc.fill_host(ev[:m], h[:m], dt[:m], 0, jd, N, oc.FS, C, want) == 0
        assert _equal(dev_fill(ctxs(), ev, h, dt, 0, jd, t, count=count, cap=cap), want) == [], (count, cap)
    for n in (0, 1, 255, 256, 257):
        want = _copy(t)
        assert pc.fill_host(ev[:n], h[:n], dt[:n], 0, jd, N, oc.FS, C, want) == 0
        assert _equal(dev_fill(ctxs(), ev[:n], h[:n], dt[:n], 0, jd, t), want) == [], n


def _code(fn):
    with pytest.raises(_lib.MkidError) as e:
        fn()
    return e.value.code


def test_argument_errors(ctxs):
    """Every MKID_E_ARG case fails before any launch: the outputs stay as they were."""
    from mkids_sdr_amd.channelizer import Channelizer
    ctx = ctxs()
    ev, h, dt, t, jd = _fill_case(71, n=400)
    d = DevTables(t)
    d_ev, d_h, d_dt = _dev(ev), _dev(h), _dev(dt)
    d_cnt = _dev(np.array([len(ev)], np.int64))

    def lst(**kw):
        a = dict(ev=d_ev, n=len(ev), j0=0, ns=2, K=t.K, layout=pc.WIDE, image=d.image, out=d.outside, words=d.words,
                 stamps=d.stamps, dropped=d.dropped)
        a.update(kw)
        rest = (a['j0'], a['ns'], a['K'], a['layout'], a['image'], a['out'], a['words'], a['stamps'], a['dropped'])
        if 'cnt' in a:
            return ctx.list_photons_counted(a['ev'], a['cnt'], a['n'], *rest)
        return ctx.list_photons_device(a['ev'], a['n'], *rest)

    def fill(**kw):
        a = dict(ev=d_ev, h=d_h, dt=d_dt, n=len(ev), j0=0, jd=jd, ns=2, K=t.K, image=d.image, stamps=d.stamps,
                 height=d.height, rdt=d.dt, fill=d.fill)
        a.update(kw)
        rest = (a['j0'], a['jd'], a['ns'], a['K'], a['image'], a['stamps'], a['height'], a['rdt'], a['fill'])
        if 'cnt' in a:
            return ctx.fill_photon_heights_counted(a['ev'], a['h'], a['dt'], a['cnt'], a['n'], *rest)
        return ctx.fill_photon_heights_device(a['ev'], a['h'], a['dt'], a['n'], *rest)

    common = (dict(ev=None), dict(image=None), dict(stamps=None), dict(n=-1), dict(j0=-1), dict(j0=1 << 62), dict(ns=0),
              dict(ns=(1 << 20) + 1), dict(K=0), dict(K=65537), dict(cnt=None), dict(cnt=d_cnt, n=-1))
    for kw in common + (dict(out=None), dict(words=None), dict(dropped=None), dict(layout=2), dict(layout=-1)):
        assert _code(lambda: lst(**kw)) == _lib.MKID_E_ARG, kw
    for kw in common + (dict(h=None), dict(height=None), dict(fill=None)):
        assert _code(lambda: fill(**kw)) == _lib.MKID_E_ARG, kw
    L = ctx._L
    assert L.mkid_list_photons(None, None, 0, 0, 1, 1, 0, None, None, None, None, None) == _lib.MKID_E_ARG
    assert L.mkid_fill_photon_heights(None, None, None, None, 0, 0, 0, 1, 1, None, None, None, None, None) == _lib.MKID_E_ARG
    # the sample clock: not an integer, and past 2^43; the reference layout with C > 254
    for fs, nch, layout in ((1e6 + 0.5, C, pc.WIDE), (2.0 ** 43 + 2, C, pc.WIDE), (oc.FS, 256, pc.REFERENCE)):
        odd = Channelizer(nch, max_chunk=2 ** 14, sample_rate=fs)
        try:
            assert _code(lambda: odd.list_photons_device(d_ev, len(ev), 0, 2, t.K, layout, d.image, d.outside, d.words,
                                                         d.stamps, d.dropped)) == _lib.MKID_E_ARG
            if nch == C:
                assert _code(lambda: odd.fill_photon_heights_device(d_ev, d_h, d_dt, len(ev), 0, jd, 2, t.K, d.image,
                                                                    d.stamps, d.height, d.dt, d.fill)) == _lib.MKID_E_ARG
        finally:
            odd.close()
    assert _equal(d.host(), t) == []
    # and the valid edges: n == 0 without lists, no dt
    lst(n=0, ev=None)
    fill(n=0, ev=None, h=None, dt=None)
    assert _equal(d.host(), t) == []
    fill(dt=None, rdt=None)
    assert d.host().fill.sum() > 0


def test_observation_end_to_end(gpu):
    """The four-call run of test_gpu_observe.test_observation_end_to_end with the fit, with and
    without photon_rows=16, each process_device followed by Observation.step and no host
    synchronisation until the end (the debug copies come from a third, identical run)."""
    import torch
    import signals
    from mkids_sdr_amd.channelizer import Channelizer
    S, K, ncoeff, pre, nbins, L, R = 2 ** 15, 4, 40, 10, 32, 3, 16
    J = S // (2 * C)
    fs = 2 * C * 600                                    # 600 rows per second: the run crosses second 1
    case = signals.make_case(C, K * S, seed=7, pulses_per_ch=24.0)
    quiet = signals.make_case(C, S, seed=7, pulses_per_ch=0)
    thr = signals.thresholds_from_quiet(quiet, signals.oracle_chain(quiet).process(quiet.iq)['raw'])
    coeff = np.random.default_rng(41).normal(size=(C, ncoeff)).astype(np.float32)
    x = torch.from_numpy(case.iq.reshape(-1)).to('cuda')
    cap = J * C
    runs = []
    for rows, debug in ((None, False), (R, False), (R, True)):
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
            obs = observe.Observation(ch, 2, nbins, -20.0, 40.0 / nbins, cap, cap, fit=True, debug=debug,
                                      photon_rows=rows, row_layout=pc.REFERENCE)
            bufs = [(torch.empty((J, C), dtype=torch.float32, device='cuda'),
                     torch.empty(cap, dtype=torch.int64, device='cuda'),
                     torch.zeros(2, dtype=torch.int64, device='cuda')) for _ in range(K)]
            torch.cuda.synchronize()
            for k, (d_ph, d_ev, d_cnt) in enumerate(bufs):
                ch.process_device(x[2 * k * S:2 * (k + 1) * S], S, d_ph, d_ev, cap, d_cnt)
                obs.step(d_ph, J, k * J, d_ev, d_cnt)
            torch.cuda.synchronize()
            evs = [d_ev[:int(d_cnt[1].item())].cpu().numpy().view(np.uint64) for _, d_ev, d_cnt in bufs]
            r = dict(image=obs.image(), spectra=obs.spectra(), outside=obs.outside(), pending=obs.pending(), evs=evs,
                     steps=obs.steps)
            if rows:
                r.update(rows=[obs.rows(s) for s in range(2)], dropped=obs.dropped(), fill=obs.fill_counts(),
                         photons={(s, p): obs.photons(s, p) for s in range(2) for p in range(C)})
            else:
                with pytest.raises(ValueError):
                    obs.rows(0)
            runs.append(r)
        finally:
            ch.close()
    plain, a, b = runs
    # 1. the feature changes no existing result, and the run repeats bit for bit
    for k in ('image', 'spectra', 'outside', 'pending'):
        assert np.array_equal(plain[k], a[k]) and np.array_equal(a[k], b[k]), k
    assert a['dropped'] == b['dropped'] and np.array_equal(a['fill'], b['fill'])
    for key, ph in a['photons'].items():
        for f in ('word', 'stamp', 'us', 'height', 'dt'):
            assert np.array_equal(ph[f], b['photons'][key][f], equal_nan=True), (key, f)
    # 2. rows(sec) equal the numpy restatement over the run's packets
    cells, outside = {}, np.zeros(2, np.int64)
    for k, ev in enumerate(a['evs']):
        outside += pc.rows_ref(ev, k * J, 2 * C, fs, C, 2, R, pc.REFERENCE, cells)[1]
    ref = pc.tables_ref(cells, outside, 2, C, R)
    kept = np.minimum(a['image'], R)
    assert np.array_equal(a['image'], ref.image) and np.array_equal(a['outside'], ref.outside)
    assert a['dropped'] == ref.dropped[0] and kept.sum() > K * C // 2 and a['image'][1].sum() > 0
    tb = packets.Timebase(fs, 2 * C)
    for s in range(2):
        assert len(a['rows'][s]) == C
        for p in range(C):
            ph = a['photons'][(s, p)]
            assert np.array_equal(a['rows'][s][p], ref.words[s, p, :kept[s, p]]), (s, p)
            assert np.array_equal(ph['word'], a['rows'][s][p]) and np.array_equal(ph['stamp'], ref.stamps[s, p, :kept[s, p]])
            assert np.array_equal(ph['us'], tb.microsecond(ph['stamp'])) and np.all(np.diff(ph['stamp']) > 0)
            assert np.array_equal(packets.decode_wire(ph['word'])['us'], ph['us'] & 0xFFFFF)
    # 3. the debug run's heights: what every packet got in the step that binned it
    got_h, nan_binned = {}, set()
    for joined, h, j0, jd in b['steps']:
        cj, jg = oc.decode(joined, j0)
        for c_, j_, h_ in zip(cj.tolist(), jg.tolist(), h):
            if c_ >= C or (not np.isfinite(h_) and j_ >= jd):
                continue                                            # deferred: it comes again
            assert (c_, j_) not in got_h and (c_, j_) not in nan_binned
            if np.isfinite(h_):
                got_h[(c_, j_)] = h_
            else:
                nan_binned.add((c_, j_))
    pend = set(zip(*(x.tolist() for x in oc.decode(a['pending'], K * J))))
    assert len(pend) == len(a['pending']) > 0
    assert a['spectra'][:, nbins + 2].sum() == len(nan_binned) and a['spectra'].sum() == len(got_h) + len(nan_binned)
    finite = np.zeros(C, np.int64)
    nan_stored = np.zeros(C, np.int64)
    pend_stored = np.zeros(C, np.int64)
    for (s, p), ph in a['photons'].items():
        for j_, h_, d_ in zip(ph['stamp'].tolist(), ph['height'], ph['dt']):
            if np.isfinite(h_):
                # 4. bit for bit the height the debug run recorded for that packet
                assert h_.tobytes() == got_h[(p, j_)].tobytes() and abs(d_) <= L + 0.5
                finite[p] += 1
            else:
                assert ((p, j_) in nan_binned) != ((p, j_) in pend)
                nan_stored[p] += (p, j_) in nan_binned
                pend_stored[p] += (p, j_) in pend
    assert np.array_equal(finite + nan_stored, kept.sum(axis=0) - pend_stored) and finite.sum() > K * C // 2
    # 5. conservation
    n_pix = sum(int((oc.decode(ev, 0)[0] < C).sum()) for ev in a['evs'])
    assert a['fill'].sum() + len(a['pending']) == n_pix == a['spectra'].sum() + len(a['pending'])
    assert a['fill'][0] == finite.sum() + nan_stored.sum()
