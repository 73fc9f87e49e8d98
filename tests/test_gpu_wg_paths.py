"""The one-workgroup scans between the sliced kernels, and the workgroup ranks, where more than one
wave is live: k_ph_scan (k_photons.hip), k_obs_scan and k_obs_scatter (k_observe.hip) at list lengths
that give 1, 2, 63, 64, 65, 128, 1023 and 1024 slices, and k_pk_scan (k_pack.hip) at 256, 512 and 2048
channels. Every output is compared byte for byte with the host twins, which the CPU suite holds
against the numpy restatements at small sizes; the lists are made in numpy, channel-major and
time-ascending. The longest list is 2.1 million packets, the smallest at which every thread of the
scans carries a slice.
"""
import functools

import numpy as np
import pytest

import observe_cases as oc
import photon_cases as pc
import ring_cases as rc_
from mkids_sdr_amd import _lib, packets

pytestmark = pytest.mark.gpu
C = 64
N = 2 * C
SLICE, MAX_BLOCKS, THREADS = 2048, 1024, 256     # csrc/pkt_common.h kObsSlice, kObsMaxBlocks; kObsThreads = kPhThreads
SLICES = [1, 2, 63, 64, 65, 128, 1023, 1024]
NBINS = 16
LIST_FIELDS = ('image', 'outside', 'words', 'stamps', 'dropped')
TABLE_FIELDS = LIST_FIELDS + ('height', 'dt', 'fill')


@pytest.fixture(scope='module')
def ctxs(gpu):
    """Contexts by channel count: one of 64 channels for the lists, one each for the pack sizes."""
    from mkids_sdr_amd.channelizer import Channelizer
    made = {}

    def get(nch=C):
        if nch not in made:
            made[nch] = Channelizer(nch, max_chunk=2 ** 14, sample_rate=oc.FS)
        return made[nch]

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


def cut(n, threads=THREADS):
    """pkt::slices -> (blocks, slice)."""
    want = (n + SLICE - 1) // SLICE
    blocks = min(max(want, 1), MAX_BLOCKS)
    per = (n + blocks - 1) // blocks
    return blocks, (per + threads - 1) // threads * threads


def length(blocks):
    """A list length that gives `blocks` slices of kObsSlice, the last one not full."""
    n = blocks * SLICE - 37
    assert cut(n) == (blocks, SLICE)
    return n


def quiet_slices(blocks):
    """Slices that get no deferred packet: the first of the list, the first of wave 1, one in the
    middle and the last but one."""
    return sorted({b for b in (0, 64, blocks // 2, blocks - 2) if 0 <= b < blocks}) if blocks >= 3 else []


@functools.lru_cache(maxsize=None)
def packet_list(blocks):
    """-> (ev, h): length(blocks) packets in the device's order over seconds 0 .. 2 and a little of
    the third, 2 % of them (3000 at the most) of channels >= C, and channel 5 with a run in second 1 that is longer than
    a slice (three quarters of the list where the list is shorter than that). With 256 cells for
    129 000 packets and more, the runs of most cells cross slices and waves. The heights have every
    special value, and none that is not finite in quiet_slices."""
    n = length(blocks)
    rng = np.random.default_rng(400 + blocks)
    tb = packets.Timebase(oc.FS, N)
    heavy = min(3 * n // 4, SLICE + 700)
    m = n - heavy
    ch = np.where(rng.random(m) < min(0.02, 3000 / n), rng.integers(C, 4096, m), rng.integers(0, C, m))
    ch = np.concatenate([ch, np.full(heavy, 5)])
    jg = np.concatenate([rng.integers(0, tb.first_row(3) + 50, m), rng.integers(tb.first_row(1), tb.first_row(2), heavy)])
    ev = oc.device_order(oc.pack(ch, jg, rng), 0)
    h = oc.heights_for(n, rng)
    for b in quiet_slices(blocks):
        h[b * SLICE:(b + 1) * SLICE] = 1.0
    return ev, h                    # shared by the tests, which leave them as they are


def row_slots(n):
    """About the mean length of a cell's row, so that many rows overflow and many do not."""
    return max(n // (3 * C), 2)


# ---- the photon rows: k_ph_scan ---------------------------------------------------------------------
def _list_parity(ctx, ev, win, K, layout, count=None, cap=None):
    """The plain form (win None: three seconds) or the ring form into fresh tables against its twin."""
    m = len(ev) if count is None else max(min(count, cap), 0)
    if win is None:
        want = pc.Tables(3, C, K)
        assert pc.list_host(ev[:m], 0, N, oc.FS, C, 3, K, layout, want)[0] == 0
        rest = (0, 3, K, layout)
        plain, counted = ctx.list_photons_device, ctx.list_photons_counted
    else:
        want = rc_.RingTables(win[1], C, K)
        assert rc_.list_ring_host(ev[:m], 0, N, oc.FS, C, win, K, layout, want)[0] == 0
        rest = (0, win[0], win[1], win[2], K, layout)
        plain, counted = ctx.list_photons_ring_device, ctx.list_photons_ring_counted
    fresh = type(want)(want.n_seconds, C, K)
    d = {k: _dev(getattr(fresh, k)) for k in LIST_FIELDS}
    outs = tuple(d[k] for k in LIST_FIELDS)
    d_ev = _dev(ev)
    if count is None:
        plain(d_ev, len(ev), *rest, *outs)
    else:
        counted(d_ev, _dev(np.array([count], np.int64)), cap, *rest, *outs)
    bad = [k for k in LIST_FIELDS if not np.array_equal(_host(d[k], getattr(want, k)), getattr(want, k))]
    assert bad == [], (bad, len(ev), win, K, layout, count, cap)
    return want


@pytest.mark.parametrize('blocks', SLICES)
def test_photon_rows_across_waves(ctxs, blocks):
    """mkid_list_photons over three seconds and mkid_list_photons_ring over seconds 1 and 2 of them in
    a ring of 2: image, outside, words, stamps and dropped."""
    ev, _ = packet_list(blocks)
    K = row_slots(len(ev))
    plain = _list_parity(ctxs(), ev, None, K, pc.WIDE)
    ring = _list_parity(ctxs(), ev, (1, 2, 3), K, pc.REFERENCE)
    assert plain.image.sum() + plain.outside.sum() == len(ev) == ring.image.sum() + ring.outside.sum()
    assert plain.image[1, 5] > min(SLICE, len(ev) // 2)                     # the run longer than a slice
    if blocks > 2:                  # non-pixel, late and early packets (the overrun kind needs a shorter ring)
        assert plain.dropped[0] > 0 and ring.dropped[0] > 0 and (plain.image <= K).any() and ring.outside[:3].min() > 0


# ---- the spectra's deferred list: k_obs_scan, k_obs_scatter --------------------------------------------
J_DEFER = 40                        # stamps on both sides of it in every channel


class Deferred:
    """The outputs of mkid_height_spectra that continue from call to call, on the host: for the twin."""

    def __init__(self, size):
        self.spectra = np.zeros((C, NBINS + 3), np.int32)
        self.deferred = np.full(max(size, 1), 0x7777, np.uint64)
        self.ndef = np.zeros(2, np.int64)

    NAMES = ('spectra', 'deferred', 'ndef')


def _spectra_call(ctx, ev, h, bins, d, want, cap_def, count=None, cap=None):
    """One call on the device buffers d and on the twin's `want`, then every output compared."""
    lo, inv = bins
    m = len(ev) if count is None else max(min(count, cap), 0)
    if 'ev' not in d:
        d.update(ev=_dev(ev), h=_dev(h), lo=_dev(lo), inv=_dev(inv))
    args = (0, J_DEFER, d['lo'], d['inv'], NBINS, d['spectra'], d['deferred'], cap_def, d['ndef'])
    if count is None:
        ctx.height_spectra_device(d['ev'], d['h'], len(ev), *args)
    else:
        ctx.height_spectra_counted(d['ev'], d['h'], _dev(np.array([count], np.int64)), cap, *args)
    p = oc._p
    rc = _lib.load().mkid_height_spectra_host(p(np.ascontiguousarray(ev[:m])), p(np.ascontiguousarray(h[:m])), m, 0, J_DEFER,
                                              C, p(lo), p(inv), NBINS, p(want.spectra), p(want.deferred), cap_def,
                                              p(want.ndef))
    assert rc == 0
    bad = [k for k in Deferred.NAMES if not np.array_equal(_host(d[k], getattr(want, k)), getattr(want, k))]
    assert bad == [], (bad, len(ev), cap_def, count, cap, want.ndef)


def _qualified(ev, h):
    ch, jg = oc.decode(ev, 0)
    return (ch < C) & ~np.isfinite(h) & (jg >= J_DEFER)


@pytest.mark.parametrize('blocks', SLICES)
def test_deferred_list_across_waves(ctxs, blocks):
    """mkid_height_spectra with a deferred list: the spectra, the deferred words in the list's order and
    both counts. cap_def above the total; then, on buffers of their own, cap_def inside the list and
    two more calls on the same counts, so that the scan starts from ndef[1] > 0 and ends below cap_def,
    above it from below, and above it from above."""
    ev, h = packet_list(blocks)
    q = _qualified(ev, h)
    nq = int(q.sum())
    per_slice = np.add.reduceat(q.astype(np.int64), np.arange(0, len(ev), SLICE))
    tail = int(np.argmax(oc.decode(ev, 0)[0] >= C))       # the channels >= C end the list: at most two slices of them
    empty = set(quiet_slices(blocks)) | {b for b in range(blocks) if b * SLICE >= tail}
    assert len(per_slice) == blocks and set(np.flatnonzero(per_slice == 0).tolist()) == empty and nq > 20
    assert len(empty) <= 6
    bins = oc.bins(C, NBINS, np.random.default_rng(7))
    size = 3 * nq + 8
    for caps in ((nq + 5,), (nq // 2, 2 * nq, 2 * nq + nq // 3, nq)):
        want = Deferred(size)
        d = {k: _dev(getattr(want, k)) for k in Deferred.NAMES}
        for cap_def in caps:
            _spectra_call(ctxs(), ev, h, bins, d, want, cap_def)
    assert list(want.ndef) == [4 * nq, 2 * nq + nq // 3]      # nq/2; + nq < 2 nq; cut at the cap; left above the cap


def test_counted_forms_across_waves(ctxs):
    """*d_count at 40 slices of a capacity of 128: the slices past the count are empty."""
    ev, h = packet_list(128)
    count = 40 * SLICE - 300
    _list_parity(ctxs(), ev, None, row_slots(count), pc.REFERENCE, count=count, cap=len(ev))
    _list_parity(ctxs(), ev, (1, 2, 3), row_slots(count), pc.WIDE, count=count, cap=len(ev))
    nq = int(_qualified(ev[:count], h[:count]).sum())
    want = Deferred(nq + 8)
    d = {k: _dev(getattr(want, k)) for k in Deferred.NAMES}
    bins = oc.bins(C, NBINS, np.random.default_rng(8))
    _spectra_call(ctxs(), ev, h, bins, d, want, nq + 5, count=count, cap=len(ev))
    _spectra_call(ctxs(), ev, h, bins, d, want, nq + 5, count=count, cap=len(ev))
    assert list(want.ndef) == [2 * nq, nq + 5]


# ---- mkid_pack_second, mkid_clear_second: k_pk_scan -----------------------------------------------------
def _pack(ctx, t, d, sec, cap_out, size):
    p = rc_.Packed(t.C, size)
    dp = {k: _dev(getattr(p, k)) for k in rc_.Packed.NAMES}
    ctx.pack_second(sec, t.n_seconds, t.K, d['image'], d['words'], d['stamps'], d['height'], d['dt'], cap_out,
                    dp['counts'], dp['offsets'], dp['words'], dp['stamps'], dp['height'], dp['dt'], dp['total'])
    for k in rc_.Packed.NAMES:
        setattr(p, k, _host(dp[k], getattr(p, k)))
    return p


@pytest.mark.parametrize('nch', [256, 512, 2048])
def test_pack_and_clear_across_waves(ctxs, nch):
    """One, two and eight full waves of k_pk_scan at four channels a thread: rows empty, partly
    filled, full and counted past K, every slot of the tables random; counts, offsets (entry C
    included), the four packed arrays and total, with cap_out above the total and inside it; then
    mkid_clear_second, whole tables."""
    ctx, K, R = ctxs(nch), 6, 2
    rng = np.random.default_rng(500 + nch)
    t = rc_.RingTables(R, nch, K)
    t.image[:] = rng.choice(np.array([0, 0, 1, 3, K, K + 1, 5 * K, -2], np.int32), (R, nch))   # -2: wrapped, a full row
    t.image[1, ::64] = K + 2                             # the first channel of every 16th thread, lane 0 of a wave among them
    shape = (R, nch, K)
    t.words[:] = rng.integers(0, 1 << 63, shape, dtype=np.int64).view(np.uint64)
    t.stamps[:] = rng.integers(0, 1 << 40, shape)
    t.height.view(np.uint32)[:] = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    t.dt.view(np.uint32)[:] = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    d = {k: _dev(getattr(t, k)) for k in TABLE_FIELDS}
    total = int(np.minimum(t.image[1].view(np.uint32).astype(np.int64), K).sum())
    assert total > nch
    for cap_out in (total + 3, total // 2 + 1):
        got = _pack(ctx, t, d, 1 + R * 5, cap_out, total + 4)
        rc, want = rc_.pack_host(t, 1 + R * 5, cap_out=cap_out, size=total + 4)
        assert rc == 0 and got.differs(want) == [], (got.differs(want), nch, cap_out)
        assert list(want.total) == [total, min(total, cap_out)] and want.offsets[nch] == total
    want = rc_.RingTables(R, nch, K)
    for k in TABLE_FIELDS:
        getattr(want, k)[...] = getattr(t, k)
    ctx.clear_second(3, R, K, d['image'], d['height'], d['dt'])
    assert rc_.clear_host(want, 3) == 0
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    bad = [k for k in TABLE_FIELDS if not np.array_equal(bits(_host(d[k], getattr(want, k))), bits(getattr(want, k)))]
    assert bad == [] and not want.image[1].any() and want.image[0].any()
