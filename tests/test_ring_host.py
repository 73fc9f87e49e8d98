"""The ring of second slots and the packed second through the host twins
(mkid_list_photons_ring_host, mkid_fill_photon_heights_ring_host, mkid_pack_second_host,
mkid_clear_second_host: the loops of csrc/obs_common.h, no device): every drained second against the
unbounded tables of the existing twins and against WireStream -> PacketMaster, the identity with the
existing twins, the four `outside` counters against the numpy restatement, the edges of pack and
clear, and every MKID_E_ARG case. Every comparison is exact.
"""
import numpy as np
import pytest

import observe_cases as oc
import photon_cases as pc
import ring_cases as rc_
from mkids_sdr_amd import _lib, observe, packets

C, N = 64, 128
CASES = pc.cases(C, N)
STREAM = rc_.stream()


def _drains(mode, seed):
    if mode == 'always':
        return lambda k: True
    rng = np.random.default_rng(seed)
    picks = rng.random(1000) < 0.5
    return lambda k: bool(picks[k])


def _stream_runs(K, R, mode, layout, seed):
    st = STREAM
    calls = rc_.cut_calls(st['rows'], np.random.default_rng(seed))
    assert any(r == 1 for _, r in calls) and len(calls) > 5
    ring = rc_.run_stream(st, calls, K, layout, R=R, drain=_drains(mode, seed))
    ref = rc_.run_stream(st, calls, K, layout, keep=ring['kept'])['t']
    return st, calls, ring, ref


@pytest.mark.parametrize('mode', ['always', 'random'])
@pytest.mark.parametrize('R', [1, 2, 3, 4])
@pytest.mark.parametrize('K', [1, 3, 2000])
def test_ring_equals_unbounded_stream(K, R, mode):
    """The multi-second stream in random contiguous calls: every drained Second equals that second
    of the tables the existing twins build without a ring from the packets that found a slot (all of
    them when the ring is long enough: drained at every legal moment, R >= 3 holds a call of up to 80
    rows of 50-row seconds). No packet ever arrives for a drained second: the settled bound."""
    st, calls, ring, ref = _stream_runs(K, R, mode, pc.WIDE, 100 * R + K)
    assert sorted(ring['seconds']) == list(range(rc_.SECONDS))
    for s, got in ring['seconds'].items():
        assert got.differs(rc_.pack_ref(ref, s)) == [], (s, got.differs(rc_.pack_ref(ref, s)))
    assert np.array_equal(ring['t'].outside, ring['kinds'][1:]) and ring['kinds'][rc_.EARLY] == 0
    assert ring['kinds'][rc_.NONPIXEL] > 0 and ring['kinds'].sum() == len(st['ev'])
    if mode == 'always' and R >= 3:
        assert ring['kinds'][rc_.OVERRUN] == 0 and len(ring['kept']) == (oc.decode(st['ev'], 0)[0] < st['C']).sum()
        assert (ref.image > K).any() == (K < 2000)
    if R == 1:
        assert ring['kinds'][rc_.OVERRUN] > 0
    assert ring['t'].dropped[0] == ref.dropped[0]
    assert np.all(ring['t'].image == 0) and np.all(ring['t'].height.view(np.uint32) == rc_.NAN_BITS)   # all cleared
    filled = sum(np.isfinite(p.height[:p.total[1]]).sum() for p in ring['seconds'].values())
    assert filled > (50 if K > 1 and R >= 3 else 0) and len(ring['pending']) > 0


@pytest.mark.parametrize('R', [1, 2, 3, 4])
@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_ring_equals_unbounded_case_table(c, R):
    """photon_cases' table, one call each, for every position of an R-slot window: the seconds inside
    it pack to the bits of the unbounded tables' seconds, the packets outside it are counted by
    kind, and the fill finds exactly the packets the unbounded fill finds in those seconds."""
    jd = c['j0'] + 200
    for K in c['Ks']:
        for layout in pc.LAYOUTS:
            _, ref = pc.list_host(c['ev'], c['j0'], N, c['fs'], C, c['n_seconds'], K, layout)
            assert pc.fill_host(c['ev'], c['h'], c['h'], c['j0'], jd, N, c['fs'], C, ref) == 0
            for sec0 in range(c['n_seconds']):
                win = (sec0, R, c['n_seconds'])
                r, t = rc_.list_ring_host(c['ev'], c['j0'], N, c['fs'], C, win, K, layout)
                assert r == 0 and rc_.fill_ring_host(c['ev'], c['h'], c['h'], c['j0'], jd, N, c['fs'], C, win, t) == 0
                kind = rc_.ring_kind(c['ev'], c['j0'], N, c['fs'], C, win)[0]
                assert np.array_equal(t.outside, rc_.outside_ref(kind))
                for s in range(sec0, min(sec0 + R, c['n_seconds'])):
                    got = rc_.pack_host(t, s)[1]
                    assert got.differs(rc_.pack_ref(ref, s)) == [], (K, layout, sec0, s)


def test_ring_equals_packetmaster():
    """REFERENCE layout: each drained second's rows equal the rows WireStream -> PacketMaster keep
    for that second (max_events = K + 1 keeps K)."""
    st, K, R = STREAM, 3, 3
    calls = rc_.cut_calls(st['rows'], np.random.default_rng(7))
    ring = rc_.run_stream(st, calls, K, pc.REFERENCE, R=R, drain=lambda k: True)
    assert ring['kinds'][rc_.OVERRUN] == 0
    ws = packets.WireStream(st['fs'], st['N'])
    pm = packets.PacketMaster(1, st['C'], rc_.SECONDS, max_events=K + 1)
    for j0, rows in calls + [(st['rows'], 2)]:           # two more rows close the last second
        w = ws.push(rc_.call_packets(st, j0, rows), j0, rows)
        pm.receive(0, (w & np.uint64(0xFFFFFFFF)).astype('>u4').tobytes(), (w >> np.uint64(32)).astype('>u4').tobytes())
    assert pm.sec[0] == rc_.SECONDS
    overflow = 0
    for s, got in ring['seconds'].items():
        assert np.array_equal(np.minimum(got.counts, K), pm.photon_counts[s])
        for p in range(st['C']):
            a, b = got.offsets[p], got.offsets[p + 1]
            assert np.array_equal(got.words[a:b], pm.rows[(0, p)][s]), (s, p)
            overflow += got.counts[p] > K
    assert overflow > 0


def test_identity_with_the_existing_twins():
    """sec0 = 0 and n_slots = sec_end = n_seconds: every output of the ring forms equals the existing
    twins', and outside[2 .. 3] stay 0; over the case table and the stream's calls (tables continued)."""
    def both(ev, h, j0, jd, fs, Cc, Nn, ns, K, layout, t_old, t_new):
        win = (0, ns, ns)
        assert pc.list_host(ev, j0, Nn, fs, Cc, ns, K, layout, t_old)[0] == 0
        assert rc_.list_ring_host(ev, j0, Nn, fs, Cc, win, K, layout, t_new)[0] == 0
        assert pc.fill_host(ev, h, h, j0, jd, Nn, fs, Cc, t_old) == 0
        assert rc_.fill_ring_host(ev, h, h, j0, jd, Nn, fs, Cc, win, t_new) == 0
        assert np.array_equal(t_new.outside[:2], t_old.outside) and not t_new.outside[2:].any()
        assert t_new.same(t_old, ('image', 'words', 'stamps', 'dropped')) == [] and np.array_equal(t_new.fill, t_old.fill)
        for k in ('height', 'dt'):
            assert np.array_equal(getattr(t_new, k).view(np.uint32), getattr(t_old, k).view(np.uint32))

    for c in CASES:
        for K in c['Ks']:
            for layout in pc.LAYOUTS:
                both(c['ev'], c['h'], c['j0'], c['j0'] + 200, c['fs'], C, N, c['n_seconds'], K, layout,
                     pc.Tables(c['n_seconds'], C, K), rc_.RingTables(c['n_seconds'], C, K))
    st = STREAM
    for ns in (rc_.SECONDS, 4):                           # 4: two seconds past the exposure
        t_old, t_new = pc.Tables(ns, st['C'], 3), rc_.RingTables(ns, st['C'], 3)
        for j0, rows in rc_.cut_calls(st['rows'], np.random.default_rng(8)):
            ev = rc_.call_packets(st, j0, rows)
            both(ev, rc_.call_heights(st, ev, j0, j0 + rows - 5)[0], j0, j0 + rows - 5, st['fs'], st['C'], st['N'], ns, 3,
                 pc.WIDE, t_old, t_new)
        assert (t_old.outside[1] > 0) == (ns == 4) and t_old.fill.min() > 0


def test_counters():
    """An input in which each of the four kinds occurs: channels >= C, seconds past the exposure,
    seconds before the window, and seconds the ring has no slot for. Each counter equals the numpy
    restatement, and found + not found + deferred is every packet with ch < C."""
    st = STREAM
    Cc, Nn, fs, K = st['C'], st['N'], st['fs'], 3
    ev = oc.device_order(st['ev'], 0)
    win = (1, 2, 5)                                       # seconds 1, 2 of an exposure of 5: 0 early, 3, 4 overrun, 5 late
    kind = rc_.ring_kind(ev, 0, Nn, fs, Cc, win)[0]
    want = rc_.outside_ref(kind)
    assert want.min() > 0
    r, t = rc_.list_ring_host(ev, 0, Nn, fs, Cc, win, K, pc.WIDE)
    assert r == 0 and np.array_equal(t.outside, want)
    assert t.image.sum() == (kind == rc_.IN).sum() and t.image.sum() + t.outside.sum() == len(ev)
    jd = 120                                              # inside second 2
    h, dt = rc_.call_heights(st, ev, 0, jd)
    ch, jg = oc.decode(ev, 0)
    deferred = (ch < Cc) & ~np.isfinite(h) & (jg >= jd)
    assert rc_.fill_ring_host(ev, h, dt, 0, jd, Nn, fs, Cc, win, t) == 0
    live = (ch < Cc) & ~deferred
    assert t.fill.sum() + deferred.sum() == (ch < Cc).sum() and deferred.sum() > 0
    # not found: the live packets of the other three kinds, and those their row dropped
    assert t.fill[1] == (live & (kind != rc_.IN)).sum() + (live & (kind == rc_.IN)).sum() - t.fill[0]
    assert t.fill[1] >= (live & (kind != rc_.IN)).sum() > 0 and t.fill[0] > 0
    # found: the stored photons that are not deferred
    stored = {(c_, j) for s in range(2) for c_ in range(Cc) for j in t.stamps[s, c_, :min(t.image[s, c_], K)].tolist()}
    assert t.fill[0] == sum((c_, j) in stored for c_, j in zip(ch[live].tolist(), jg[live].tolist()))


def _filled_tables(K=3, R=3):
    """Tables of three slots holding seconds 0 .. 2 of the stream, heights filled."""
    st = STREAM
    ev = oc.device_order(st['ev'], 0)
    win = (0, R, R)
    _, t = rc_.list_ring_host(ev, 0, st['N'], st['fs'], st['C'], win, K, pc.WIDE)
    h, dt = rc_.call_heights(st, ev, 0, 1 << 20)
    assert rc_.fill_ring_host(ev, h, dt, 0, 1 << 20, st['N'], st['fs'], st['C'], win, t) == 0
    return t


def test_pack_edges():
    t = _filled_tables()
    total = int(np.minimum(t.image[1], t.K).sum())
    assert total > 10 and (t.image[1] > t.K).any()
    for cap in (0, 1, total - 1, total, total + 1):       # the buffers are exactly cap entries, then roomier
        for size in (None, total + 5):
            r, got = rc_.pack_host(t, 1, cap, size)
            want = rc_.pack_ref(t, 1, cap, size)
            assert r == 0 and got.differs(want) == [] and list(got.total) == [total, min(total, cap)]
            assert np.all(got.words[min(total, cap):] == pc.POISON_W)
            assert np.all(got.height.view(np.uint32)[min(total, cap):] == rc_.POISON_F)
    # sec and sec + n_slots are the same slot; no stamps and no dt wanted: those outputs keep their poison
    assert rc_.pack_host(t, 1 + 3 * 7)[1].differs(rc_.pack_host(t, 1)[1]) == []
    bare = rc_.pack_host(t, 1, stamps=False, dt=False)[1]
    assert bare.differs(rc_.pack_ref(t, 1, stamps=False, dt=False)) == [] and np.all(bare.stamps == pc.POISON_S)
    assert r == 0 and _lib.load().mkid_pack_second_host(1, 3, t.K, t.C, oc._p(t.image), oc._p(t.words), None, oc._p(t.height),
                                                        None, 0, oc._p(got.counts), oc._p(got.offsets), None, None, None,
                                                        None, oc._p(got.total)) == 0      # cap_out 0: no outputs
    # an empty second
    e = rc_.RingTables(2, 5, 4)
    r, got = rc_.pack_host(e, 1)
    assert r == 0 and not got.counts.any() and not got.offsets.any() and not got.total.any()
    assert np.all(got.words == pc.POISON_W)
    # a count that wrapped past 2^31 is kept modulo 2^32 (row_fill): a full row; and one that wrapped to a small value
    t.image[1, 0], t.image[1, 1] = np.int32(-5), np.int32(2)
    r, got = rc_.pack_host(t, 1)
    assert r == 0 and got.differs(rc_.pack_ref(t, 1)) == []
    assert got.counts[0] == -5 and got.offsets[1] == t.K and got.offsets[2] == t.K + 2


def test_clear_and_reuse():
    """Exactly the first m_c heights and dt of the slot's rows become 0x7FC00000 and its image row 0;
    poison elsewhere, the words, the stamps and the other slots stay; the slot then takes a later
    second whose packed rows are exact."""
    st = STREAM
    t = _filled_tables()
    m = np.minimum(t.image[1], t.K)
    hb, db = t.height.view(np.uint32), t.dt.view(np.uint32)
    for c in range(t.C):                                   # poison behind every row's photons
        hb[1, c, m[c]:], db[1, c, m[c]:] = rc_.POISON_F, rc_.POISON_F
    before = {k: getattr(t, k).copy() for k in ('image', 'words', 'stamps', 'height', 'dt')}
    assert rc_.clear_host(t, 1 + 3) == 0                   # second 4 shares slot 1
    for c in range(t.C):
        assert np.all(hb[1, c, :m[c]] == rc_.NAN_BITS) and np.all(db[1, c, :m[c]] == rc_.NAN_BITS)
        assert np.all(hb[1, c, m[c]:] == rc_.POISON_F) and np.all(db[1, c, m[c]:] == rc_.POISON_F)
    assert not t.image[1].any() and m.sum() > 10
    assert np.array_equal(t.words, before['words']) and np.array_equal(t.stamps, before['stamps'])
    for s in (0, 2):
        assert np.array_equal(t.image[s], before['image'][s])
        assert np.array_equal(hb[s], before['height'][s].view(np.uint32)) and np.array_equal(db[s], before['dt'][s].view(np.uint32))
    # without a dt table only the heights are cleared
    u = _filled_tables()
    dt0 = u.dt.copy()
    assert rc_.clear_host(u, 0, dt=False) == 0 and np.array_equal(u.dt.view(np.uint32), dt0.view(np.uint32))
    assert np.all(u.height.view(np.uint32)[0] == rc_.NAN_BITS)
    # reuse: slot 1, cleared above, takes second 4 (with the stale words and stamps of second 1 behind it)
    hb[1], db[1] = rc_.NAN_BITS, rc_.NAN_BITS
    ev = oc.device_order(st['ev'], 0)
    win = (2, 3, 6)
    assert rc_.list_ring_host(ev, 0, st['N'], st['fs'], st['C'], win, t.K, pc.WIDE, t)[0] == 0
    h, dt = rc_.call_heights(st, ev, 0, 1 << 20)
    assert rc_.fill_ring_host(ev, h, dt, 0, 1 << 20, st['N'], st['fs'], st['C'], win, t) == 0
    _, ref = pc.list_host(ev, 0, st['N'], st['fs'], st['C'], 6, t.K, pc.WIDE)
    assert pc.fill_host(ev, h, dt, 0, 1 << 20, st['N'], st['fs'], st['C'], ref) == 0
    assert rc_.pack_host(t, 4)[1].differs(rc_.pack_ref(ref, 4)) == [] and ref.image[4].sum() > 10


def test_argument_errors():
    """Every MKID_E_ARG case of the four twins, with the outputs left as they were."""
    lib = _lib.load()
    p = oc._p
    ev = oc.pack([1, 2], [10, 20])
    h = np.ones(2, np.float32)
    t, ref = rc_.RingTables(2, C, 4), rc_.RingTables(2, C, 4)
    out = rc_.Packed(C, 8)

    def lst(**kw):
        a = dict(ev=ev, n=2, j0=0, N=N, fs=1e6, C=C, sec0=0, R=2, end=5, K=4, layout=pc.WIDE, image=t.image, out=t.outside,
                 words=t.words, stamps=t.stamps, dropped=t.dropped)
        a.update(kw)
        return lib.mkid_list_photons_ring_host(p(a['ev']), a['n'], a['j0'], a['N'], float(a['fs']), a['C'], a['sec0'],
                                               a['R'], a['end'], a['K'], a['layout'], p(a['image']), p(a['out']),
                                               p(a['words']), p(a['stamps']), p(a['dropped']))

    def fill(**kw):
        a = dict(ev=ev, h=h, dt=h, n=2, j0=0, jd=0, N=N, fs=1e6, C=C, sec0=0, R=2, end=5, K=4, image=t.image,
                 stamps=t.stamps, height=t.height, rdt=t.dt, fill=t.fill)
        a.update(kw)
        return lib.mkid_fill_photon_heights_ring_host(p(a['ev']), p(a['h']), p(a['dt']), a['n'], a['j0'], a['jd'], a['N'],
                                                      float(a['fs']), a['C'], a['sec0'], a['R'], a['end'], a['K'],
                                                      p(a['image']), p(a['stamps']), p(a['height']), p(a['rdt']),
                                                      p(a['fill']))

    def pack(**kw):
        a = dict(sec=0, R=2, K=4, C=C, image=t.image, words=t.words, stamps=t.stamps, height=t.height, rdt=t.dt, cap=8,
                 counts=out.counts, offsets=out.offsets, ow=out.words, os=out.stamps, oh=out.height, odt=out.dt,
                 total=out.total)
        a.update(kw)
        return lib.mkid_pack_second_host(a['sec'], a['R'], a['K'], a['C'], p(a['image']), p(a['words']), p(a['stamps']),
                                         p(a['height']), p(a['rdt']), a['cap'], p(a['counts']), p(a['offsets']),
                                         p(a['ow']), p(a['os']), p(a['oh']), p(a['odt']), p(a['total']))

    def clear(**kw):
        a = dict(sec=0, R=2, K=4, C=C, image=t.image, height=t.height, rdt=t.dt)
        a.update(kw)
        return lib.mkid_clear_second_host(a['sec'], a['R'], a['K'], a['C'], p(a['image']), p(a['height']), p(a['rdt']))

    window = (dict(R=0), dict(R=(1 << 20) + 1), dict(sec0=-1), dict(sec0=6), dict(end=-1, sec0=0),
              dict(end=(1 << 63) // 10 ** 6), dict(end=(1 << 63) - 1))
    common = (dict(ev=None), dict(image=None), dict(stamps=None), dict(n=-1), dict(j0=-1), dict(j0=1 << 62), dict(K=0),
              dict(K=65537), dict(fs=1e6 + 0.5), dict(fs=0), dict(fs=2.0 ** 43 + 1), dict(C=0), dict(C=4097), dict(N=0))
    for kw in window + common + (dict(out=None), dict(words=None), dict(dropped=None), dict(layout=2), dict(layout=-1),
                                 dict(layout=pc.REFERENCE, C=255)):
        assert lst(**kw) == _lib.MKID_E_ARG, kw
    for kw in window + common + (dict(h=None), dict(height=None), dict(fill=None)):
        assert fill(**kw) == _lib.MKID_E_ARG, kw
    slot = (dict(sec=-1), dict(R=0), dict(R=(1 << 20) + 1), dict(K=0), dict(K=65537), dict(C=0), dict(C=4097),
            dict(image=None), dict(height=None))
    for kw in slot + (dict(words=None), dict(counts=None), dict(offsets=None), dict(total=None), dict(cap=-1), dict(ow=None),
                      dict(oh=None), dict(stamps=None), dict(rdt=None)):
        assert pack(**kw) == _lib.MKID_E_ARG, kw
    for kw in slot:
        assert clear(**kw) == _lib.MKID_E_ARG, kw
    assert t.same(ref) == [] and t.same_heights(ref) == [] and out.differs(rc_.Packed(C, 8)) == []
    # the valid edges: an empty list without pointers, a window at the exposure's end, the largest
    # exposure of the clock, optional tables and outputs left out
    assert lst(n=0, ev=None) == 0 and fill(n=0, ev=None, h=None, dt=None) == 0
    assert lst(sec0=5, n=0) == 0 and lst(end=(1 << 63) // 10 ** 6 - 2, n=0) == 0 and lst(R=1 << 20, n=0) == 0
    assert fill(dt=None, rdt=None, n=0) == 0
    assert t.same(ref) == [] and t.same_heights(ref) == []
    assert pack(os=None, stamps=None) == 0 and pack(odt=None, rdt=None) == 0 and pack(odt=None) == 0
    assert pack(cap=0, ow=None, os=None, oh=None, odt=None) == 0 and clear(rdt=None) == 0 and pack(sec=1 << 40) == 0
