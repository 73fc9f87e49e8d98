"""The per-pixel, per-second photon rows through the host twins (mkid_list_photons_host,
mkid_fill_photon_heights_host: the loops of csrc/obs_common.h, no device): against the existing host
path WireStream -> PacketMaster, against the numpy restatement of tests/photon_cases.py over the
case table in both layouts, chunk invariance down to one-row calls, the heights of the deferral
protocol filled into the rows, and every MKID_E_ARG case. Every comparison is exact.
"""
import numpy as np
import pytest

import observe_cases as oc
import photon_cases as pc
from mkids_sdr_amd import _lib, observe, packets

C, N = 64, 128


def test_rows_equal_packetmaster():
    """Three calls of device-order lists over two second boundaries through WireStream ->
    (low, high) big-endian blocks -> PacketMaster keeping K events, against the twin's rows in the
    reference layout; a row overflows K and a cell straddles two calls."""
    K, fs, rows = 7, N * 300, 250                       # 300 rows per second, calls of 250 rows
    rng = np.random.default_rng(51)
    ws = packets.WireStream(fs, N)
    pm = packets.PacketMaster(1, C, 2, max_events=K + 1)
    t = pc.Tables(2, C, K)
    per_call = []
    for k in range(3):
        j0 = k * rows
        jg = rng.integers(j0, j0 + rows - 1, 500)       # a call stamps [j0 - 1, j0 + rows - 1)
        ch = rng.integers(0, C, 500)
        if k == 0:                                      # pixel 3 overflows K in second 0
            jg, ch = np.concatenate([jg, np.arange(10, 150, 10)]), np.concatenate([ch, np.full(14, 3)])
        ev = oc.device_order(pc.unique_packets(ch, jg, rng), j0)
        per_call.append(ev)
        rc, _ = pc.list_host(ev, j0, N, fs, C, 2, K, pc.REFERENCE, t)
        assert rc == 0
        w = ws.push(ev, j0, rows)
        pm.receive(0, (w & np.uint64(0xFFFFFFFF)).astype('>u4').tobytes(), (w >> np.uint64(32)).astype('>u4').tobytes())
    assert pm.sec[0] == 2 and t.image[0, 3] > K and t.dropped[0] > 0 and t.outside[1] > 0
    # a cell with packets of two calls: second 1 is rows 300 .. 599, calls 1 and 2 meet at row 500
    sec1 = [packets.Timebase(fs, N).second(oc.decode(ev, k * rows)[1]) == 1 for k, ev in enumerate(per_call)]
    both = set(oc.decode(per_call[1][sec1[1]], 0)[0].tolist()) & set(oc.decode(per_call[2][sec1[2]], 0)[0].tolist())
    assert len(both) > C // 2
    kept = np.minimum(t.image, K)
    assert np.array_equal(pm.photon_counts, kept)
    for sec in range(2):
        for p in range(C):
            assert np.array_equal(pm.rows[(0, p)][sec], t.words[sec, p, :kept[sec, p]]), (sec, p)
    # the table's image is the count image
    image = np.zeros((2, C), np.int32)
    for k, ev in enumerate(per_call):
        oc.count_ref(ev, k * rows, N, fs, C, 2, image)
    assert np.array_equal(t.image, image)


CASES = pc.cases(C, N)


@pytest.mark.parametrize('layout', pc.LAYOUTS)
@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_twin_equals_restatement(c, layout):
    for K in c['Ks']:
        cells, outside = pc.rows_ref(c['ev'], c['j0'], N, c['fs'], C, c['n_seconds'], K, layout)
        ref = pc.tables_ref(cells, outside, c['n_seconds'], C, K)
        rc, t = pc.list_host(c['ev'], c['j0'], N, c['fs'], C, c['n_seconds'], K, layout)
        assert rc == 0 and t.same(ref) == [], (K, t.same(ref))
        _, image, out = oc.count_host(c['ev'], c['j0'], N, c['fs'], C, c['n_seconds'])
        assert np.array_equal(t.image, image) and np.array_equal(t.outside, out)
        assert t.image.sum() + t.outside.sum() == len(c['ev'])
        if c['name'] == 'one_channel_long_runs':               # about 1700 packets a cell
            assert (t.dropped[0] > 0) == (K < 2000)


def test_case_table_covers_the_edges():
    names = {c['name'] for c in CASES}
    assert {'timebase', 'outside', 'empty', 'base_j0_%d' % ((1 << 27) - 3), 'base_j0_%d' % ((1 << 27) + 3)} <= names
    for c in CASES:
        if c['name'].startswith('base_j0'):
            ch, jg = oc.decode(c['ev'], c['j0'])
            assert (ch >= C).any() and jg.min() == max(c['j0'] - (1 << 27), 0) and jg.max() == c['j0'] + (1 << 27) - 1
            if c['j0'] > 1 << 27:                              # the window holds a 28-bit wrap
                assert len(set((jg >> 28).tolist())) == 2
    c = next(c for c in CASES if c['name'] == 'timebase')     # a second boundary inside a channel's run
    ch, jg = oc.decode(c['ev'], 0)
    sec = packets.Timebase(c['fs'], N).second(jg)
    assert ((ch[1:] == ch[:-1]) & (sec[1:] != sec[:-1])).any()


@pytest.mark.parametrize('layout', pc.LAYOUTS)
def test_chunk_invariance(layout):
    """One call over a stream against the same stream in one-row calls (the packets of one phase row,
    every channel that fired in it, with j0 = that row), bit for bit."""
    rng = np.random.default_rng(52)
    fs, K = N * 200, 5
    ev = pc.unique_packets(rng.integers(0, C + 2, 1500), rng.integers(0, 700, 1500), rng)
    rc, one = pc.list_host(oc.device_order(ev, 0), 0, N, fs, C, 3, K, layout)
    assert rc == 0 and one.dropped[0] > 0 and one.outside.min() > 0
    ch, jg = oc.decode(ev, 0)
    t = pc.Tables(3, C, K)
    for row in np.unique(jg):
        part = ev[jg == row]
        assert pc.list_host(part[np.argsort(oc.decode(part, row)[0])], int(row), N, fs, C, 3, K, layout, t)[0] == 0
    assert t.same(one) == []


def _fit_host(phase, ev, coeff, pre, L):
    lib = _lib.load()
    h, dt = np.zeros(len(ev)), np.zeros(len(ev))
    assert lib.mkid_pulse_fit_host(oc._p(phase), len(phase), phase.shape[1], 0, oc._p(np.ascontiguousarray(ev)), len(ev),
                                   oc._p(coeff), coeff.shape[1], pre, L, -1, oc._p(h), oc._p(dt), None, None) == 0
    return h.astype(np.float32), dt.astype(np.float32)


def _protocol(shuffle):
    """The streamed step on the host, four calls: list the call's packets, join them behind the
    deferred ones, mkid_pulse_fit_host over the rows so far, bin (which defers), fill."""
    rng = np.random.default_rng(53)
    Cs, J, calls, ncoeff, pre, L, K, fs = 8, 120, 4, 21, 6, 3, 12, N * 150
    n_seconds = 3                                              # 480 rows: seconds 0 .. 3, the last one late
    phase = rng.normal(size=(J * calls, Cs)).astype(np.float32)
    coeff = rng.normal(size=(Cs, ncoeff)).astype(np.float32)
    lo, inv = np.full(Cs, -50, np.float32), np.full(Cs, 1, np.float32)
    t = pc.Tables(n_seconds, Cs, K)
    deferred, spectra, all_ev = np.zeros(0, np.uint64), np.zeros((Cs, 103), np.int32), []
    order = np.random.default_rng(59)
    for k in range(calls):
        j0 = k * J
        ev = oc.device_order(pc.unique_packets(rng.integers(0, Cs + 1, 150), rng.integers(j0, j0 + J, 150), rng), j0)
        all_ev.append(ev)
        assert pc.list_host(ev, j0, N, fs, Cs, n_seconds, K, pc.WIDE, t)[0] == 0
        joined = np.concatenate([deferred, ev])
        if shuffle:
            joined = order.permutation(joined)
        h, dt = _fit_host(phase[:j0 + J], joined, coeff, pre, L)
        jd = observe.j_defer(j0, J, ncoeff, pre, L)
        rc, _, deferred, ndef = oc.spectra_host(joined, h, j0, jd, Cs, lo, inv, 100, True, 1000, spectra=spectra)
        assert rc == 0 and ndef[0] == ndef[1] and (k == calls - 1 or ndef[0] > 0)
        assert pc.fill_host(joined, h, dt, j0, jd, N, fs, Cs, t) == 0
    h, dt = _fit_host(phase, np.concatenate(all_ev), coeff, pre, L)      # the whole stream at once
    return dict(t=t, pending=deferred, spectra=spectra, ev=np.concatenate(all_ev), h=h, dt=dt, Cs=Cs, K=K, fs=fs,
                n_seconds=n_seconds, early=pre + L)


def test_fill_through_the_deferral_protocol():
    """After the last step every stored photon whose window ever completed holds the height and dt
    the fit gives it over the whole stream, the rest are NaN, and fill[0] + fill[1] + pending is
    every packet with ch < C; a shuffled joined list gives identical tables."""
    r = _protocol(False)
    t, ev, Cs, K = r['t'], r['ev'], r['Cs'], r['K']
    ch, jg = oc.decode(ev, 0)
    sec = packets.Timebase(r['fs'], N).second(jg)
    pending = set(r['pending'].tolist())
    assert np.isnan(r['h'][jg < r['early']]).all() and 0 < len(pending) < np.isnan(r['h'][ch < Cs]).sum()
    want = pc.Tables(r['n_seconds'], Cs, K)
    want.image[:], want.stamps[:] = t.image, t.stamps
    for p in np.flatnonzero(ch < Cs):
        at = np.zeros(0, np.int64)
        if sec[p] < r['n_seconds']:
            at = np.flatnonzero(t.stamps[sec[p], ch[p], :min(t.image[sec[p], ch[p]], K)] == jg[p])
        assert at.size <= 1
        if at.size:                                            # a pending packet's height is NaN in h too
            want.height[sec[p], ch[p], at[0]], want.dt[sec[p], ch[p], at[0]] = r['h'][p], r['dt'][p]
        if int(ev[p]) not in pending:
            want.fill[0 if at.size else 1] += 1
    assert t.same_heights(want) == [], t.same_heights(want)
    assert t.fill.sum() + len(pending) == (ch < Cs).sum() and t.fill.min() > 0 and t.dropped[0] > 0
    assert np.isfinite(t.height).sum() > 100 and r['spectra'].sum() == t.fill.sum()
    s = _protocol(True)['t']
    assert s.same(t) == [] and s.same_heights(t) == []


def test_fill_specials_and_no_dt():
    """Heights NaN (with a payload), +-inf, +-0 are copied bit for bit; a null dt leaves the dt table
    alone; deferred packets and channels >= C touch nothing."""
    rng = np.random.default_rng(54)
    fs, K = N * 100, 4
    ev = oc.device_order(pc.unique_packets(rng.integers(0, C + 5, 800), rng.integers(0, 250, 800), rng), 0)
    _, t = pc.list_host(ev, 0, N, fs, C, 2, K, pc.WIDE)
    h = oc.heights_for(len(ev), rng)
    h[::7] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    dt = rng.normal(size=len(ev)).astype(np.float32)
    jd = 200
    before_dt = t.dt.copy()
    assert pc.fill_host(ev, h, None, 0, jd, N, fs, C, t) == 0
    assert np.array_equal(t.dt.view(np.uint32), before_dt.view(np.uint32))
    t2 = pc.Tables(2, C, K)
    t2.image[:], t2.stamps[:] = t.image, t.stamps
    assert pc.fill_host(ev, h, dt, 0, jd, N, fs, C, t2) == 0
    assert np.array_equal(t.height.view(np.uint32), t2.height.view(np.uint32)) and np.array_equal(t.fill, t2.fill)
    ch, jg = oc.decode(ev, 0)
    sec = packets.Timebase(fs, N).second(jg)
    live = (ch < C) & ~(~np.isfinite(h) & (jg >= jd))
    found = 0
    hb, db = t2.height.view(np.uint32), t2.dt.view(np.uint32)
    nan32 = np.array([np.nan], np.float32).view(np.uint32)[0]
    for p in range(len(ev)):
        if ch[p] >= C or sec[p] >= 2:
            continue
        at = np.flatnonzero(t.stamps[sec[p], ch[p], :min(t.image[sec[p], ch[p]], K)] == jg[p])
        if at.size and live[p]:
            assert hb[sec[p], ch[p], at[0]] == h[p:p + 1].view(np.uint32)[0] and db[sec[p], ch[p], at[0]] == dt[p:p + 1].view(np.uint32)[0]
            found += 1
        elif at.size:
            assert hb[sec[p], ch[p], at[0]] == nan32 and db[sec[p], ch[p], at[0]] == nan32
    assert t.fill[0] == found > 100 and t.fill[1] == live.sum() - found > 0


def test_argument_errors():
    """Every MKID_E_ARG case of the two twins, with the outputs left as they were."""
    lib = _lib.load()
    ev = oc.pack([1, 2], [10, 20])
    h, dt = np.ones(2, np.float32), np.ones(2, np.float32)
    t = pc.Tables(2, C, 4)
    ref = pc.Tables(2, C, 4)
    p = oc._p

    def lst(**kw):
        a = dict(ev=ev, n=2, j0=0, N=N, fs=1e6, C=C, ns=2, K=4, layout=pc.WIDE, image=t.image, out=t.outside,
                 words=t.words, stamps=t.stamps, dropped=t.dropped)
        a.update(kw)
        return lib.mkid_list_photons_host(p(a['ev']), a['n'], a['j0'], a['N'], float(a['fs']), a['C'], a['ns'], a['K'],
                                          a['layout'], p(a['image']), p(a['out']), p(a['words']), p(a['stamps']),
                                          p(a['dropped']))

    def fill(**kw):
        a = dict(ev=ev, h=h, dt=dt, n=2, j0=0, jd=0, N=N, fs=1e6, C=C, ns=2, K=4, image=t.image, stamps=t.stamps,
                 height=t.height, rdt=t.dt, fill=t.fill)
        a.update(kw)
        return lib.mkid_fill_photon_heights_host(p(a['ev']), p(a['h']), p(a['dt']), a['n'], a['j0'], a['jd'], a['N'],
                                                 float(a['fs']), a['C'], a['ns'], a['K'], p(a['image']), p(a['stamps']),
                                                 p(a['height']), p(a['rdt']), p(a['fill']))

    common = (dict(ev=None), dict(image=None), dict(stamps=None), dict(n=-1), dict(j0=-1), dict(j0=1 << 62), dict(ns=0),
              dict(ns=(1 << 20) + 1), dict(K=0), dict(K=65537), dict(fs=1e6 + 0.5), dict(fs=0), dict(fs=2.0 ** 43 + 1),
              dict(C=0), dict(C=4097), dict(N=0))
    for kw in common + (dict(out=None), dict(words=None), dict(dropped=None), dict(layout=2), dict(layout=-1),
                        dict(layout=pc.REFERENCE, C=255)):
        assert lst(**kw) == _lib.MKID_E_ARG, kw
    for kw in common + (dict(h=None), dict(height=None), dict(fill=None)):
        assert fill(**kw) == _lib.MKID_E_ARG, kw
    assert t.same(ref) == [] and t.same_heights(ref) == []
    # the valid edges: an empty list without pointers, the largest clock, C = 254 in the reference layout
    assert lst(n=0, ev=None) == 0 and fill(n=0, ev=None, h=None, dt=None) == 0
    assert t.same(ref) == [] and t.same_heights(ref) == []
    assert lst(fs=2.0 ** 43) == 0 and fill(dt=None, rdt=None) == 0
    big = pc.Tables(1, 254, 1)
    assert pc.list_host(oc.pack([253], [5]), 0, N, 1e6, 254, 1, 1, pc.REFERENCE, big)[0] == 0 and big.image[0, 253] == 1
