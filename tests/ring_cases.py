"""Shared by tests/test_ring_host.py and tests/test_gpu_ring.py: the ring of second slots and the packed
second. ctypes wrappers of the four host twins (mkid_list_photons_ring_host,
mkid_fill_photon_heights_ring_host, mkid_pack_second_host, mkid_clear_second_host), the numpy
restatement of the window's four `outside` kinds and of a packed second, a multi-second stream cut
into calls with heights that follow the deferral protocol, and the streamed step with drains run on
the host twins. Every comparison made with these is exact.
"""
import numpy as np

import observe_cases as oc
import photon_cases as pc
from mkids_sdr_amd import _lib, observe, packets

_p = oc._p
NAN_BITS = 0x7FC00000               # the NaN the height tables are pre-filled with, and cleared to
POISON_F = 0x7FC0BEEF               # packed heights / dt that must not be written
IN, NONPIXEL, LATE, EARLY, OVERRUN = 0, 1, 2, 3, 4      # ring_kind; outside[kind - 1]


class RingTables(pc.Tables):
    """photon_cases.Tables of n_slots slots, with the ring forms' outside int64 [4]."""

    def __init__(self, n_slots, C, K):
        super().__init__(n_slots, C, K)
        self.outside = np.zeros(4, np.int64)


def _u64(ev):
    return None if ev is None else np.ascontiguousarray(ev, np.uint64)


def list_ring_host(ev, j0, N, fs, C, win, K, layout, t=None, n=None):
    """mkid_list_photons_ring_host with the window win = (sec0, n_slots, sec_end) -> (rc, t)."""
    sec0, R, sec_end = win
    t = RingTables(R, C, K) if t is None else t
    ev = _u64(ev)
    n = (0 if ev is None else len(ev)) if n is None else n
    rc = _lib.load().mkid_list_photons_ring_host(_p(ev), n, j0, N, float(fs), C, sec0, R, sec_end, K, layout,
                                                 _p(t.image), _p(t.outside), _p(t.words), _p(t.stamps), _p(t.dropped))
    return rc, t


def fill_ring_host(ev, h, dt, j0, j_defer, N, fs, C, win, t, n=None):
    """mkid_fill_photon_heights_ring_host into t.height, t.dt (dt None: no dt table) and t.fill."""
    sec0, R, sec_end = win
    ev = _u64(ev)
    h = None if h is None else np.ascontiguousarray(h, np.float32)
    dt = None if dt is None else np.ascontiguousarray(dt, np.float32)
    n = (0 if ev is None else len(ev)) if n is None else n
    return _lib.load().mkid_fill_photon_heights_ring_host(_p(ev), _p(h), _p(dt), n, j0, j_defer, N, float(fs), C, sec0,
                                                          R, sec_end, t.K, _p(t.image), _p(t.stamps), _p(t.height),
                                                          None if dt is None else _p(t.dt), _p(t.fill))


class Packed:
    """The outputs of mkid_pack_second: buffers of exactly `size` entries (cap_out unless given),
    poisoned, so that an entry that must not be written keeps its pattern."""
    NAMES = ('counts', 'offsets', 'words', 'stamps', 'height', 'dt', 'total')

    def __init__(self, C, size):
        self.counts = np.full(C, -77, np.int32)
        self.offsets = np.full(C + 1, -77, np.int64)
        self.words = np.full(size, pc.POISON_W, np.uint64)
        self.stamps = np.full(size, pc.POISON_S, np.int64)
        self.height = np.full(size, POISON_F, np.uint32).view(np.float32)
        self.dt = np.full(size, POISON_F, np.uint32).view(np.float32)
        self.total = np.full(2, -77, np.int64)

    def bits(self, k):
        a = getattr(self, k)
        return a.view(np.uint32) if a.dtype == np.float32 else a

    def differs(self, other, names=NAMES):
        return [k for k in names if not np.array_equal(self.bits(k), other.bits(k))]


def pack_host(t, sec, cap_out=None, size=None, stamps=True, dt=True):
    """mkid_pack_second_host of slot sec mod n_slots of Tables t -> (rc, Packed)."""
    cap_out = t.C * t.K if cap_out is None else cap_out
    out = Packed(t.C, max(cap_out, 0) if size is None else size)
    rc = _lib.load().mkid_pack_second_host(sec, t.n_seconds, t.K, t.C, _p(t.image), _p(t.words), _p(t.stamps),
                                           _p(t.height), _p(t.dt) if dt else None, cap_out, _p(out.counts),
                                           _p(out.offsets), _p(out.words), _p(out.stamps) if stamps else None,
                                           _p(out.height), _p(out.dt) if dt else None, _p(out.total))
    return rc, out


def clear_host(t, sec, dt=True):
    return _lib.load().mkid_clear_second_host(sec, t.n_seconds, t.K, t.C, _p(t.image), _p(t.height),
                                              _p(t.dt) if dt else None)


# ---- numpy restatement ---------------------------------------------------------------------------
def ring_kind(ev, j0, N, fs, C, win):
    """-> (kind of every packet, its second, its channel): IN the window, or which `outside` counter."""
    sec0, R, sec_end = win
    ch, jg = oc.decode(ev, j0)
    sec = packets.Timebase(fs, N).second(jg)
    kind = np.full(len(ch), IN, np.int64)
    kind[sec >= sec0 + R] = OVERRUN
    kind[sec < sec0] = EARLY
    kind[sec >= sec_end] = LATE
    kind[ch >= C] = NONPIXEL
    return kind, sec, ch


def outside_ref(kind):
    return np.bincount(kind, minlength=5)[1:].astype(np.int64)


def pack_ref(t, sec, cap_out=None, size=None, stamps=True, dt=True):
    """The packed second of slot sec mod n_slots of Tables t, by numpy slicing -> Packed."""
    s = sec % t.n_seconds
    cap_out = t.C * t.K if cap_out is None else cap_out
    out = Packed(t.C, cap_out if size is None else size)
    m = np.minimum(t.image[s].view(np.uint32).astype(np.int64), t.K)
    out.counts[:] = t.image[s]
    out.offsets[:] = np.concatenate([[0], np.cumsum(m)])
    cat = lambda a: np.concatenate([a[s, c, :m[c]] for c in range(t.C)])[:cap_out]
    tot = int(m.sum())
    w = min(tot, cap_out)
    out.words[:w] = cat(t.words)
    if stamps:
        out.stamps[:w] = cat(t.stamps)
    out.height.view(np.uint32)[:w] = cat(t.height.view(np.uint32))
    if dt:
        out.dt.view(np.uint32)[:w] = cat(t.dt.view(np.uint32))
    out.total[:] = tot, w
    return out


# ---- a multi-second stream and the streamed step on the host --------------------------------------
ROWS_PER_SEC, SECONDS = 50, 6


def stream(C=8, N=16, seed=81, n=500):
    """Six seconds of 50 rows: unique (ch, stamp) packets in stamps 0 .. 298 (a stream of 300 rows
    stamps nothing later), channel 2 firing at every row of second 1 (its row overflows K = 1 and 3),
    channels >= C among them; every packet's height and dt once its window is complete, NaNs with a
    payload, infinities and zeros among them."""
    rng = np.random.default_rng(seed)
    rows = ROWS_PER_SEC * SECONDS
    ch = np.concatenate([rng.integers(0, C + 2, n), np.full(ROWS_PER_SEC, 2)])
    jg = np.concatenate([rng.integers(0, rows - 1, n), ROWS_PER_SEC + np.arange(ROWS_PER_SEC)])
    ev = np.sort(pc.unique_packets(ch, jg, rng))
    h = oc.heights_for(len(ev), rng)
    h[::11] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    dt = rng.normal(size=len(ev)).astype(np.float32)
    dt[::13] = np.nan
    return dict(C=C, N=N, fs=N * ROWS_PER_SEC, rows=rows, ev=ev, h=h, dt=dt, ncoeff=9, pre=2)


def cut_calls(rows, rng, longest=80):
    """Random contiguous calls (j0, rows) over 0 .. rows - 1, one-row calls included."""
    out, j0 = [], 0
    while j0 < rows:
        r = 1 if len(out) == 1 or rng.random() < 0.3 else int(rng.integers(1, longest + 1))
        r = min(r, rows - j0)
        out.append((j0, r))
        j0 += r
    return out


def call_packets(st, j0, rows):
    """The packets the call over rows j0 .. j0 + rows - 1 produces: stamps j0 - 1 .. j0 + rows - 2, in
    the device's order."""
    jg = oc.decode(st['ev'], 0)[1]
    return oc.device_order(st['ev'][(jg >= j0 - 1) & (jg < j0 + rows - 1)], j0)


def call_heights(st, joined, j0, jd):
    """Heights and dt of a step's joined list: a packet stamped below jd has its window inside the
    rows so far and gets its height (finite or not), the others NaN."""
    at = np.searchsorted(st['ev'], joined)
    jg = oc.decode(joined, j0)[1]
    done = jg < jd
    return np.where(done, st['h'][at], np.float32(np.nan)), np.where(done, st['dt'][at], np.float32(np.nan))


class HostRing:
    """The four calls of a ring step on the host twins; tests/test_gpu_ring.py has the device's."""

    def __init__(self, st, K, layout):
        self.st, self.K, self.layout = st, K, layout

    def tables(self, R):
        return RingTables(R, self.st['C'], self.K)

    def list(self, ev, j0, win, t):
        st = self.st
        assert list_ring_host(ev, j0, st['N'], st['fs'], st['C'], win, self.K, self.layout, t)[0] == 0

    def fill(self, ev, h, dt, j0, jd, win, t):
        st = self.st
        assert fill_ring_host(ev, h, dt, j0, jd, st['N'], st['fs'], st['C'], win, t) == 0

    def pack(self, t, sec):
        rc, out = pack_host(t, sec)
        assert rc == 0
        return out

    def clear(self, t, sec):
        assert clear_host(t, sec) == 0

    def host(self, t):
        return t


def run_stream(st, calls, K, layout, R=None, sec_end=SECONDS, drain=None, keep=None, ops=None):
    """The streamed step on the host twins over `calls`: list the call's packets, join them behind
    the deferred ones, fill. R None: the unbounded tables through mkid_list_photons_host and
    mkid_fill_photon_heights_host over the packets whose word is in `keep` (all when None) ->
    dict(t=Tables). R: the ring forms with the window moved by drains, drain(k) saying whether to
    drain after call k (and a final drain at the end) -> dict(seconds={sec: Packed}, t, kept=the
    words that found their slot, kinds=the restatement's count of every kind [5], pending); `ops`
    makes the ring's calls (HostRing when None)."""
    C, N, fs = st['C'], st['N'], st['fs']
    tb = packets.Timebase(fs, N)
    ops = HostRing(st, K, layout) if ops is None else ops
    t = pc.Tables(sec_end, C, K) if R is None else ops.tables(R)
    deferred = np.zeros(0, np.uint64)
    sec0, settled, seconds, kept, kinds = 0, 0, {}, [], np.zeros(5, np.int64)

    def take(secs):
        nonlocal sec0
        for s in secs:
            seconds[s] = ops.pack(t, s)
            ops.clear(t, s)
            sec0 = s + 1

    for k, (j0, rows) in enumerate(calls):
        ev = call_packets(st, j0, rows)
        jd = observe.j_defer(j0, rows, st['ncoeff'], st['pre'])
        joined = np.concatenate([deferred, ev])
        h, dt = call_heights(st, joined, j0, jd)
        ch, jg = oc.decode(joined, j0)
        deferred = joined[(ch < C) & ~np.isfinite(h) & (jg >= jd)]
        if R is None:
            sel = np.ones(len(ev), bool) if keep is None else np.isin(ev, keep)
            selj = np.ones(len(joined), bool) if keep is None else np.isin(joined, keep)
            assert pc.list_host(ev[sel], j0, N, fs, C, sec_end, K, layout, t)[0] == 0
            assert pc.fill_host(joined[selj], h[selj], dt[selj], j0, jd, N, fs, C, t) == 0
            continue
        win = (sec0, R, sec_end)
        kind = ring_kind(ev, j0, N, fs, C, win)[0]
        kinds += np.bincount(kind, minlength=5)
        kept.append(ev[kind == IN])
        ops.list(ev, j0, win, t)
        ops.fill(joined, h, dt, j0, jd, win, t)
        settled = max(settled, observe.settled_bound(j0, rows, jd))
        if drain(k):
            take(observe.ready_seconds(tb, sec0, R, sec_end, settled))
    if R is None:
        return dict(t=t)
    last = int(tb.second(calls[-1][0] + calls[-1][1] - 1))
    while True:
        secs = observe.ready_seconds(tb, sec0, R, sec_end, settled, last)
        if not secs:
            break
        take(secs)
    return dict(seconds=seconds, t=ops.host(t), kept=np.concatenate(kept), kinds=kinds, pending=deferred)
