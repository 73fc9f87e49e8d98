"""Shared by tests/test_photon_rows_host.py and tests/test_gpu_photon_rows.py: the numpy restatement
of the photon rows (a dictionary of lists per cell, packets.Timebase.microsecond,
packets.encode_wire), ctypes wrappers of the host twins mkid_list_photons_host and
mkid_fill_photon_heights_host, the tables they write into, and the case table. Every comparison made
with these is exact.
"""
import numpy as np

import observe_cases as oc
from mkids_sdr_amd import _lib, codecs, packets

WIDE, REFERENCE = _lib.ROW_WIDE, _lib.ROW_REFERENCE
LAYOUTS = [WIDE, REFERENCE]
POISON_W, POISON_S = np.uint64(0x5A5A5A5A5A5A5A5A), np.int64(-0x123456789)


class Tables:
    """The caller-owned outputs: image [n_seconds][C] int32, outside int64 [2], words uint64 and
    stamps int64 [n_seconds][C][K] (poisoned: a slot that is never written keeps the pattern),
    dropped int64 [1]; height and dt float32 [n_seconds][C][K] pre-filled with NaN, fill int64 [2]."""

    def __init__(self, n_seconds, C, K):
        self.n_seconds, self.C, self.K = n_seconds, C, K
        self.image = np.zeros((n_seconds, C), np.int32)
        self.outside = np.zeros(2, np.int64)
        self.words = np.full((n_seconds, C, K), POISON_W, np.uint64)
        self.stamps = np.full((n_seconds, C, K), POISON_S, np.int64)
        self.dropped = np.zeros(1, np.int64)
        self.height = np.full((n_seconds, C, K), np.nan, np.float32)
        self.dt = np.full((n_seconds, C, K), np.nan, np.float32)
        self.fill = np.zeros(2, np.int64)

    NAMES = ('image', 'outside', 'words', 'stamps', 'dropped')

    def same(self, other, names=NAMES):
        return [k for k in names if not np.array_equal(getattr(self, k), getattr(other, k))]

    def same_heights(self, other):
        """Bit equality of the finite heights and dt, NaN where the other is NaN."""
        bad = []
        for k in ('height', 'dt'):
            a, b = getattr(self, k), getattr(other, k)
            fin = np.isfinite(a) | np.isinf(a)
            if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32))):
                bad.append(k)
        return bad + ([] if np.array_equal(self.fill, other.fill) else ['fill'])

    def pairs(self, sec, ch):
        m = min(int(self.image[sec, ch]), self.K)
        return sorted(zip(self.stamps[sec, ch, :m].tolist(), self.words[sec, ch, :m].tolist()))


# ---- numpy restatement ---------------------------------------------------------------------------
def rows_ref(ev, j0, N, fs, C, n_seconds, K, layout, cells=None):
    """The packets of one call appended to `cells`: {(sec, ch): [(word, stamp), ...]} in list order,
    every packet of the cell (the table keeps the first K); -> (cells, outside int64 [2])."""
    cells = {} if cells is None else cells
    ev = np.asarray(ev, np.uint64)
    tb = packets.Timebase(fs, N)
    ch, jg = oc.decode(ev, j0)
    sec = tb.second(jg)
    pix = ch < C
    late = pix & (sec >= n_seconds)
    ok = pix & ~late
    f = codecs.unpack_wide(ev[ok])
    words = packets.encode_wire(f['ch'], f['peak'], f['base'], tb.microsecond(jg[ok]), wide=layout == WIDE)
    for s, c, w, j in zip(sec[ok].tolist(), ch[ok].tolist(), words.tolist(), jg[ok].tolist()):
        cells.setdefault((s, c), []).append((w, j))
    return cells, np.array([(~pix).sum(), late.sum()], np.int64)


def tables_ref(cells, outside, n_seconds, C, K):
    t = Tables(n_seconds, C, K)
    t.outside += outside
    for (s, c), lst in cells.items():
        t.image[s, c] = len(lst)
        kept = lst[:K]
        t.words[s, c, :len(kept)] = np.array([w for w, _ in kept], np.uint64)
        t.stamps[s, c, :len(kept)] = np.array([j for _, j in kept], np.int64)
        t.dropped[0] += len(lst) - len(kept)
    return t


# ---- the host twins -----------------------------------------------------------------------------
_p = oc._p


def list_host(ev, j0, N, fs, C, n_seconds, K, layout, t=None, n=None):
    """mkid_list_photons_host into Tables t (a fresh one when None) -> (rc, t)."""
    t = Tables(n_seconds, C, K) if t is None else t
    ev = None if ev is None else np.ascontiguousarray(ev, np.uint64)
    n = (0 if ev is None else len(ev)) if n is None else n
    rc = _lib.load().mkid_list_photons_host(_p(ev), n, j0, N, float(fs), C, n_seconds, K, layout, _p(t.image),
                                            _p(t.outside), _p(t.words), _p(t.stamps), _p(t.dropped))
    return rc, t


def fill_host(ev, h, dt, j0, j_defer, N, fs, C, t, n=None):
    """mkid_fill_photon_heights_host into t.height, t.dt (None with dt None: no dt table) and t.fill."""
    ev = None if ev is None else np.ascontiguousarray(ev, np.uint64)
    h = None if h is None else np.ascontiguousarray(h, np.float32)
    dt = None if dt is None else np.ascontiguousarray(dt, np.float32)
    n = (0 if ev is None else len(ev)) if n is None else n
    return _lib.load().mkid_fill_photon_heights_host(_p(ev), _p(h), _p(dt), n, j0, j_defer, N, float(fs), C,
                                                     t.n_seconds, t.K, _p(t.image), _p(t.stamps), _p(t.height),
                                                     None if dt is None else _p(t.dt), _p(t.fill))


# ---- cases --------------------------------------------------------------------------------------
def unique_packets(ch, jg, rng):
    """Wide packets with random fields, one per distinct (ch, jg): a trigger with a dead time never
    stamps a channel twice in a row, and the fill's search needs distinct stamps in a row."""
    key = np.unique(np.asarray(ch, np.int64) << 40 | np.asarray(jg, np.int64))
    return oc.pack(key >> 40, key & ((1 << 40) - 1), rng)


def cases(C, N, seed=5):
    """observe_cases' table (second boundaries inside a channel's run, long runs, a channel change at
    every packet, ch >= C, sec >= n_seconds, stamps across the 28-bit wrap for j0 = 0, 1000,
    2^28 - 7, 3 2^28) and, for the rows: j0 just below and above 2^27 (where the unwrap's base
    leaves 0) with stamps across the 28-bit wrap, and an empty list. Each with the Ks to run."""
    rng = np.random.default_rng(seed)
    out = [dict(c, Ks=(1, 7, 2000) if c['name'] == 'one_channel_long_runs' else (1, 7)) for c in oc.cases(C, N)]
    fs = N << 27                                   # 2^27 rows per second, as observe_cases' wrap cases
    for j0 in ((1 << 27) - 3, (1 << 27) + 3, (1 << 28) + (1 << 27) - 2):
        lo = max(j0 - (1 << 27), 0)
        jg = np.concatenate([lo + np.arange(0, 6), (1 << 28) + np.arange(-6, 6), j0 + np.arange(-4, 4),
                             j0 + (1 << 27) - 1 - np.arange(0, 6), rng.integers(lo, j0 + (1 << 27), 500)])
        jg = jg[(jg >= lo) & (jg < j0 + (1 << 27))]
        ev = oc.device_order(unique_packets(rng.integers(0, C + 3, jg.size), jg, rng), j0)
        out.append(dict(oc.case('base_j0_%d' % j0, C, N, j0, 3, ev, rng, fs=fs), Ks=(1, 7)))
    out.append(dict(oc.case('empty', C, N, 0, 2, np.zeros(0, np.uint64), rng), Ks=(1, 7)))
    return out
