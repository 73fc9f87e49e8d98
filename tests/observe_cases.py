"""Shared by tests/test_observe_host.py and tests/test_gpu_observe.py: a packet builder, the numpy
restatement of the count image and the spectra (np.add.at with packets.Timebase.second; the column
rule in np.float32 arithmetic), ctypes wrappers of the host twins, and the case table. Every
comparison made with these is exact integer or list equality.
"""
import ctypes

import numpy as np

from mkids_sdr_amd import _lib, codecs, packets

TS_MASK = codecs.PKT_TS_MASK
FS = 1000000            # with N = 128: 7812.5 rows per second, second boundaries fall between rows
J0S = [0, 1000, (1 << 28) - 7, 3 << 28]
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e38, -1e38], np.float32)


def pack(ch, jg, rng=None):
    """Wide packets of channels ch stamped at global rows jg (28-bit stamps); with rng, random peak
    and baseline fields, which nothing here may depend on."""
    ch, jg = np.asarray(ch, np.uint64), np.asarray(jg, np.int64)
    w = (ch << np.uint64(52)) | (jg & TS_MASK).astype(np.uint64)
    if rng is not None:
        w |= rng.integers(0, 1 << 24, size=w.shape).astype(np.uint64) << np.uint64(28)
    return w


def decode(ev, j0):
    """(ch, jg) as pkt::decode: base = max(j0 - 2^27, 0), jg = base + ((ts - base) mod 2^28)."""
    ev = np.asarray(ev, np.uint64)
    ch = ((ev >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.int64)
    ts = (ev & np.uint64(TS_MASK)).astype(np.int64)
    base = max(int(j0) - (1 << 27), 0)
    return ch, base + ((ts - base) % (1 << 28))


def device_order(ev, j0):
    ch, jg = decode(ev, j0)
    return ev[np.lexsort((jg, ch))]


# ---- numpy restatement ---------------------------------------------------------------------------
def count_ref(ev, j0, N, fs, C, n_seconds, image=None, outside=None):
    image = np.zeros((n_seconds, C), np.int32) if image is None else image
    outside = np.zeros(2, np.int64) if outside is None else outside
    ch, jg = decode(ev, j0)
    sec = packets.Timebase(fs, N).second(jg)
    pix = ch < C
    late = pix & (sec >= n_seconds)
    ok = pix & ~late
    np.add.at(image, (sec[ok], ch[ok]), 1)
    outside += np.array([(~pix).sum(), late.sum()], np.int64)
    return image, outside


def column_ref(h, lo, inv, nbins):
    """Columns of heights h with per-packet lo and inv, all float32: t = h - lo and u = t inv are
    numpy float32 operations, one rounding each."""
    h, lo, inv = (np.asarray(a, np.float32) for a in (h, lo, inv))
    with np.errstate(all='ignore'):
        u = (h - lo) * inv
        assert u.dtype == np.float32
        col = np.full(h.shape, nbins + 2, np.int64)
        good = np.isfinite(h) & ~np.isnan(u)
        under, over = good & (u < 0), good & (u >= np.float32(nbins))
        mid = good & ~under & ~over
        col[under] = 0
        col[over] = nbins + 1
        col[mid] = 1 + u[mid].astype(np.int64)
    return col


def spectra_ref(ev, h, j0, j_defer, C, lo, inv, nbins, defer=False, cap_def=0, spectra=None):
    """-> (spectra [C][nbins + 3] int32, deferred uint64, ndef int64 [2] of this call)."""
    spectra = np.zeros((C, nbins + 3), np.int32) if spectra is None else spectra
    h = np.asarray(h, np.float32)
    ch, jg = decode(ev, j0)
    pix = ch < C
    q = pix & ~np.isfinite(h) & (jg >= j_defer) if defer else np.zeros(len(ev), bool)
    b = pix & ~q
    np.add.at(spectra, (ch[b], column_ref(h[b], lo[ch[b]], inv[ch[b]], nbins)), 1)
    return spectra, np.asarray(ev, np.uint64)[q][:cap_def], np.array([q.sum(), min(q.sum(), cap_def)], np.int64)


# ---- the host twins -----------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def count_host(ev, j0, N, fs, C, n_seconds, image=None, outside=None, n=None):
    """mkid_count_photons_host -> (rc, image, outside); adds to image / outside when given."""
    L = _lib.load()
    ev = None if ev is None else np.ascontiguousarray(ev, np.uint64)
    image = np.zeros((max(n_seconds, 1), max(C, 1)), np.int32) if image is None else image
    outside = np.zeros(2, np.int64) if outside is None else outside
    n = (0 if ev is None else len(ev)) if n is None else n
    rc = L.mkid_count_photons_host(_p(ev), n, j0, N, float(fs), C, n_seconds, _p(image), _p(outside))
    return rc, image, outside


def spectra_host(ev, h, j0, j_defer, C, lo, inv, nbins, defer=False, cap_def=0, spectra=None, n=None):
    """mkid_height_spectra_host -> (rc, spectra, deferred, ndef); adds to spectra when given."""
    L = _lib.load()
    ev = None if ev is None else np.ascontiguousarray(ev, np.uint64)
    h = None if h is None else np.ascontiguousarray(h, np.float32)
    spectra = np.zeros((C, nbins + 3), np.int32) if spectra is None else spectra
    d = np.zeros(max(cap_def, 1), np.uint64) if defer else None
    ndef = np.zeros(2, np.int64) if defer else None
    n = (0 if ev is None else len(ev)) if n is None else n
    rc = L.mkid_height_spectra_host(_p(ev), _p(h), n, j0, j_defer, C, _p(lo), _p(inv), nbins, _p(spectra), _p(d),
                                    cap_def, _p(ndef))
    if not defer:
        return rc, spectra, np.zeros(0, np.uint64), np.zeros(2, np.int64)
    return rc, spectra, d[:int(ndef[1])], ndef


# ---- cases --------------------------------------------------------------------------------------
def bins(C, nbins, rng, odd=True):
    """Per-channel lo and inv that differ; with `odd`, one channel has inv = inf and one inv = NaN."""
    lo = rng.uniform(-3, 0, C).astype(np.float32)
    step = rng.uniform(0.5, 2.0, C).astype(np.float32) * np.float32(8.0 / nbins)
    inv = np.float32(1) / step
    if odd and C >= 4:
        inv[1], inv[2] = np.inf, np.nan
    return lo, inv


def heights_for(n, rng):
    """Normal heights around the bins with every special value sprinkled in."""
    h = rng.normal(1.0, 3.0, n).astype(np.float32)
    k = rng.random(n) < 0.15
    h[k] = rng.choice(SPECIALS, int(k.sum()))
    return h


def case(name, C, N, j0, n_seconds, ev, rng, nbins=256, fs=FS):
    lo, inv = bins(C, nbins, rng)
    return dict(name=name, C=C, N=N, fs=fs, j0=j0, n_seconds=n_seconds, ev=np.ascontiguousarray(ev, np.uint64),
                h=heights_for(len(ev), rng), nbins=nbins, lo=lo, inv=inv)


def cases(C, N, seed=1):
    """The case table for a C-channel context with transform length N; the lists are in the
    device's order unless the name says otherwise."""
    rng = np.random.default_rng(seed)
    tb = packets.Timebase(FS, N)
    out = []
    # second boundaries: every row next to the first rows of seconds 1 .. 3, on every channel parity
    edge = np.concatenate([tb.first_row(s) + np.arange(-3, 3) for s in (1, 2, 3)])
    assert tb.second(tb.first_row(1) - 1) == 0 and tb.second(tb.first_row(1)) == 1
    jg = np.concatenate([edge, rng.integers(0, tb.first_row(3), 300)])
    ch = rng.integers(0, C, jg.size)
    out.append(case('timebase', C, N, 0, 3, device_order(pack(ch, jg, rng), 0), rng))
    # one channel, runs far longer than a workgroup
    jg = np.sort(rng.integers(0, tb.first_row(3), 5000))
    out.append(case('one_channel_long_runs', C, N, 0, 3, pack(np.full(jg.size, C // 3), jg, rng), rng))
    # a channel change at every packet
    out.append(case('channel_change_every_packet', C, N, 0, 2,
                    pack(np.arange(C), rng.integers(0, tb.first_row(2), C), rng), rng))
    # any order: a shuffled list (its sorted twin is made by the test)
    jg = rng.integers(0, tb.first_row(4), 1500)
    out.append(case('shuffled', C, N, 0, 4, rng.permutation(pack(rng.integers(0, C, 1500), jg, rng)), rng))
    # outside: channels >= C and seconds >= n_seconds, in runs and alone
    jg = rng.integers(0, tb.first_row(5), 1200)
    ch = np.where(rng.random(1200) < 0.3, rng.integers(C, 4096, 1200), rng.integers(0, C, 1200))
    out.append(case('outside', C, N, 0, 2, device_order(pack(ch, jg, rng), 0), rng))
    # stamps wrapped around j0. Past 2^20 rows the seconds of a 10^6 S/s clock leave a small image, and
    # the sample clock is free in the rule: there fs = N 2^27, 2^27 rows per second, so that
    # j0 = 2^28 - 7 lies just before a second boundary and the stamps cross it and the 28-bit wrap
    for j0 in J0S:
        fs = FS if j0 < (1 << 20) else N << 27
        t = packets.Timebase(fs, N)
        first = -1 if j0 else 0
        jg = j0 + np.concatenate([np.arange(first, 12), rng.integers(first, t.first_row(2) if fs == FS else 1 << 27, 600)])
        out.append(case('wrap_j0_%d' % j0, C, N, j0, int(t.second(j0)) + 2,
                        device_order(pack(rng.integers(0, C, jg.size), jg, rng), j0), rng, fs=fs))
    return out


def column_case(C, nbins, seed=3):
    """Heights at the rule's edges for every channel's own lo / inv: exactly lo, the first value the
    rule puts in each of the first bins' successor (found with np.nextafter from below), the last
    bin's upper edge and its neighbours, the special values, and random ones."""
    rng = np.random.default_rng(seed)
    lo, inv = bins(C, nbins, rng)
    hs, chs = [], []
    for c in range(min(C, 8)):
        cand = [lo[c], np.nextafter(lo[c], np.float32(-np.inf)), np.nextafter(lo[c], np.float32(np.inf))]
        if np.isfinite(inv[c]):
            step = np.float32(1) / inv[c]
            for b in sorted({1, 2, nbins // 2, nbins - 1, nbins} - {0}):
                x = np.float32(lo[c] + np.float32(b) * step)       # near the lower edge of bin b
                for _ in range(4):
                    x = np.nextafter(x, np.float32(-np.inf))
                # walk up to the first value that the rule puts in a higher column
                col0 = column_ref([x], [lo[c]], [inv[c]], nbins)[0]
                for _ in range(64):
                    y = np.nextafter(x, np.float32(np.inf))
                    if column_ref([y], [lo[c]], [inv[c]], nbins)[0] != col0:
                        cand += [x, y]
                        break
                    x = y
        cand += list(SPECIALS)
        hs += cand
        chs += [c] * len(cand)
    hs += list(heights_for(400, rng))
    chs += list(rng.integers(0, C, 400))
    h = np.array(hs, np.float32)
    ev = pack(np.array(chs), rng.integers(0, 1000, h.size), rng)
    return dict(name='columns_%d' % nbins, C=C, N=0, fs=FS, j0=0, n_seconds=1, ev=ev, h=h, nbins=nbins, lo=lo, inv=inv)


def deferred_case(C, N, seed=4, n=900):
    """Stamps on both sides of j_defer, non-finite heights on both sides of it, channels >= C among
    them; the list is in the device's order, so the deferred packets are scattered through it."""
    rng = np.random.default_rng(seed)
    j0, rows = 5000, 2000
    jd = j0 + rows - 80
    jg = j0 + rng.integers(0, rows, n)
    ch = np.where(rng.random(n) < 0.1, rng.integers(C, 4096, n), rng.integers(0, C, n))
    ev = device_order(pack(ch, jg, rng), j0)
    c = case('deferred', C, N, j0, 2, ev, rng)
    _, jgs = decode(ev, j0)
    late = jgs >= jd
    c['h'][late & (rng.random(n) < 0.7)] = np.nan      # most of the tail waits
    c['h'][~late & (rng.random(n) < 0.05)] = np.nan    # early windows: no height, not deferred
    c['j_defer'] = jd
    return c
