"""The count image and the pulse-height spectra through the host twins (mkid_count_photons_host,
mkid_height_spectra_host: the loops of csrc/obs_common.h, no device) against the numpy restatement
of tests/observe_cases.py. All results are integers and every comparison is exact.
"""
import ctypes

import numpy as np
import pytest

import observe_cases as oc
from mkids_sdr_amd import _lib, observe, packets

C, N = 64, 128
CASES = oc.cases(C, N)


def _check_case(c):
    rc, image, outside = oc.count_host(c['ev'], c['j0'], c['N'], c['fs'], c['C'], c['n_seconds'])
    assert rc == 0
    rimage, routside = oc.count_ref(c['ev'], c['j0'], c['N'], c['fs'], c['C'], c['n_seconds'])
    assert np.array_equal(image, rimage) and np.array_equal(outside, routside)
    rc, spectra, _, _ = oc.spectra_host(c['ev'], c['h'], c['j0'], 0, c['C'], c['lo'], c['inv'], c['nbins'])
    assert rc == 0
    rspectra, _, _ = oc.spectra_ref(c['ev'], c['h'], c['j0'], 0, c['C'], c['lo'], c['inv'], c['nbins'])
    assert np.array_equal(spectra, rspectra)
    ch, _ = oc.decode(c['ev'], c['j0'])
    assert image.sum() + outside.sum() == len(c['ev'])
    assert spectra.sum() == (ch < c['C']).sum()
    return image, outside, spectra


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_case_table(c):
    image, outside, spectra = _check_case(c)
    if c['name'] == 'timebase':
        assert image.shape == (3, C) and np.all(image.sum(axis=1) > 0) and outside[1] > 0
    if c['name'] == 'outside':
        assert outside[0] > 100 and outside[1] > 100
    if c['name'].startswith('wrap'):
        assert image.sum() > 0 and np.count_nonzero(image.sum(axis=1)) >= 2   # stamps cross a second


def test_channel_change_every_packet_1024():
    for c in oc.cases(1024, 2048):
        if c['name'] == 'channel_change_every_packet':
            image, _, _ = _check_case(c)
            assert image.sum() == 1024 and image.max() == 1


def test_any_order():
    c = next(c for c in CASES if c['name'] == 'shuffled')
    o = np.lexsort(oc.decode(c['ev'], 0)[::-1])
    assert not np.array_equal(o, np.arange(len(o)))
    a = _check_case(c)
    b = _check_case(dict(c, ev=c['ev'][o], h=c['h'][o]))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_outside_changes_nothing_else():
    c = next(c for c in CASES if c['name'] == 'outside')
    ch, jg = oc.decode(c['ev'], 0)
    sec = packets.Timebase(c['fs'], N).second(jg)
    keep = (ch < C) & (sec < c['n_seconds'])
    image, outside, spectra = _check_case(c)
    image2, outside2, _ = _check_case(dict(c, ev=c['ev'][keep], h=c['h'][keep]))
    assert np.array_equal(image, image2) and not outside2.any()
    assert np.array_equal(outside, [(ch >= C).sum(), ((ch < C) & (sec >= c['n_seconds'])).sum()])
    _, _, spectra3 = _check_case(dict(c, ev=c['ev'][ch < C], h=c['h'][ch < C]))
    assert np.array_equal(spectra, spectra3)


def _cuts(n, rng):
    k = np.sort(rng.integers(0, n + 1, 7))
    return [0] + list(k) + [n]


@pytest.mark.parametrize('name', ['timebase', 'one_channel_long_runs', 'outside', 'wrap_j0_%d' % ((1 << 28) - 7)])
def test_chunking(name):
    """One call over a list equals the list cut into calls at arbitrary points, one-packet calls
    included: image, spectra and outside."""
    c = next(c for c in CASES if c['name'] == name)
    whole = _check_case(c)
    rng = np.random.default_rng(8)
    n = len(c['ev'])
    for cuts in (_cuts(n, rng), list(range(0, 41)) + [n]):
        image = np.zeros_like(whole[0])
        outside = np.zeros(2, np.int64)
        spectra = np.zeros_like(whole[2])
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert oc.count_host(c['ev'][a:b], c['j0'], N, c['fs'], C, c['n_seconds'], image, outside)[0] == 0
            assert oc.spectra_host(c['ev'][a:b], c['h'][a:b], c['j0'], 0, C, c['lo'], c['inv'], c['nbins'],
                                   spectra=spectra)[0] == 0
        assert np.array_equal(image, whole[0]) and np.array_equal(outside, whole[1])
        assert np.array_equal(spectra, whole[2])


@pytest.mark.parametrize('nbins', [1, 2, 256, 16384])
def test_column_rule(nbins):
    c = oc.column_case(C, nbins)
    rc, spectra, _, _ = oc.spectra_host(c['ev'], c['h'], 0, 0, C, c['lo'], c['inv'], nbins)
    assert rc == 0
    ref, _, _ = oc.spectra_ref(c['ev'], c['h'], 0, 0, C, c['lo'], c['inv'], nbins)
    assert np.array_equal(spectra, ref)
    # the rule's fixed points, packet by packet through the twin
    one = lambda h, ch: int(np.flatnonzero(oc.spectra_host(oc.pack([ch], [0]), np.array([h], np.float32), 0, 0, C,
                                                           c['lo'], c['inv'], nbins)[1][ch])[0])
    for ch in (0, 3, 5):
        lo, inv = c['lo'][ch], c['inv'][ch]
        assert one(lo, ch) == 1                                                   # exactly lo: t = +0
        assert one(np.nextafter(lo, np.float32(-np.inf)), ch) == 0                # just under
        for v in (np.inf, -np.inf, np.nan):
            assert one(v, ch) == nbins + 2
        assert one(1e38, ch) == nbins + 1 and one(-1e38, ch) == 0
        # the first value of the next bin, found with nextafter from inside bin 1 upwards
        # (column 2: bin 2, or "over" when there is one bin)
        x = np.float32(lo + np.float32(1) / inv)
        for _ in range(8):
            x = np.nextafter(x, np.float32(-np.inf))
        assert oc.column_ref([x], [lo], [inv], nbins)[0] == 1
        while oc.column_ref([x], [lo], [inv], nbins)[0] == 1:
            prev, x = x, np.nextafter(x, np.float32(np.inf))
        assert one(prev, ch) == 1 and one(x, ch) == 2
        # the last bin's upper edge: u >= nbins is over, the float just below it the last bin
        top = np.float32(lo + np.float32(nbins) / inv)
        for h in (top, np.nextafter(top, np.float32(-np.inf)), np.nextafter(top, np.float32(np.inf))):
            u = np.float32(np.float32(h - lo) * inv)
            assert one(h, ch) == (nbins + 1 if u >= np.float32(nbins) else 1 + int(u))
    # -0.0 with lo = 0 lands in column 1; inv = inf and inv = NaN give defined columns
    z = dict(lo=np.zeros(C, np.float32), inv=np.ones(C, np.float32))
    sp = oc.spectra_host(oc.pack([0], [0]), np.array([-0.0], np.float32), 0, 0, C, z['lo'], z['inv'], nbins)[1]
    assert sp[0, 1] == 1 and sp.sum() == 1
    assert np.isinf(c['inv'][1]) and np.isnan(c['inv'][2])
    assert one(np.float32(c['lo'][1]), 1) == nbins + 2                            # 0 * inf = NaN
    assert one(np.float32(c['lo'][1] + 1), 1) == nbins + 1 and one(np.float32(c['lo'][1] - 1), 1) == 0
    assert one(np.float32(0.5), 2) == nbins + 2


def test_deferred():
    c = oc.deferred_case(C, N)
    ch, jg = oc.decode(c['ev'], c['j0'])
    bad = ~np.isfinite(c['h'])
    assert (bad & (jg < c['j_defer']) & (ch < C)).sum() > 5 and (bad & (jg >= c['j_defer']) & (ch < C)).sum() > 20
    assert (bad & (jg >= c['j_defer']) & (ch >= C)).sum() > 0
    nq = int((bad & (jg >= c['j_defer']) & (ch < C)).sum())
    for cap_def in (nq + 5, nq, nq - 7, 1, 0):
        rc, spectra, deferred, ndef = oc.spectra_host(c['ev'], c['h'], c['j0'], c['j_defer'], C, c['lo'], c['inv'],
                                                      c['nbins'], defer=True, cap_def=cap_def)
        assert rc == 0
        rs, rd, rn = oc.spectra_ref(c['ev'], c['h'], c['j0'], c['j_defer'], C, c['lo'], c['inv'], c['nbins'],
                                    defer=True, cap_def=cap_def)
        assert np.array_equal(spectra, rs) and np.array_equal(deferred, rd) and np.array_equal(ndef, rn)
        assert ndef[0] == nq and ndef[1] == min(nq, cap_def)
        full = c['ev'][bad & (jg >= c['j_defer']) & (ch < C)]                  # stable: list order
        assert np.array_equal(deferred, full[:cap_def])
        assert spectra.sum() + ndef[1] == (ch < C).sum() - (ndef[0] - ndef[1])
    # without a deferred list every packet is binned
    rc, spectra, _, _ = oc.spectra_host(c['ev'], c['h'], c['j0'], c['j_defer'], C, c['lo'], c['inv'], c['nbins'])
    assert spectra.sum() == (ch < C).sum()
    # ndef and the list continue: a second call appends
    L = _lib.load()
    d = np.zeros(2 * nq, np.uint64)
    ndef = np.zeros(2, np.int64)
    sp = np.zeros((C, c['nbins'] + 3), np.int32)
    for _ in range(2):
        assert L.mkid_height_spectra_host(oc._p(c['ev']), oc._p(c['h']), len(c['ev']), c['j0'], c['j_defer'], C,
                                          oc._p(c['lo']), oc._p(c['inv']), c['nbins'], oc._p(sp), oc._p(d), 2 * nq,
                                          oc._p(ndef)) == 0
    assert np.array_equal(ndef, [2 * nq, 2 * nq]) and np.array_equal(d, np.concatenate([full, full]))


def test_cross_check_with_wire_stream():
    """packets.WireStream.push on the same packets, decoded with decode_wire and counted between the
    end-of-second markers, equals the image's first two rows."""
    rng = np.random.default_rng(12)
    tb = packets.Timebase(oc.FS, N)
    rows = tb.first_row(2) + 40
    jg = np.concatenate([rng.integers(0, rows - 1, 3000), tb.first_row(1) + np.arange(-2, 2),
                         tb.first_row(2) + np.arange(-2, 2)])
    ev = oc.device_order(oc.pack(rng.integers(0, C, jg.size), jg, rng), 0)
    words = packets.WireStream(oc.FS, N).push(ev, 0, rows)
    f = packets.decode_wire(words)
    eos = np.flatnonzero(f['ch'] == 255)
    assert len(eos) == 2
    counted = np.zeros((2, C), np.int32)
    start = 0
    for s, e in enumerate(eos):
        np.add.at(counted[s], f['ch'][start:e], 1)
        start = e + 1
    rc, image, _ = oc.count_host(ev, 0, N, oc.FS, C, 3)
    assert rc == 0 and image[2].sum() > 0
    assert np.array_equal(image[:2], counted)


@pytest.mark.parametrize('L', [0, 3])
def test_j_defer_pin(L):
    """Observation's j_defer against mkid_pulse_fit_host on a small phase block: the packet stamped
    j_defer - 1 gets a finite height, the one stamped j_defer NaN."""
    lib = _lib.load()
    rng = np.random.default_rng(13)
    Cs, rows, j0, ncoeff, pre = 4, 60, 1000, 17, 5
    phase = rng.normal(size=(rows, Cs)).astype(np.float32)
    coeff = rng.normal(size=(Cs, ncoeff)).astype(np.float32)
    jd = observe.j_defer(j0, rows, ncoeff, pre, L)
    assert jd == j0 + rows + pre - ncoeff - L + 1
    ev = oc.pack([1, 1, 2, 2], [jd - 1, jd, jd - 1, jd])
    h = np.zeros(4, np.float64)
    assert lib.mkid_pulse_fit_host(oc._p(phase), rows, Cs, j0, oc._p(ev), 4, oc._p(coeff), ncoeff, pre, L, -1,
                                   oc._p(h), None, None, None) == 0
    assert np.array_equal(np.isfinite(h), [True, False, True, False])


def test_host_twin_argument_errors():
    lib = _lib.load()
    ev, h = oc.pack([1, 2], [3, 4]), np.zeros(2, np.float32)
    image, outside = np.zeros((2, C), np.int32), np.zeros(2, np.int64)
    lo, inv, sp = np.zeros(C, np.float32), np.ones(C, np.float32), np.zeros((C, 7), np.int32)
    d, ndef = np.zeros(4, np.uint64), np.zeros(2, np.int64)

    def count(**kw):
        a = dict(ev=ev, n=2, j0=0, N=N, fs=1e6, C=C, ns=2, image=image, outside=outside)
        a.update(kw)
        return lib.mkid_count_photons_host(oc._p(a['ev']), a['n'], a['j0'], a['N'], ctypes.c_double(a['fs']), a['C'],
                                           a['ns'], oc._p(a['image']), oc._p(a['outside']))

    def spec(**kw):
        a = dict(ev=ev, h=h, n=2, j0=0, jd=0, C=C, lo=lo, inv=inv, nbins=4, sp=sp, d=d, cap=4, ndef=ndef)
        a.update(kw)
        return lib.mkid_height_spectra_host(oc._p(a['ev']), oc._p(a['h']), a['n'], a['j0'], a['jd'], a['C'],
                                            oc._p(a['lo']), oc._p(a['inv']), a['nbins'], oc._p(a['sp']), oc._p(a['d']),
                                            a['cap'], oc._p(a['ndef']))

    assert count() == 0 and count(n=0, ev=None) == 0 and count(ns=1 << 20, image=None) == _lib.MKID_E_ARG
    for kw in (dict(image=None), dict(outside=None), dict(ev=None), dict(n=-1), dict(j0=-1), dict(ns=0),
               dict(ns=(1 << 20) + 1), dict(fs=1e6 + 0.5), dict(fs=0.0), dict(fs=-1e6), dict(fs=2.0 ** 53),
               dict(fs=float('nan')), dict(fs=float('inf')), dict(C=0), dict(C=4097), dict(N=0),
               dict(j0=(1 << 62))):
        assert count(**kw) == _lib.MKID_E_ARG, kw
    assert image.sum() == 2 and outside.sum() == 0            # only the one good call counted
    assert spec() == 0 and spec(n=0, ev=None, h=None) == 0 and spec(d=None, ndef=None) == 0
    assert spec(d=None) == 0                                    # ndef alone is ignored
    before = sp.copy()
    for kw in (dict(lo=None), dict(inv=None), dict(sp=None), dict(ev=None), dict(h=None), dict(n=-1), dict(j0=-1),
               dict(cap=-1), dict(nbins=0), dict(nbins=16385), dict(ndef=None), dict(C=0), dict(C=4097)):
        assert spec(**kw) == _lib.MKID_E_ARG, kw
    assert np.array_equal(sp, before) and not ndef.any()
