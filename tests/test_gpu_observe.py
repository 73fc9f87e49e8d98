"""mkid_count_photons, mkid_height_spectra and mkid_concat_packets on the device (k_observe.hip)
against the host twins, which tests/test_observe_host.py holds against the numpy restatement. All
results are integers and every comparison is exact: image, spectra, outside, the deferred list and
both of its counts. Then the kernels' own edges (tiny lists, one workgroup's slice, the grid's
stride, device-side counts, more channels than LDS rows, a row that fits no LDS), the error paths,
and a small streamed run through observe.Observation with no host synchronisation between calls.
"""
import ctypes
import os

import numpy as np
import pytest

import observe_cases as oc
from mkids_sdr_amd import _lib, observe, packets

pytestmark = pytest.mark.gpu
C = 64
SLICE, MAX_BLOCKS = 2048, 1024      # csrc/pkt_common.h kObsSlice, kObsMaxBlocks


@pytest.fixture(scope='module')
def ctxs(gpu):
    """Contexts by (C, fs, lds): the sample clock is part of a context's configuration, and so is the
    form of the spectra kernel (the plain one is shipped; MKID_OBS_LDS=1 at creation asks for the LDS
    table)."""
    from mkids_sdr_amd.channelizer import Channelizer
    made = {}

    def get(nch=C, fs=oc.FS, lds=False):
        key = (nch, fs, lds)
        if key not in made:
            old = os.environ.get('MKID_OBS_LDS')
            os.environ['MKID_OBS_LDS'] = '1' if lds else '0'
            try:
                made[key] = Channelizer(nch, max_chunk=2 ** 14, sample_rate=fs)
            finally:
                os.environ.pop('MKID_OBS_LDS')
                if old is not None:
                    os.environ['MKID_OBS_LDS'] = old
        return made[key]

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


def dev_count(ctx, ev, j0, n_seconds, count=None, cap=None, image=None, outside=None):
    """Device count -> (image, outside) on the host; count: a device-side count with capacity cap."""
    d_ev = _dev(ev) if len(ev) else None
    d_image = _dev(np.zeros((n_seconds, ctx.C), np.int32) if image is None else image)
    d_out = _dev(np.zeros(2, np.int64) if outside is None else outside)
    if count is None:
        ctx.count_photons_device(d_ev, len(ev), j0, n_seconds, d_image, d_out)
    else:
        ctx.count_photons_counted(d_ev, _dev(np.array([count], np.int64)), cap, j0, n_seconds, d_image, d_out)
    return _host(d_image, d_out)


def dev_spectra(ctx, ev, h, j0, j_defer, lo, inv, nbins, defer=False, cap_def=0, count=None, cap=None,
                spectra=None):
    """Device spectra -> (spectra, deferred, ndef) on the host."""
    d_ev, d_h = (_dev(ev), _dev(np.asarray(h, np.float32))) if len(ev) else (None, None)
    d_sp = _dev(np.zeros((ctx.C, nbins + 3), np.int32) if spectra is None else spectra)
    d_def = _dev(np.full(max(cap_def, 1), 0x7777, np.uint64)) if defer else None
    d_ndef = _dev(np.zeros(2, np.int64)) if defer else None
    args = (j0, j_defer, _dev(lo), _dev(inv), nbins, d_sp, d_def, cap_def, d_ndef)
    if count is None:
        ctx.height_spectra_device(d_ev, d_h, len(ev), *args)
    else:
        ctx.height_spectra_counted(d_ev, d_h, _dev(np.array([count], np.int64)), cap, *args)
    if not defer:
        return _host(d_sp)[0], np.zeros(0, np.uint64), np.zeros(2, np.int64)
    sp, d, ndef = _host(d_sp, d_def, d_ndef)
    d = d.view(np.uint64)
    assert np.all(d[int(ndef[1]):] == 0x7777)          # nothing past the written part
    return sp, d[:int(ndef[1])], ndef


def _parity(ctx, c, defer=False, cap_def=0, lds_ctx=None):
    jd = c.get('j_defer', 0)
    image, outside = dev_count(ctx, c['ev'], c['j0'], c['n_seconds'])
    rc, himage, houtside = oc.count_host(c['ev'], c['j0'], ctx.N, c['fs'], ctx.C, c['n_seconds'])
    assert rc == 0 and np.array_equal(image, himage) and np.array_equal(outside, houtside)
    got = dev_spectra(ctx, c['ev'], c['h'], c['j0'], jd, c['lo'], c['inv'], c['nbins'], defer, cap_def)
    rc, hsp, hd, hn = oc.spectra_host(c['ev'], c['h'], c['j0'], jd, ctx.C, c['lo'], c['inv'], c['nbins'], defer, cap_def)
    assert rc == 0
    assert np.array_equal(got[0], hsp) and np.array_equal(got[1], hd) and np.array_equal(got[2], hn)
    if lds_ctx is not None:                             # the LDS form of the same kernel
        again = dev_spectra(lds_ctx, c['ev'], c['h'], c['j0'], jd, c['lo'], c['inv'], c['nbins'], defer, cap_def)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
    return image, outside, got


CASES = oc.cases(C, 2 * C)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_parity_case_table(ctxs, c):
    image, outside, got = _parity(ctxs(C, c['fs']), c, lds_ctx=ctxs(C, c['fs'], lds=True))
    assert image.sum() + outside.sum() == len(c['ev']) and image.sum() > 0


def test_parity_channel_change_every_packet_1024(ctxs):
    """C = 1024, one packet per channel: every run has length 1, and a spectra slice spans more
    channels than the LDS table has rows."""
    c = next(c for c in oc.cases(1024, 2048) if c['name'] == 'channel_change_every_packet')
    image, _, got = _parity(ctxs(1024), c, lds_ctx=ctxs(1024, lds=True))
    assert image.sum() == 1024 and image.max() == 1 and got[0].sum() == 1024


@pytest.mark.parametrize('nbins', [1, 2, 256, 16384])
def test_parity_column_rule(ctxs, nbins):
    """The column cases, nbins = 16384 among them, where no LDS row fits."""
    _parity(ctxs(), oc.column_case(C, nbins), lds_ctx=ctxs(lds=True))


def test_parity_deferred(ctxs):
    c = oc.deferred_case(C, 2 * C)
    ch, jg = oc.decode(c['ev'], c['j0'])
    nq = int(((ch < C) & ~np.isfinite(c['h']) & (jg >= c['j_defer'])).sum())
    assert nq > 20
    for cap_def in (nq + 5, nq, nq - 7, 1, 0):
        _, _, (sp, d, ndef) = _parity(ctxs(), c, defer=True, cap_def=cap_def, lds_ctx=ctxs(lds=True))
        assert ndef[0] == nq and ndef[1] == min(nq, cap_def)
        assert sp.sum() + ndef[1] == (ch < C).sum() - (ndef[0] - ndef[1])


def _long_list(n, seed, nch=C):
    """n packets in the device's order over two seconds, channels >= nch among them."""
    rng = np.random.default_rng(seed)
    tb = packets.Timebase(oc.FS, 2 * nch)
    ch = np.where(rng.random(n) < 0.02, rng.integers(nch, 4096, n), rng.integers(0, nch, n))
    ev = oc.device_order(oc.pack(ch, rng.integers(0, tb.first_row(2) + 50, n), rng), 0)
    lo, inv = oc.bins(nch, 64, rng)
    return dict(name='long', C=nch, N=2 * nch, fs=oc.FS, j0=0, n_seconds=2, ev=ev, h=oc.heights_for(n, rng), nbins=64,
                lo=lo, inv=inv, j_defer=tb.first_row(1))


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 256, 257, SLICE + 5, 2 * SLICE + 300])
def test_small_lists_and_one_slice(ctxs, n):
    c = _long_list(n, 20 + n)
    _parity(ctxs(), c, defer=True, cap_def=n, lds_ctx=ctxs(lds=True))


def test_past_the_grid(ctxs):
    """A list a little longer than the spectra grid's largest slices of kObsSlice (its slices grow)
    and longer than the count kernel's grid stride, with the deferred list cut by cap_def; and two
    runs give the same bits."""
    c = _long_list(MAX_BLOCKS * SLICE + 300, 31)
    a = _parity(ctxs(), c, defer=True, cap_def=5000, lds_ctx=ctxs(lds=True))
    assert a[2][2][0] > 5000 and a[2][2][1] == 5000
    b = _parity(ctxs(), c, defer=True, cap_def=5000)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def test_counted_forms(ctxs):
    """*d_count < n: the packet after the last valid one is of the same cell as the last valid one and
    must not act as its neighbour; *d_count > cap; *d_count == 0."""
    ctx = ctxs()
    c = _long_list(3000, 33)
    ch, jg = oc.decode(c['ev'], 0)
    sec = packets.Timebase(oc.FS, ctx.N).second(jg)
    same = np.flatnonzero((ch[1:] == ch[:-1]) & (sec[1:] == sec[:-1]) & (ch[1:] < C)) + 1
    assert same.size > 100
    for count, cap in ((int(same[same.size // 2]), 3000), (int(same[5]), 2900), (5000, 2000), (0, 3000), (1, 3000),
                       (3000, 3000)):
        m = min(count, cap)
        image, outside = dev_count(ctx, c['ev'], 0, 2, count=count, cap=cap)
        _, himage, houtside = oc.count_host(c['ev'][:m], 0, ctx.N, oc.FS, C, 2)
        assert np.array_equal(image, himage) and np.array_equal(outside, houtside), (count, cap)
        got = dev_spectra(ctx, c['ev'], c['h'], 0, c['j_defer'], c['lo'], c['inv'], 64, True, 3000, count=count, cap=cap)
        _, hsp, hd, hn = oc.spectra_host(c['ev'][:m], c['h'][:m], 0, c['j_defer'], C, c['lo'], c['inv'], 64, True, 3000)
        assert np.array_equal(got[0], hsp) and np.array_equal(got[1], hd) and np.array_equal(got[2], hn), (count, cap)


def test_prefix_contribution(ctxs):
    """A list ten times longer with the same prefix: its results are the prefix's plus the rest's,
    and the results continue in caller-owned buffers."""
    ctx = ctxs()
    big = _long_list(30000, 35)
    rng = np.random.default_rng(36)
    big['ev'], big['h'] = big['ev'].copy(), big['h'].copy()
    p = rng.permutation(30000)                      # the prefix need not be sorted like the rest
    big['ev'], big['h'] = big['ev'][p], big['h'][p]
    big['ev'][:3000] = oc.device_order(big['ev'][:3000], 0)
    pre = dict(big, ev=big['ev'][:3000], h=big['h'][:3000])
    rest = dict(big, ev=big['ev'][3000:], h=big['h'][3000:])
    pi, po, (ps, _, _) = _parity(ctx, pre)
    bi, bo, (bs, _, _) = _parity(ctx, big)
    _, ri, ro = oc.count_host(rest['ev'], 0, ctx.N, oc.FS, C, 2)
    _, rs, _, _ = oc.spectra_host(rest['ev'], rest['h'], 0, 0, C, big['lo'], big['inv'], 64)
    assert np.array_equal(bi, pi + ri) and np.array_equal(bo, po + ro) and np.array_equal(bs, ps + rs)
    ci, co = dev_count(ctx, rest['ev'], 0, 2, image=pi, outside=po)            # continued
    cs, _, _ = dev_spectra(ctx, rest['ev'], rest['h'], 0, 0, big['lo'], big['inv'], 64, spectra=ps)
    assert np.array_equal(ci, bi) and np.array_equal(co, bo) and np.array_equal(cs, bs)


def test_concat_packets(ctxs):
    ctx = ctxs()
    rng = np.random.default_rng(37)
    a, b = (rng.integers(0, 1 << 62, n).astype(np.uint64) for n in (700, 900))
    d_a, d_b = _dev(a), _dev(b)
    for na, cap_a, nb, cap_b, cap_out in ((300, 700, 500, 900, 2000), (0, 700, 500, 900, 2000), (300, 700, 0, 900, 2000),
                                          (0, 700, 0, 900, 2000), (900, 700, 1200, 900, 2000), (700, 700, 900, 900, 1000),
                                          (300, 700, 500, 900, 300), (300, 700, 500, 900, 299), (300, 700, 500, 900, 0),
                                          (5, 0, 500, 900, 2000), (-3, 700, 10, 900, 2000)):
        d_out = _dev(np.full(max(cap_out, 1) + 8, 0x5555, np.uint64))
        d_nout = _dev(np.full(2, -1, np.int64))
        ctx.concat_packets(d_a if cap_a else None, _dev(np.array([na], np.int64)), cap_a, d_b,
                           _dev(np.array([nb], np.int64)), cap_b, d_out, cap_out, d_nout)
        out, nout = _host(d_out, d_nout)
        out = out.view(np.uint64)
        ref = np.concatenate([a[:max(min(na, cap_a), 0)], b[:max(min(nb, cap_b), 0)]])
        assert np.array_equal(nout, [len(ref), min(len(ref), cap_out)])
        assert np.array_equal(out[:nout[1]], ref[:cap_out]) and np.all(out[nout[1]:] == 0x5555)


def _code(fn):
    with pytest.raises(_lib.MkidError) as e:
        fn()
    return e.value.code


def test_argument_errors(ctxs):
    """Every MKID_E_ARG case fails before any launch: the outputs stay as they were."""
    from mkids_sdr_amd.channelizer import Channelizer
    ctx = ctxs()
    c = _long_list(500, 38)
    d_ev, d_h, d_lo, d_inv = _dev(c['ev']), _dev(c['h']), _dev(c['lo']), _dev(c['inv'])
    d_image, d_out = _dev(np.full((2, C), 7, np.int32)), _dev(np.full(2, 7, np.int64))
    d_sp, d_def, d_ndef = _dev(np.full((C, 67), 7, np.int32)), _dev(np.full(500, 7, np.int64)), _dev(np.full(2, 7, np.int64))
    d_cnt = _dev(np.array([500], np.int64))

    def count(**kw):
        a = dict(ev=d_ev, n=500, j0=0, ns=2, image=d_image, out=d_out)
        a.update(kw)
        if 'cnt' in a:
            return ctx.count_photons_counted(a['ev'], a['cnt'], a['n'], a['j0'], a['ns'], a['image'], a['out'])
        return ctx.count_photons_device(a['ev'], a['n'], a['j0'], a['ns'], a['image'], a['out'])

    def spec(**kw):
        a = dict(ev=d_ev, h=d_h, n=500, j0=0, jd=0, lo=d_lo, inv=d_inv, nbins=64, sp=d_sp, d=d_def, cap=500, ndef=d_ndef)
        a.update(kw)
        rest = (a['j0'], a['jd'], a['lo'], a['inv'], a['nbins'], a['sp'], a['d'], a['cap'], a['ndef'])
        if 'cnt' in a:
            return ctx.height_spectra_counted(a['ev'], a['h'], a['cnt'], a['n'], *rest)
        return ctx.height_spectra_device(a['ev'], a['h'], a['n'], *rest)

    for kw in (dict(ev=None), dict(image=None), dict(out=None), dict(n=-1), dict(j0=-1), dict(j0=1 << 62), dict(ns=0),
               dict(ns=(1 << 20) + 1), dict(cnt=None), dict(cnt=d_cnt, n=-1)):
        assert _code(lambda: count(**kw)) == _lib.MKID_E_ARG, kw
    for kw in (dict(ev=None), dict(h=None), dict(lo=None), dict(inv=None), dict(sp=None), dict(n=-1), dict(j0=-1),
               dict(cap=-1), dict(nbins=0), dict(nbins=16385), dict(ndef=None), dict(cnt=None), dict(cnt=d_cnt, n=-1)):
        assert _code(lambda: spec(**kw)) == _lib.MKID_E_ARG, kw
    cat = lambda *a: ctx.concat_packets(*a)
    d_n = _dev(np.array([3], np.int64))
    for a in ((d_ev, None, 5, d_ev, d_n, 5, d_def, 10, d_ndef), (d_ev, d_n, 5, d_ev, None, 5, d_def, 10, d_ndef),
              (d_ev, d_n, 5, d_ev, d_n, 5, d_def, 10, None), (d_ev, d_n, -1, d_ev, d_n, 5, d_def, 10, d_ndef),
              (d_ev, d_n, 5, d_ev, d_n, -1, d_def, 10, d_ndef), (d_ev, d_n, 5, d_ev, d_n, 5, d_def, -1, d_ndef),
              (None, d_n, 5, d_ev, d_n, 5, d_def, 10, d_ndef), (d_ev, d_n, 5, None, d_n, 5, d_def, 10, d_ndef),
              (d_ev, d_n, 5, d_ev, d_n, 5, None, 10, d_ndef)):
        assert _code(lambda: cat(*a)) == _lib.MKID_E_ARG
    L = ctx._L
    assert L.mkid_count_photons(None, None, 0, 0, 1, None, None) == _lib.MKID_E_ARG
    assert L.mkid_height_spectra(None, None, None, 0, 0, 0, None, None, 1, None, None, 0, None) == _lib.MKID_E_ARG
    assert L.mkid_concat_packets(None, None, None, 0, None, None, 0, None, 0, None) == _lib.MKID_E_ARG
    # a sample clock that is not an integer number of samples per second
    odd = Channelizer(C, max_chunk=2 ** 14, sample_rate=1e6 + 0.5)
    try:
        assert _code(lambda: odd.count_photons_device(d_ev, 500, 0, 2, d_image, d_out)) == _lib.MKID_E_ARG
    finally:
        odd.close()
    for t in _host(d_image, d_out, d_sp, d_def, d_ndef):
        assert np.all(t == 7)
    # and the valid edges: n == 0 without lists, no deferred list
    count(n=0, ev=None)
    spec(n=0, ev=None, h=None)
    spec(d=None, ndef=None)
    image, sp, ndef = _host(d_image, d_sp, d_ndef)
    assert np.all(image == 7) and np.all(ndef == 7) and sp.sum() == 7 * sp.size + (oc.decode(c['ev'], 0)[0] < C).sum()


def test_observation_end_to_end(gpu):
    """Four process_device calls, each followed by Observation.step, with no host synchronisation
    until the end (the debug copies are taken from a second, identical run)."""
    import torch
    import signals
    from mkids_sdr_amd.channelizer import Channelizer
    S, K, ncoeff, pre, nbins = 2 ** 15, 4, 40, 10, 32
    J = S // (2 * C)
    fs = 2 * C * 600                                    # 600 rows per second: the run crosses second 1
    case = signals.make_case(C, K * S, seed=7, pulses_per_ch=24.0)
    quiet = signals.make_case(C, S, seed=7, pulses_per_ch=0)
    thr = signals.thresholds_from_quiet(quiet, signals.oracle_chain(quiet).process(quiet.iq)['raw'])
    coeff = np.random.default_rng(41).normal(size=(C, ncoeff)).astype(np.float32)
    x = torch.from_numpy(case.iq.reshape(-1)).to('cuda')
    cap = J * C
    runs = []
    for debug in (False, True):
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
            obs = observe.Observation(ch, 2, nbins, -20.0, 40.0 / nbins, cap, cap, debug=debug)
            bufs = [(torch.empty((J, C), dtype=torch.float32, device='cuda'),
                     torch.empty(cap, dtype=torch.int64, device='cuda'),
                     torch.zeros(2, dtype=torch.int64, device='cuda')) for _ in range(K)]
            torch.cuda.synchronize()
            for k, (d_ph, d_ev, d_cnt) in enumerate(bufs):
                ch.process_device(x[2 * k * S:2 * (k + 1) * S], S, d_ph, d_ev, cap, d_cnt)
                obs.step(d_ph, J, k * J, d_ev, d_cnt)
            torch.cuda.synchronize()
            evs = [d_ev[:int(d_cnt[1].item())].cpu().numpy().view(np.uint64) for _, d_ev, d_cnt in bufs]
            assert all(int(d_cnt[0].item()) == int(d_cnt[1].item()) for _, _, d_cnt in bufs)
            runs.append(dict(image=obs.image(), spectra=obs.spectra(), outside=obs.outside(), pending=obs.pending(),
                             counts=obs.photon_counts(3), evs=evs, steps=obs.steps, lo=obs.lo, inv=obs.inv,
                             ndef=obs.deferred_counts(), edges=obs.edges(3)))
        finally:
            ch.close()
    a, b = runs
    for k in ('image', 'spectra', 'outside', 'pending'):                          # the run repeats bit for bit
        assert np.array_equal(a[k], b[k]), k
    n_all = sum(len(e) for e in a['evs'])
    assert n_all >= K * C and a['ndef'][0] == a['ndef'][1]     # a packet per channel and call on average, at least
    # 1. the image equals the numpy count over all packets of the run
    image, outside = np.zeros((2, C), np.int32), np.zeros(2, np.int64)
    for k, ev in enumerate(a['evs']):
        oc.count_ref(ev, k * J, 2 * C, fs, C, 2, image, outside)
    assert np.array_equal(a['image'], image) and np.array_equal(a['outside'], outside)
    assert image[0].sum() > 0 and image[1].sum() > 0 and image.sum() + outside.sum() == n_all
    assert np.array_equal(a['counts'], np.minimum(image, 2)) and a['edges'].shape == (nbins + 1,)
    # 2. the spectra equal the host twin accumulated over every step's joined list and heights
    sp = np.zeros((C, nbins + 3), np.int32)
    deferred = np.zeros(0, np.uint64)
    for k, (joined, h, j0, jd) in enumerate(b['steps']):
        assert j0 == k * J and jd == observe.j_defer(j0, J, ncoeff, pre)
        assert np.array_equal(joined, np.concatenate([deferred, b['evs'][k]]))    # the join, in order
        rc, _, deferred, _ = oc.spectra_host(joined, h, j0, jd, C, b['lo'], b['inv'], nbins, True, cap, spectra=sp)
        assert rc == 0
        if k < K - 1:
            assert len(deferred) > 0
    assert np.array_equal(a['spectra'], sp) and np.array_equal(a['pending'], deferred)
    # 3. per channel: spectra + pending = packets
    per_ch = np.zeros(C, np.int64)
    for ev in a['evs']:
        np.add.at(per_ch, oc.decode(ev, 0)[0], 1)
    pend = np.bincount(oc.decode(a['pending'], K * J)[0], minlength=C)
    assert np.array_equal(a['spectra'].sum(axis=1) + pend, per_ch)
    # 4. deferral lost nothing but the stream's first windows
    early = sum(int((oc.decode(ev, k * J)[1] < pre).sum()) for k, ev in enumerate(a['evs']))
    assert a['spectra'][:, nbins + 2].sum() == early
    for k, (joined, h, j0, jd) in enumerate(b['steps']):
        _, jg = oc.decode(joined, j0)
        assert np.all(jg[~np.isfinite(h) & (jg < jd)] < pre)
