"""mkid_iq_noise on the device (k_welch.hip) against its host twin mkid_iq_noise_host, which
tests/test_iqnoise_host.py holds against numpy and against IQsweep.AnalyzeNoise's own lines, and
RoachSetup.analyzeNoise through the shim. Device and twin differ only through atan2, sin and cos: the
exact sums, the segment counts and the status are equal, resang and rad within 1e-12 relative, every
stitched bin under the bar of iqnoise_cases.py, fn1k within what the bar allows the line; a repeated
call gives the same bits.

Recorded on an MI355X (profiles/iqnoise/new_gputests.txt): the largest |P - Pref| over the bar is 2e-4
against the host twin on the two small cases, 1.4e-3 at the reference's shape (two channels of
2 000 000 samples, 0.8 s), 0.054 against the golden file and 0.048 through the shim; the 7 tests take
under 4 s.
"""
import ctypes

import numpy as np
import pytest

import iqnoise_cases as nc
from mkids_sdr_amd import _lib, iqnoise

pytestmark = pytest.mark.gpu
C = 64


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(C, max_chunk=2 ** 14)
    yield ch
    ch.close()


def dev_noise(ctx, I, Q, n, off, cfg, fill=-7.0, nullify=()):
    """mkid_iq_noise on [nch][ld] int16 blocks into pre-filled outputs -> (pn, an, res bytes)."""
    import torch
    c = cfg if isinstance(cfg, _lib.IqNoiseCfg) else iqnoise.make_cfg(**cfg)
    nch, ld = I.shape
    no = max(iqnoise.nout(c), 1) if c.nfft_high > 0 else 4096
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    t = dict(i=up(I), q=up(Q), i0=up(off['i0']), q0=up(off['q0']), icen=up(off['icen']), qcen=up(off['qcen']),
             qfit=up(off['qfit']), pn=torch.full((nch, no), fill, dtype=torch.float64, device='cuda'),
             an=torch.full((nch, no), fill, dtype=torch.float64, device='cuda'),
             res=torch.full((nch * nc.RES_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda'))
    a = dict(t)
    for k in nullify:
        a[k] = None
    torch.cuda.synchronize()
    try:
        ctx.iq_noise_device(a['i'], a['q'], n, ld, nch, a['i0'], a['q0'], a['icen'], a['qcen'], a['qfit'],
                            None if 'cfg' in nullify else c, a['pn'], a['an'], a['res'])
    finally:
        torch.cuda.synchronize()
    return t['pn'].cpu().numpy(), t['an'].cpu().numpy(), t['res'].cpu().numpy()


def as_dict(cfg, pn, an, res):
    r = res.view(nc.RES_DT)
    out = {k: r[k].copy() for k in iqnoise.RESULT_FIELDS}
    out.update(pn=pn, an=an, freq=iqnoise.freqs(iqnoise.make_cfg(**cfg)), pad=r['pad'])
    return out


@pytest.mark.parametrize('name', ['fixture2', 'second'])
def test_device_against_host_twin(ctx, name):
    c = nc.noise_case(name)
    nch, n = c['I'].shape
    wide = lambda x: np.ascontiguousarray(np.concatenate([x, np.full((nch, 5), 12345, np.int16)], axis=1))
    ref = nc.with_sums(c['host'], c['ref'])
    first = None
    for group in (0, 0, 1):          # the second call runs on warm tables and workspace
        pn, an, res = dev_noise(ctx, wide(c['I']), wide(c['Q']), n, c['off'], dict(c['cfg'], group=group))
        got = as_dict(c['cfg'], pn, an, res)
        assert np.all(got['pad'] == 0)
        worst = nc.compare_noise(got, ref, c['cfg'], '%s group %d' % (name, group))
        print('%s: device against host twin, largest ratio to the bar %.4f' % (name, worst))
        if first is None:
            first = (pn, an, res)
        else:
            assert nc.same_bits(pn, first[0]) and nc.same_bits(an, first[1]) and nc.same_bits(res, first[2])
    one = {k: v[1:2] for k, v in c['off'].items()}
    pn, an, res = dev_noise(ctx, c['I'][1:2], c['Q'][1:2], n, one, c['cfg'])
    assert nc.same_bits(pn[0], first[0][1]) and nc.same_bits(res, first[2].reshape(nch, -1)[1])


def test_golden_fixture_on_the_device(ctx):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'iqnoise_mlab.npz'))
    cfg = nc.FIXTURE_CFG
    off = {k: g[k] for k in ('i0', 'q0', 'icen', 'qcen', 'qfit')}
    pn, an, res = dev_noise(ctx, g['I'], g['Q'], g['I'].shape[1], off, cfg)
    got = as_dict(cfg, pn, an, res)
    ref = {k: g[k] for k in ('pn', 'an', 'fn1k', 'resang', 'rad', 'S_low', 'S_high', 'qfit')}
    ref.update(freq=got['freq'], status=np.zeros(2, np.int32))
    assert np.all(got['status'] == 0)
    print('golden on the device: largest ratio to the bar %.4f' % nc.compare_noise(got, ref, cfg, 'golden', exact_ints=False))


def test_reference_shape_two_channels(ctx):
    """The 2^18 path once: nch = 2, n = 2 000 000, 262144 / 4096 / 8 / 521 / 5."""
    cfg = nc.REFERENCE_CFG
    I, Q = nc.synth_records(2, 2000000, 78)
    off = nc.synth_offsets(2, 178)
    host = iqnoise.analyze_noise_host(I, Q, nc.fits_of(off), i0=off['i0'], q0=off['q0'], **cfg)
    S = dict(qfit=off['qfit'], S_low=np.zeros(2), S_high=np.zeros(2))
    for ch in range(2):              # S of the bar from the twin's own spectra, all bins, both series
        r = iqnoise.make_cfg(**cfg)
        c, s, rad = np.cos(host['resang'][ch]), np.sin(host['resang'][ch]), host['rad'][ch]
        Ia = ((I[ch] * r.gain) / r.full_scale - off['i0'][ch]) - off['icen'][ch]
        Qa = ((Q[ch] * r.gain) / r.full_scale - off['q0'][ch]) - off['qcen'][ch]
        nI, nQ = (Ia * c + Qa * s) / rad, (Qa * c - Ia * s) / rad
        for key, nfft in (('S_low', r.nfft_low), ('S_high', r.nfft_high)):
            pa, pb = iqnoise.welch_host(np.arctan2(nQ, nI), np.sqrt(nI * nI + nQ * nQ), nfft, r.samprate)
            S[key][ch] = pa.sum() + pb.sum()
    pn, an, res = dev_noise(ctx, I, Q, 2000000, off, cfg)
    got = as_dict(cfg, pn, an, res)
    assert pn.shape == (2, 2552) and list(got['nseg_low']) == [14, 14] and list(got['nseg_high']) == [975, 975]
    worst = nc.compare_noise(got, dict(host, **S), cfg, 'reference shape')
    print('reference shape: device against host twin, largest ratio to the bar %.4f' % worst)


def test_status_bits_on_the_device(ctx):
    cfg = dict(nc.FIXTURE_CFG, gain=1.0, full_scale=1.0)
    n = 20580
    rng = np.random.default_rng(3)
    I = np.rint(30 * rng.standard_normal((4, n))).astype(np.int16) + 100
    Q = np.rint(30 * rng.standard_normal((4, n))).astype(np.int16) - 50
    I[0, -1] -= np.int16(I[0].astype(np.int64).sum() - 100 * n)      # the mean is exactly the centre
    Q[0, -1] -= np.int16(Q[0].astype(np.int64).sum() + 50 * n)
    off = dict(i0=np.zeros(4), q0=np.zeros(4), icen=np.array([100.0, 3.0, 4.0, np.inf]),
               qcen=np.array([-50.0, 2.0, 1.0, 0.0]), qfit=np.array([2e4, 0.0, np.nan, 2e4]))
    pn, an, res = dev_noise(ctx, I, Q, n, off, cfg)
    got = as_dict(cfg, pn, an, res)
    B = _lib
    assert list(got['status']) == [B.IQN_BAD_RAD, B.IQN_BAD_Q, B.IQN_BAD_Q, B.IQN_NONFINITE | B.IQN_BAD_RAD]
    ref = nc.iq_ref(I, Q, off, cfg)
    ref['qfit'] = off['qfit']
    nc.compare_noise(got, ref, cfg, 'status')


def test_argument_errors_launch_nothing(ctx):
    c = nc.noise_case('fixture2')
    I, Q, off, n = c['I'], c['Q'], c['off'], c['I'].shape[1]
    ok = dict(c['cfg'])
    bad_cfg = [dict(nfft_high=4), dict(nfft_high=96), dict(nfft_high=8192, nfft_low=16384), dict(nfft_low=128),
               dict(nfft_low=12288), dict(nfft_low=2 ** 19), dict(k_join=0), dict(k_join=64), dict(fit_first=-1),
               dict(fit_first=186), dict(fit_count=1), dict(group=-1), dict(samprate=0.0), dict(f_eval=float('inf')),
               dict(gain=0.0), dict(full_scale=float('nan'))]
    import torch
    for kw in bad_cfg:
        with pytest.raises(_lib.MkidError) as e:
            dev_noise(ctx, I, Q, n, off, {**ok, **kw})
        assert e.value.code == _lib.MKID_E_ARG, kw
    # the outputs keep their fill pattern: one set of buffers through every refused call
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    t = [up(I), up(Q)] + [up(off[k]) for k in ('i0', 'q0', 'icen', 'qcen', 'qfit')]
    pn = torch.full((2, 190), -7.0, dtype=torch.float64, device='cuda')
    an = torch.full((2, 190), -7.0, dtype=torch.float64, device='cuda')
    res = torch.full((2 * nc.RES_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    calls = [dict(cfg=iqnoise.make_cfg(**{**ok, **kw})) for kw in bad_cfg]
    calls += [dict(null=i) for i in range(7)] + [dict(n=8191), dict(ld=n - 1), dict(nch=0), dict(cfg=None)]
    for kw in calls:
        a = list(t)
        if 'null' in kw:
            a[kw['null']] = None
        with pytest.raises(_lib.MkidError) as e:
            ctx.iq_noise_device(a[0], a[1], kw.get('n', n), kw.get('ld', n), kw.get('nch', 2), *a[2:],
                                kw.get('cfg', iqnoise.make_cfg(**ok)), pn, an, res)
        assert e.value.code == _lib.MKID_E_ARG, kw
    for out in ('pn', 'an', 'res'):
        a = dict(pn=pn, an=an, res=res)
        a[out] = None
        with pytest.raises(_lib.MkidError):
            ctx.iq_noise_device(*t[:2], n, n, 2, *t[2:], iqnoise.make_cfg(**ok), a['pn'], a['an'], a['res'])
    torch.cuda.synchronize()
    assert bool((pn == -7.0).all()) and bool((an == -7.0).all()) and bool((res == 0x5A).all())
    ctx.iq_noise_device(*t[:2], n, n, 2, *t[2:], iqnoise.make_cfg(**ok), pn, an, res)
    torch.cuda.synchronize()
    assert not bool((pn == -7.0).any()) and not bool((res == 0x5A).all())


def test_analyze_noise_through_the_shim(gpu):
    """The 64-channel loop-back feedline with four resonators of test_fit_loops_through_the_shim:
    fitLoops(), then analyzeNoise(rows=2**14, nfft_low=8192, nfft_high=128, ..): self.noise equals
    analyze_noise_host on the same tapped records under the module's rules, and no register is
    written. The fn1k values are printed, not asserted."""
    from mkids_sdr_amd.roach import FpgaClient, RoachSetup
    fs, lo = 128e6, 4.0e9
    roach = FpgaClient(n_channels=C, sample_rate=fs, noise_sigma=4.0, seed=8)
    roach.progdev('pulse_trigger_2022_Jan_24_1322.bof')
    res_hz = fs / 2 ** 16
    offs = np.array([-40e6, -12e6, 21e6, 50e6])
    freqs = list(lo + np.round(offs / res_hz) * res_hz)
    rs = RoachSetup(roach, freqs, lo, n_channels=C, sample_rate=fs)
    rng = np.random.default_rng(2)
    res = [dict(Q=2.0e4, f0=f + 20e3, ang1=float(rng.uniform(-3, 3)), Ioff=float(rng.uniform(-.3, .3)),
                Qoff=float(rng.uniform(-.3, .3))) for f in freqs]
    rs.define_LUTs()
    rs.toggleDAC()
    rs.programLOrev2board(lo, 0)
    roach.set_resonators(res, lo)
    rs.sweepLOready(1.2e6, 24)
    fits = rs.fitLoops()

    writes = []
    write_int, write = roach.write_int, roach.write
    roach.write_int = lambda *a, **k: (writes.append(a), write_int(*a, **k))[1]
    roach.write = lambda *a, **k: (writes.append(a[:1]), write(*a, **k))[1]
    regs, centres = dict(roach.regs), rs.iq_centers.copy()
    cfg = dict(nfft_low=8192, nfft_high=128, k_join=2, fit_first=140, fit_count=5, samprate=1.0e6, f_eval=1.2e5)
    out = rs.analyzeNoise(rows=2 ** 14, **cfg)
    assert out is rs.noise and writes == [] and dict(roach.regs) == regs and np.array_equal(rs.iq_centers, centres)
    assert list(out['channels']) == [0, 1, 2, 3] and out['I'].shape == (4, 2 ** 14) and out['pn'].shape == (4, 190)

    full = dict(cfg, gain=1.0, full_scale=1.0)
    off = dict(i0=np.zeros(4), q0=np.zeros(4), icen=fits['p'][:, 8].copy(), qcen=fits['p'][:, 9].copy(),
               qfit=fits['p'][:, 0].copy())
    host = iqnoise.analyze_noise_host(out['I'], out['Q'], nc.fits_of(off), **full)
    ref = nc.iq_ref(out['I'], out['Q'], off, full)
    ref['qfit'] = off['qfit']
    worst = nc.compare_noise(out, nc.with_sums(host, ref), full, 'shim')
    print('shim: fn1k', out['fn1k'], 'rad', out['rad'], 'status', out['status'], 'largest ratio to the bar %.4f' % worst)
    two = rs.analyzeNoise(rows=2 ** 14, channels=[2, 0], **cfg)
    assert list(two['channels']) == [2, 0] and two['pn'].shape == (2, 190) and writes == []
