"""mkid_iq_noise_host (csrc/welch_common.h through mkid_iqnoise.hip) against the numpy restatement of
iqnoise_cases.py, against tests/golden/iqnoise_mlab.npz (IQsweep.AnalyzeNoise's own lines with
matplotlib.mlab.psd and np.polyfit, made by tools/make_iqnoise_golden.py), and at the reference's own
shape; status bits, argument errors, the frequency axis and LoadNoise's file layout. No GPU. The rules
of a comparison are iqnoise_cases.compare_noise's; no stitched bin is left out.

Observed here: the largest |P - Pref| over the bar is 0.027 against the golden file, 0.013
against the restatement on the two small cases and 0.0092 at the reference's shape (n = 2 000 000,
262144 / 4096); fn1k agrees with np.polyfit's line to the digits printed.
"""
import ctypes
import os

import numpy as np
import pytest

import iqnoise_cases as nc
from mkids_sdr_amd import _lib, iqnoise

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'iqnoise_mlab.npz')


def test_golden_mlab_fixture():
    g = np.load(GOLDEN)
    cfg = {k: g['cfg_' + k].item() for k in nc.FIXTURE_CFG}
    assert cfg == nc.FIXTURE_CFG
    off = {k: g[k] for k in ('i0', 'q0', 'icen', 'qcen', 'qfit')}
    got = iqnoise.analyze_noise_host(g['I'], g['Q'], nc.fits_of(off), i0=off['i0'], q0=off['q0'], **cfg)
    assert got['pn'].shape == (2, 190) and np.all(got['status'] == 0)
    assert np.all(np.abs(got['freq'] - g['pnidx'][0]) <= 2 * np.spacing(g['pnidx'][0]))
    ref = {k: g[k] for k in ('pn', 'an', 'fn1k', 'resang', 'rad', 'S_low', 'S_high', 'qfit')}
    ref.update(freq=got['freq'], status=np.zeros(2, np.int32))
    worst = nc.compare_noise(got, ref, cfg, 'golden', exact_ints=False)
    print('golden: largest ratio to the bar %.4f' % worst)


@pytest.mark.parametrize('name', ['fixture2', 'second'])
def test_twin_against_restatement(name):
    c = nc.noise_case(name)
    assert np.all(c['ref']['status'] == 0)
    for k in ('mean_i', 'mean_q'):
        assert np.allclose(c['host'][k], c['ref'][k], rtol=1e-14, atol=0)
    worst = nc.compare_noise(c['host'], c['ref'], c['cfg'], name)
    print('%s: largest ratio to the bar %.4f' % (name, worst))


def test_reference_shape_once():
    """nch = 1, n = 2 000 000, 262144 / 4096 / 8 / 521 / 5: 2552 stitched bins, 14 and 975 segments."""
    cfg = nc.REFERENCE_CFG
    I, Q = nc.synth_records(1, 2000000, 77)
    off = nc.synth_offsets(1, 177)
    got = iqnoise.analyze_noise_host(I, Q, nc.fits_of(off), i0=off['i0'], q0=off['q0'], **cfg)
    assert got['pn'].shape == (1, 2552) and got['freq'].shape == (2552,)
    assert got['nseg_low'][0] == 14 and got['nseg_high'][0] == 975
    ref = nc.iq_ref(I, Q, off, cfg)
    ref['qfit'] = off['qfit']
    worst = nc.compare_noise(got, ref, cfg, 'reference shape')
    print('reference shape: largest ratio to the bar %.4f' % worst)


def test_block_stride_and_grouping_give_the_same_bits():
    c = nc.noise_case('fixture2')
    nch, n = c['I'].shape
    wide = lambda x: np.ascontiguousarray(np.concatenate([x, np.full((nch, 3), 12345, np.int16)], axis=1))
    for group in (0, 1):
        rc, pn, an, res = nc.host_noise(wide(c['I']), wide(c['Q']), n, c['off'], dict(c['cfg'], group=group))
        assert rc == 0 and nc.same_bits(pn, c['host']['pn']) and nc.same_bits(an, c['host']['an'])
        r = res.view(nc.RES_DT)
        assert all(nc.same_bits(r[k], c['host'][k]) for k in iqnoise.RESULT_FIELDS) and np.all(r['pad'] == 0)
    one = {k: v[1:2] for k, v in c['off'].items()}
    rc, pn, an, res = nc.host_noise(c['I'][1:2].copy(), c['Q'][1:2].copy(), n, one, c['cfg'])
    assert rc == 0 and nc.same_bits(pn[0], c['host']['pn'][1]) and nc.same_bits(res.view(nc.RES_DT)['fn1k'],
                                                                            c['host']['fn1k'][1:2])


def test_status_bits():
    """rad == 0 is reached with a record whose mean equals the centre: NaN spectra and fn1k; a zero or
    non-finite Q leaves the spectra and makes fn1k NaN; a non-finite offset sets its bit (and rad's)."""
    cfg = dict(nc.FIXTURE_CFG, gain=1.0, full_scale=1.0)
    n = 20580
    rng = np.random.default_rng(3)
    I = np.rint(30 * rng.standard_normal((4, n))).astype(np.int16) + 100
    Q = np.rint(30 * rng.standard_normal((4, n))).astype(np.int16) - 50
    I[0, -1] -= np.int16(I[0].astype(np.int64).sum() - 100 * n)      # the mean is exactly (100, -50)
    Q[0, -1] -= np.int16(Q[0].astype(np.int64).sum() + 50 * n)
    off = dict(i0=np.zeros(4), q0=np.zeros(4), icen=np.array([100.0, 3.0, 4.0, np.inf]),
               qcen=np.array([-50.0, 2.0, 1.0, 0.0]), qfit=np.array([2e4, 0.0, np.nan, 2e4]))
    got = iqnoise.analyze_noise_host(I, Q, nc.fits_of(off), **cfg)
    B = _lib
    assert list(got['status']) == [B.IQN_BAD_RAD, B.IQN_BAD_Q, B.IQN_BAD_Q, B.IQN_NONFINITE | B.IQN_BAD_RAD]
    assert got['rad'][0] == 0.0 and got['sum_i'][0] == 100 * n and got['sum_q'][0] == -50 * n
    for ch in (0, 3):
        assert np.all(np.isnan(got['pn'][ch])) and np.all(np.isnan(got['an'][ch])) and np.isnan(got['fn1k'][ch])
    for ch in (1, 2):
        assert np.all(np.isfinite(got['pn'][ch])) and np.all(np.isfinite(got['an'][ch])) and np.isnan(got['fn1k'][ch])
    ref = nc.iq_ref(I, Q, off, cfg)
    ref['qfit'] = off['qfit']
    nc.compare_noise(got, ref, cfg, 'status')


def test_argument_errors_touch_nothing():
    c = nc.noise_case('fixture2')
    I, Q, off, n = np.ascontiguousarray(c['I']), np.ascontiguousarray(c['Q']), c['off'], c['I'].shape[1]
    ok = dict(c['cfg'])
    bad_cfg = [dict(nfft_high=4), dict(nfft_high=96), dict(nfft_high=8192, nfft_low=16384), dict(nfft_low=128),
               dict(nfft_low=64), dict(nfft_low=12288), dict(nfft_low=2 ** 19), dict(k_join=0), dict(k_join=64),
               dict(k_join=63, nfft_high=64), dict(fit_first=-1), dict(fit_first=186),
               dict(fit_count=1), dict(group=-1), dict(samprate=0.0), dict(samprate=float('nan')),
               dict(f_eval=float('inf')), dict(gain=0.0), dict(gain=float('nan')), dict(full_scale=0.0),
               dict(full_scale=float('inf'))]
    for kw in bad_cfg:
        rc, pn, an, res = nc.host_noise(I, Q, n, off, {**ok, **kw})
        assert rc == _lib.MKID_E_ARG, kw
        assert np.all(pn == -7.0) and np.all(an == -7.0) and np.all(res == 0x5A), kw
        with pytest.raises(_lib.MkidError):
            iqnoise.freqs(iqnoise.make_cfg(**{**ok, **kw}))
    for null in ('i', 'q', 'i0', 'q0', 'icen', 'qcen', 'qfit', 'pn', 'an', 'res', 'cfg'):
        rc, pn, an, res = nc.host_noise(I, Q, n, off, ok, nullify=(null,))
        assert rc == _lib.MKID_E_ARG and np.all(pn == -7.0) and np.all(an == -7.0) and np.all(res == 0x5A), null
    for nn in (8191, n + 1):          # n < nfft_low; ld < n
        rc, pn, an, res = nc.host_noise(I, Q, nn, off, ok)
        assert rc == _lib.MKID_E_ARG and np.all(pn == -7.0) and np.all(res == 0x5A)
    rc, pn, an, res = nc.host_noise(I, Q, n, off, ok)
    assert rc == 0 and not np.any(pn == -7.0) and not np.all(res == 0x5A)


def test_frequency_axis():
    f = iqnoise.freqs()
    assert f.shape == (2552,) and iqnoise.nout(iqnoise.make_cfg()) == 2552
    assert np.array_equal(f[:512], np.arange(512) * (200000.0 / 262144))
    assert np.array_equal(f[512:], np.arange(8, 2048) * (200000.0 / 4096))
    assert f[521] < 1000.0 < f[525]          # the reference's five bins straddle 1 kHz
    with pytest.raises(TypeError):
        iqnoise.make_cfg(nfft=4096)


def test_load_noise_layout(tmp_path):
    """LoadNoise's layout: 12 float64, then ten blocks of 200000 int16 I, Q of resonator 0, then of 1."""
    rng = np.random.default_rng(9)
    hdr = rng.standard_normal(12)
    blocks = rng.integers(-30000, 30000, (10, 4, 200000)).astype(np.int16)
    path = tmp_path / 'noise.dat'
    with open(path, 'wb') as f:
        f.write(hdr.tobytes())
        f.write(blocks.tobytes())
    for resnum, k in ((0, 0), (1, 2)):
        h, I, Q = iqnoise.load_noise(str(path), resnum)
        assert np.array_equal(h, hdr) and I.dtype == np.int16 and I.shape == (2000000,)
        assert np.array_equal(I, blocks[:, k].reshape(-1)) and np.array_equal(Q, blocks[:, k + 1].reshape(-1))
    short = tmp_path / 'short.dat'
    short.write_bytes(b'\0' * 9)
    with pytest.raises(ValueError):
        iqnoise.load_noise(str(short), 0)
