"""mkid_welch_psd_host (csrc/welch_common.h through mkid_iqnoise.hip) against a numpy restatement of
the rule of include/mkidgpu.h, against the same rule in long double (scipy.fft), against the closed
form for an impulse, and, where matplotlib is installed, the restatement against matplotlib.mlab.psd.
No GPU. The bar and the cases are iqnoise_cases.py's; no bin of any case is left out.

Observed here (the eta a difference needs, in units of 2^-53 log2(nfft); the bar is 4): over every
shape and input kind the host twin needs at most 0.37 against the numpy restatement and at most
0.51 against the long-double truth (numpy itself: 0.51, at nfft = 8); the largest |P - Pref| over the
bar is 0.086. The restatement differs from mlab.psd by at most 2.5e-13 relative in a bin, and its
frequency axis by at most 1 ulp.
"""
import numpy as np
import pytest

import iqnoise_cases as nc
from mkids_sdr_amd import _lib


@pytest.mark.parametrize('nfft,n', nc.SHAPES)
def test_twin_against_restatement_and_truth(nfft, n):
    """Every kind of a shape, run alone: under the bar against np.fft.fft's restatement and against
    the long-double truth, S being the truth's; all-zero series give exactly 0.0, never NaN; an impulse
    gives its closed form."""
    ins, (ja, jb) = nc.welch_inputs(nfft, n)
    got = nc.host_kinds(nfft, n)
    for kind in nc.KINDS:
        a, b = ins[kind]
        pa, pb = got[kind]
        assert np.all(np.isfinite(pa)) and np.all(np.isfinite(pb)) and np.all(pa >= 0) and np.all(pb >= 0)
        ra, rb = nc.welch_ref(a, b, nfft, nc.FS)
        ta, tb = nc.welch_ref(a, b, nfft, nc.FS, long_double=True)
        S = float(ta.sum() + tb.sum())
        for p, r, t in ((pa, ra, ta), (pb, rb, tb)):
            if kind == 'zeros':
                assert np.all(p == 0.0)          # exactly; a zero series beside a live one is under the bar
            u = (nc.units(p, r, S, nfft), nc.units(p, t, S, nfft), nc.units(r, t, S, nfft))
            print('nfft %d n %d %-7s eta needed: twin-numpy %.4f twin-truth %.4f numpy-truth %.4f; ratio to the bar %.4f'
                  % (nfft, n, kind, u[0], u[1], u[2], max(nc.ratio(p, r, S, nfft).max(), nc.ratio(p, t, S, nfft).max())))
            assert np.all(nc.ratio(p, r, S, nfft) <= 1.0) and np.all(nc.ratio(p, t, S, nfft) <= 1.0), (kind, u)
        if kind == 'impulse':
            for p, j0 in ((pa, ja), (pb, jb)):
                cf = nc.impulse_psd(nfft, n, j0, nc.FS)
                assert cf.max() > 0 and np.all(nc.ratio(p, cf, S, nfft) <= 1.0)


@pytest.mark.parametrize('nfft,n', [s for s in nc.SHAPES if s[0] < 262144])
def test_blocks_strides_and_groups_give_the_same_bits(nfft, n):
    """A channel alone (nch = 1, ld = n), in a block of 3 (ld = n + 1, NaN padding), with group 1 and
    group 0, and without the second output gives the same bits; a null b is a row of zeros."""
    ins, _ = nc.welch_inputs(nfft, n)
    alone = nc.host_kinds(nfft, n)
    for kinds in (nc.KINDS[:3], nc.KINDS[3:]):
        A = nc.block([ins[k][0] for k in kinds], n + 1)
        B = nc.block([ins[k][1] for k in kinds], n + 1)
        for group in (0, 1, 2):
            rc, pa, pb = nc.host_psd(A, B, n, nfft, group=group)
            assert rc == 0
            for i, k in enumerate(kinds):
                assert nc.same_bits(pa[i], alone[k][0]) and nc.same_bits(pb[i], alone[k][1]), (k, group)
        rc, pa, pb = nc.host_psd(A, B, n, nfft, want_b=False)
        assert rc == 0 and pb is None and all(nc.same_bits(pa[i], alone[k][0]) for i, k in enumerate(kinds))
    rc, pa, _ = nc.host_psd(nc.block([ins['a_only'][0]], n), None, n, nfft)
    assert rc == 0 and nc.same_bits(pa[0], alone['a_only'][0])


def test_strips_are_summed_as_stated():
    """nfft = 8 with 34 segments, so two strips: the twin equals numpy's segment powers added strip by
    strip (32, then 2; each from 0.0, then the strips from 0.0) within 1e-13 relative in every bin."""
    nfft, n = 8, 143
    a, b = nc.welch_inputs(nfft, n)[0]['white']
    assert (n - 4) // 4 == 34 > nc.STRIP
    pa, _ = nc.host_kinds(nfft, n)['white']
    w, S2 = nc.window(nfft)
    seg = np.array([np.abs(np.fft.fft(a[4 * s:4 * s + 8] * w)[:5]) ** 2 for s in range(34)])
    strips = np.zeros(5)
    for s0 in (0, 32):
        st = np.zeros(5)
        for s in range(s0, min(34, s0 + 32)):
            st = st + seg[s]
        strips = strips + st
    scale = np.array([1, 2, 2, 2, 1.0])
    assert np.allclose(pa, strips / 34 / (nc.FS * S2) * scale, rtol=1e-13, atol=0)


def test_restatement_equals_mlab_psd():
    """Where matplotlib is installed: the restatement is mlab.psd with its defaults, within 1e-11
    relative per bin (measured: 1.1e-12, on the amplitude series), the frequency axis within 2 ulp."""
    mlab = pytest.importorskip('matplotlib.mlab')
    case = nc.noise_case('fixture2')
    I, Q, off, cfg = case['I'], case['Q'], case['off'], case['cfg']
    x = (I[0] * cfg['gain'] / cfg['full_scale'] - off['icen'][0])
    y = (Q[0] * cfg['gain'] / cfg['full_scale'] - off['qcen'][0])
    phase, amp = np.arctan2(y, x), np.hypot(x, y) / np.hypot(x, y).mean()
    worst, worst_f = 0.0, 0.0
    for nfft in (8192, 128):
        ra, rb = nc.welch_ref(phase, amp, nfft, nc.FS)
        for r, s in ((ra, phase), (rb, amp)):
            m, f = mlab.psd(s, NFFT=nfft, Fs=nc.FS, noverlap=nfft // 2)
            worst = max(worst, float(np.max(np.abs(r - m) / m)))
            mine = np.arange(nfft // 2 + 1) * (nc.FS / nfft)
            worst_f = max(worst_f, float(np.max(np.abs(mine - f) / np.spacing(np.maximum(f, 1e-300)))))
    print('restatement against mlab.psd: %.3e relative, frequency axis %.1f ulp' % (worst, worst_f))
    assert worst <= 1e-11 and worst_f <= 2.0


def test_argument_errors_touch_nothing():
    a = nc.block([np.arange(40.0)], 41)
    ok = dict(n=40, nfft=16, fs=nc.FS, group=0)
    rc, pa, pb = nc.host_psd(a, a, **ok)
    assert rc == 0 and not np.any(pa == -7.0) and not np.any(pb == -7.0)
    bad = [dict(nfft=12), dict(nfft=4), dict(nfft=0), dict(nfft=2 ** 19), dict(n=15), dict(n=42), dict(group=-1),
           dict(fs=0.0), dict(fs=-1.0), dict(fs=float('nan')), dict(fs=float('inf'))]
    for kw in bad:
        rc, pa, pb = nc.host_psd(a, a, **{**ok, **kw})
        assert rc == _lib.MKID_E_ARG, kw
        assert np.all(pa == -7.0) and np.all(pb == -7.0), kw
    L = _lib.load()
    out = np.full((1, 9), -7.0)
    p = lambda x: x.ctypes.data_as(__import__('ctypes').c_void_p)
    assert L.mkid_welch_psd_host(None, None, 40, 41, 1, 16, nc.FS, 0, p(out), None) == _lib.MKID_E_ARG
    assert L.mkid_welch_psd_host(p(a), None, 40, 41, 1, 16, nc.FS, 0, None, None) == _lib.MKID_E_ARG
    assert L.mkid_welch_psd_host(p(a), None, 40, 41, 0, 16, nc.FS, 0, p(out), None) == _lib.MKID_E_ARG
    assert np.all(out == -7.0)
