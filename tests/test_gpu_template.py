"""Device MakeTemplate and optimal filter (k_template.hip) against oracle/template_ref.py where the
kernel can go wrong: phase wraps (sets at rest near +-pi), every accept / reject branch of both
passes at chosen pulses, set sizes around the branch points (1, 24, 99..101, 257, 1003), the
filter's window edges, and the failures that must be loud.

The sets, what each reaches in the oracle and the bars come from tests/template_pulses.py; the CPU
tests of tests/test_template.py show that the sets reach what they claim and that no decision on
them hangs on the last bits of atan2, which is what makes exact counts a fair demand here.
"""
import numpy as np
import pytest

import template_pulses as tp
from oracle import template_ref

pytestmark = pytest.mark.gpu


@pytest.fixture
def ch(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    c = Channelizer(64, max_chunk=1 << 14)
    yield c
    c.close()


def _check(got, ref, bars):
    dev = tp.deviations(ref, got)
    print('device vs oracle:', ' '.join('%s %.2e (bar %.2e)' % (k, dev[k], bars[k]) for k in tp.BARS),
          'count1 %g count %g' % (got['count1'], got['count']))
    assert got['count1'] == ref['count1'] and got['count'] == ref['count']
    assert got['flag'] == ref['flag'] and got['pstart'] == ref['pstart']
    assert abs(got['pm'] - ref['pm']) < bars['pm'] and abs(got['pdev'] - ref['pdev']) < bars['pdev']
    np.testing.assert_allclose(got['template'], ref['template'], rtol=0, atol=bars['template'])
    np.testing.assert_allclose(got['noise'], ref['noise'], rtol=bars['noise'], atol=1e-9 * ref['noise'].max())


@pytest.mark.parametrize('P,theta', tp.CATEGORY_CASES)
def test_device_template_categories(ch, P, theta):
    """The category mix (every accept / reject branch of both passes at placed pulses) at P pulses,
    at rest at theta degrees: exact count1, count, flag and pstart; template, noise, pm and pdev
    within the project's bars at theta = 0 and within tp.bars (jitter-derived, see
    tests/test_template.py::test_decisions_do_not_hang_on_atan2) at rest near +-pi. At 24 pulses
    one wrong decision moves the template by 4 %."""
    from mkids_sdr_amd import template
    I, Q, ref = tp.case('cat', P, theta)
    _check(template.make_template(ch, I.copy(), Q.copy()), ref, tp.bars('cat', P, theta))


@pytest.mark.parametrize('P,rest', tp.PHASE_CASES)
def test_device_template_from_phase_records(ch, P, rest):
    """The production route: phase records at rest at +-3.1 rad, where the noise alone wraps,
    through template.iq_from_phase."""
    from mkids_sdr_amd import template
    I, Q, ref = tp.case('phase', P, rest)
    _check(template.make_template(ch, I.copy(), Q.copy()), ref, tp.bars('phase', P, rest))


@pytest.mark.parametrize('P', [24, 1])
def test_device_template_empty_second_pass_is_loud(ch, P):
    """One good pulse among flat rows, or alone: pass 1 accepts it and pass 2 accepts nothing (the
    oracle raises on this input, tests/test_template.py). The device has to say MKID_E_STATE; it
    used to return MKID_OK with a template and a noise PSD of NaN (0 / 0), count = 0, pstart = 0."""
    from mkids_sdr_amd import _lib, template
    I, Q = tp.one_good_among_flat(P)
    with pytest.raises(_lib.MkidError) as e:
        r = template.make_template(ch, I, Q)
        print('returned: count1 %g count %g pstart %d, NaN in template: %s' % (
            r['count1'], r['count'], r['pstart'], bool(np.isnan(r['template']).any())))
    assert e.value.code == _lib.MKID_E_STATE


def test_device_filters_from_bank_takes_the_fallback(ch):
    """A hand-built bank on the device: a channel with enough records of which one is a pulse, a
    healthy channel and a channel below min_records. The first and the third take the fallback
    row; no NaN reaches the filter table."""
    import torch
    from mkids_sdr_amd import template
    rec, ready = tp.filter_bank_records()
    bank = (torch.from_numpy(rec).cuda(), torch.zeros(rec.shape[:2], dtype=torch.int64, device='cuda'),
            torch.from_numpy(np.stack((ready, np.zeros_like(ready)), axis=1)).cuda())
    fallback = np.arange(100, dtype=np.float32)
    got = template.filters_from_bank(ch, bank, ncoeff=100, pre=100, min_records=20, fallback=fallback)
    assert got['used'].tolist() == [False, True, False]
    assert got['flag'].tolist()[::2] == [-1, -1] and got['pstart'].tolist()[::2] == [-1, -1]
    assert np.array_equal(got['coeff'][0], fallback) and np.array_equal(got['coeff'][2], fallback)
    assert np.isfinite(got['coeff']).all() and np.abs(got['coeff'][1]).max() > 0
    ref = template_ref.make_template(*template.iq_from_phase(rec[1]))
    assert got['count'][1] == ref['count'] and got['pstart'][1] == ref['pstart'] and got['flag'][1] == ref['flag']


def test_device_template_leaves_inputs_alone_and_repeats(ch):
    """include/mkidgpu.h: the pulses are "not modified" (the kernels read them where they lie and
    write nothing back), and k_template.hip accumulates in pulse order: two runs give the same bits.
    Nothing beyond npulses rows is read: the same 24 pulses at the head of [27][2000] tensors whose
    last three rows are NaN give the same bits again and leave all 27 rows as they were."""
    import torch
    from mkids_sdr_amd import template
    I, Q, _ = tp.case('cat', 24, 180)
    dI, dQ = torch.from_numpy(I.copy()).cuda(), torch.from_numpy(Q.copy()).cuda()
    a = template.make_template(ch, dI, dQ)
    assert np.array_equal(dI.cpu().numpy(), I) and np.array_equal(dQ.cpu().numpy(), Q)
    b = template.make_template(ch, dI, dQ)
    assert np.array_equal(a['template'], b['template']) and np.array_equal(a['noise'], b['noise'])
    assert (a['count1'], a['count'], a['pm'], a['pdev']) == (b['count1'], b['count'], b['pm'], b['pdev'])
    nan3 = np.full((3, 2000), np.nan, np.float32)
    wI, wQ = (torch.from_numpy(np.concatenate((x, nan3))).cuda() for x in (I, Q))
    before = [w.view(dtype=torch.int32).clone() for w in (wI, wQ)]
    assert wI[:24].is_contiguous() and wI[:24].data_ptr() == wI.data_ptr()   # npulses = 24 of the 27 rows
    c = template.make_template(ch, wI[:24], wQ[:24])
    for k in ('template', 'noise'):
        assert np.array_equal(a[k].view(np.uint64), c[k].view(np.uint64)), k
    for k in ('count', 'count1', 'pm', 'pdev', 'flag', 'pstart'):
        assert a[k] == c[k], k
    assert torch.equal(wI.view(dtype=torch.int32), before[0]) and torch.equal(wQ.view(dtype=torch.int32), before[1])


@pytest.mark.parametrize('peak,pre,ncoeff', tp.FILTER_WINDOW_CASES)
def test_device_optimal_filter_windows(ch, peak, pre, ncoeff):
    """The filter on the oracle's template and noise at the window's edges (a window that starts
    before the record or ends after it reads zeros there; weights past g[799] are zero), at the
    bar of exact arithmetic."""
    from mkids_sdr_amd import template
    t, J = (a.copy() for a in tp.filter_inputs(peak))
    want = template_ref.optimal_filter(t, J, ncoeff=ncoeff, pre=pre)
    g = template.optimal_filter(ch, t, J, pre=pre, ncoeff=ncoeff)
    np.testing.assert_allclose(g, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    inside = min(max(810 - pre, 0), ncoeff)
    assert not g[inside:].any() and (inside == 0 or g[:inside].any())
    if (pre, ncoeff) == (100, 800):
        assert inside == 710 and np.array_equal(g[-90:], np.zeros(90))


def test_device_optimal_filter_coloured_noise(ch):
    from mkids_sdr_amd import template
    t, J = (a.copy() for a in tp.coloured_filter_inputs())
    assert J.max() / J.min() > 100
    want = template_ref.optimal_filter(t, J)
    g = template.optimal_filter(ch, t, J)
    np.testing.assert_allclose(g, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    white = template_ref.optimal_filter(t, np.ones(800))
    assert np.abs(want / np.abs(want).max() - white / np.abs(white).max()).max() > 0.1   # J matters


def test_device_template_refuses_bad_requests(ch):
    """Out-of-range requests are refused on the host, before any launch."""
    from mkids_sdr_amd import _lib, template
    t, J = (a.copy() for a in tp.filter_inputs(None))
    for pre, ncoeff in ((9, 100), (2001, 100), (100, 0), (100, 801)):
        with pytest.raises(_lib.MkidError) as e:
            template.optimal_filter(ch, t, J, pre=pre, ncoeff=ncoeff)
        assert e.value.code == _lib.MKID_E_ARG
    with pytest.raises(_lib.MkidError) as e:
        template.make_template(ch, np.zeros((0, 2000), np.float32), np.zeros((0, 2000), np.float32))
    assert e.value.code == _lib.MKID_E_ARG
    with pytest.raises(ValueError):
        template.make_template(ch, np.zeros((3, 1999), np.float32), np.zeros((3, 1999), np.float32))
