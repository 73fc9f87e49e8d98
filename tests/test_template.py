"""MakeTemplate (a18) and the optimal filter: oracle restatement (CPU) and device parity (GPU).

Input pulses follow the reference's own generator FakeTemplateData (pulses.py:429-481), restated
and extended in tests/template_pulses.py. The CPU tests below also show that the pulse sets of
tests/test_gpu_template.py reach what they claim to reach in the oracle, and that no decision on
them hangs on the last bits of atan2.
"""
import numpy as np
import pytest

import template_pulses as tp
from oracle import template_ref
from template_pulses import fake_pulses


def test_oracle_template_on_fake_pulses():
    I, Q = fake_pulses(300, 1, bad_every=50, big_every=40)
    r = template_ref.make_template(I, Q)
    assert 20.0 < r['pm'] < 28.0                 # atan2(1, 2.25) = 24 deg peak
    assert 0 < r['count'] <= 300 and r['count1'] > 200
    assert abs(r['pstart'] - 1000) < 15 and 0.9 < r['template'].max() <= 1.0 + 1e-12
    assert r['flag'] == 1                        # count < 500
    g = template_ref.optimal_filter(r['template'], r['noise'])
    assert g.shape == (100,) and np.isfinite(g).all()


@pytest.mark.gpu
@pytest.mark.parametrize('n,seed', [(1200, 2), (257, 3)])
def test_device_template_matches_oracle(gpu, n, seed):
    from mkids_sdr_amd import template
    from mkids_sdr_amd.channelizer import Channelizer
    I, Q = fake_pulses(n, seed, bad_every=97, big_every=61)
    ref = template_ref.make_template(I, Q)
    ch = Channelizer(64, max_chunk=1 << 14)
    try:
        got = template.make_template(ch, I, Q)
        assert got['count1'] == ref['count1'] and got['count'] == ref['count']
        assert got['flag'] == ref['flag'] and got['pstart'] == ref['pstart']
        assert abs(got['pm'] - ref['pm']) < 1e-4 and abs(got['pdev'] - ref['pdev']) < 1e-4
        np.testing.assert_allclose(got['template'], ref['template'], rtol=0, atol=2e-5)
        np.testing.assert_allclose(got['noise'], ref['noise'], rtol=2e-4, atol=1e-9 * ref['noise'].max())
        g_ref = template_ref.optimal_filter(ref['template'], ref['noise'])
        g = template.optimal_filter(ch, got['d_template'], got['d_noise'])
        np.testing.assert_allclose(g, g_ref, rtol=0, atol=1e-3 * np.abs(g_ref).max())
        taps, taps12 = template.matched_fir_taps(g)
        assert len(taps12) == 26 and np.abs(taps12).max() <= 2047
        # exactness of the device arithmetic itself, independent of the oracle
        g2 = template.optimal_filter(ch, ref['template'], ref['noise'])
        np.testing.assert_allclose(g2, g_ref, rtol=1e-9, atol=1e-12 * np.abs(g_ref).max())
    finally:
        ch.close()


@pytest.mark.gpu
def test_device_template_no_pulses_is_loud(gpu):
    from mkids_sdr_amd import _lib, template
    from mkids_sdr_amd.channelizer import Channelizer
    I = np.full((20, 2000), 2.0, np.float32)
    Q = np.zeros((20, 2000), np.float32)
    ch = Channelizer(64, max_chunk=1 << 14)
    try:
        with pytest.raises(_lib.MkidError):
            template.make_template(ch, I, Q)
    finally:
        ch.close()


# ---- the pulse sets of tests/test_gpu_template.py, judged on the oracle (CPU) -------------------

def _plain_fake_pulses(n, seed, bad_every=0, big_every=0):
    """fake_pulses as it stood before it learnt categories, rotation and roll_sigma."""
    rng = np.random.default_rng(seed)
    I = np.zeros((n, 2000), np.float32)
    Q = np.zeros((n, 2000), np.float32)
    idx = np.arange(1000, dtype='float32')
    shape = (1.0 - np.exp(-idx / 0.1)) * np.exp(-idx / 65.0)
    for j in range(n):
        i = np.zeros(2000)
        q = np.zeros(2000)
        amp = 10.0 if (big_every and j % big_every == 3) else 1.0
        i[1000:2000] = shape * 0.25 * amp
        q[1000:2000] = shape * amp
        i += 2.0 - rng.normal(size=2000) * .01
        q += rng.normal(size=2000) * .01
        if bad_every and j % bad_every == 5:
            q[1500:] += 0.3
        i = np.roll(i, int((rng.normal() * 10.0) + 0.5))
        q = np.roll(q, int((rng.normal() * 10.0) + 0.5))
        I[j], Q[j] = i, q
    return I, Q


def test_fake_pulses_keeps_its_plain_output():
    """The categories, the rotation and roll_sigma leave what the plain arguments produce alone."""
    for args in ((257, 3, 97, 61), (300, 1, 50, 40), (120, 2, 0, 0)):
        want, got = _plain_fake_pulses(*args), fake_pulses(*args)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


@pytest.mark.parametrize('P,theta', tp.CATEGORY_CASES)
def test_category_sets_hit_every_category(P, theta):
    """Every placed pulse draws the decision its category was built for, in both passes, every
    unplaced pulse is accepted twice, and a rotation changes no decision. Together the sets hold
    every code in both passes (24 pulses are too few for `tall`, see template_pulses.EXPECTED).
    At rest at 168 and 180 deg the unwrap corrects samples of accepted pulses (at 168 the pulse
    crosses pi, at 180 the noise does at about every second sample); at -170 deg positive pulses
    lead away from -pi and the unwrap must leave every sample alone."""
    _, _, ref = tp.case('cat', P, theta)
    d1, d2 = tp.expected_decisions(P)
    assert ref['dec1'].tolist() == d1.tolist() and ref['dec2'].tolist() == d2.tolist()
    assert ref['count1'] == np.count_nonzero(d1 == 0) and ref['count'] == np.count_nonzero(d2 == 0)
    want1 = {tp.A, tp.BAD, tp.LOW, tp.HIGH, tp.PLOC1}
    want2 = {tp.A, tp.BAD, tp.OUTL, tp.PLOC2}
    assert set(d1.tolist()) == want1 and set(d2.tolist()) == want2
    cats = [c for _, c, _, _ in tp.EXPECTED[P]]
    assert ('tall' in cats) == (P >= 99)
    if P == 1003:      # the pulses past the first-pass cap are of three categories
        assert d2[1000:].tolist() == [tp.BAD, tp.OUTL, tp.PLOC2]
    accepted = ref['dec2'] == 0
    if theta in (168, 180):
        assert ref['nwrap'][accepted].max() >= 900
        # every accepted pulse wraps, but for `weak` at 168 deg, which stops short of pi
        assert np.count_nonzero(ref['nwrap'][accepted]) >= np.count_nonzero(accepted) - 1
    else:
        assert ref['nwrap'].max() == 0


@pytest.mark.parametrize('P,rest', tp.PHASE_CASES)
def test_phase_sets_hit_their_categories(P, rest):
    """The production route (phase records -> iq_from_phase): the placed pulses draw their
    decisions, and the noise alone wraps every record (rest = +-3.1 rad, sigma 0.02)."""
    _, _, ref = tp.case('phase', P, rest)
    for j, _, a, b in tp.PHASE_EXPECTED:
        assert ref['dec1'][j] == a and (b is None or ref['dec2'][j] == b)
    placed = [j for j, _, _, _ in tp.PHASE_EXPECTED]
    assert np.count_nonzero(np.delete(ref['dec1'], placed)) == 0
    assert {tp.A, tp.BAD, tp.OUTL} == set(ref['dec2'].tolist())
    assert ref['count'] >= 30 and ref['nwrap'][ref['dec2'] == 0].min() > 0


@pytest.mark.parametrize('kind,P,where', [('cat', P, th) for P, th in tp.CATEGORY_CASES]
                         + [('phase', P, r) for P, r in tp.PHASE_CASES])
def test_decisions_do_not_hang_on_atan2(kind, P, where):
    """The oracle again with its float32 arctan2 output moved by a random -2..+2 ulp per sample
    (tp.JITTER_ULP: the ROCm installation states no error bound for the device atan2f), three
    draws: every decision of both passes stays. This is what makes exact equality of count1 and
    count a fair demand on the device. The same runs set the bars of the sets at rest near +-pi
    (tp.bars: the larger of the project's bar and 4 x the largest deviation from the unjittered
    oracle). Measured deviations (largest of three draws; the project's bars are template 2e-5,
    noise 2e-4 relative, pm and pdev 1e-4):

        set             template   noise rel.   pm        pdev
        24   at 0       7.3e-8     1.4e-7       3.8e-6    6.7e-6
        257  at 0       2.1e-8     3.9e-8       3.8e-6    1.3e-6
        1003 at 0       9.8e-9     2.1e-8       3.8e-6    5.5e-7
        24   at 168     8.4e-7     8.2e-5       3.0e-5    1.1e-5
        257  at 168     2.0e-7     2.7e-5       3.5e-5    4.1e-6
        1003 at 168     9.7e-8     2.2e-5       2.0e-5    1.3e-6
        24   at 180     9.2e-6     6.0e-3       1.4e-4    7.5e-5
        257  at 180     2.0e-6     1.7e-3       2.8e-4    1.2e-5
        24   at -170    8.1e-7     9.3e-5       3.1e-5    2.7e-6
        257  at -170    2.2e-7     2.6e-5       3.0e-5    5.5e-7
        phase +3.1      1.9e-6     2.4e-4       7.6e-5    1.2e-5
        phase -3.1      1.8e-6     3.0e-4       5.7e-5    6.8e-6

    so 4 x the deviation exceeds the project's bar for: the template at 24 pulses at 180 deg
    (3.7e-5); the noise at 24 at 168 and -170 (3.3e-4, 3.7e-4), at 180 deg (2.4e-2 at 24 pulses,
    6.6e-3 at 257) and on the phase route (9.4e-4, 1.2e-3); pm at 24 and 257 at 168, 180 and -170
    (1.2e-4 .. 1.1e-3) and on the phase route (3.0e-4, 2.3e-4); pdev at 24 at 180 (3.0e-4)."""
    _, _, ref = tp.case(kind, P, where)
    for r in tp.jitter_runs(kind, P, where):
        assert r['dec1'].tolist() == ref['dec1'].tolist() and r['dec2'].tolist() == ref['dec2'].tolist()
        assert r['count1'] == ref['count1'] and r['count'] == ref['count']
        assert r['flag'] == ref['flag'] and r['pstart'] == ref['pstart']
    dev = tp.jitter_deviation(kind, P, where)
    bars = tp.bars(kind, P, where)
    print('jitter %s P=%d at %s:' % (kind, P, where), ' '.join('%s %.2e (bar %.2e)' % (k, dev[k], bars[k])
                                                                 for k in tp.BARS))
    if kind == 'cat' and where == 0:       # far from the wraps the project's bars have room to spare
        assert all(4.0 * dev[k] < tp.BARS[k] for k in tp.BARS)


def test_one_good_pulse_raises_in_the_oracle():
    """One good pulse among flat rows, or alone: pass 1 accepts it, pdev = 0, and after the second
    re-reference its peak is off pm by float32 rounding: pass 2 accepts nothing."""
    for P in (24, 1):
        I, Q = tp.one_good_among_flat(P)
        with pytest.raises(ValueError, match='second pass'):
            template_ref.make_template(I, Q)
    with pytest.raises(ValueError, match='first pass'):
        template_ref.make_template(np.full((20, 2000), 2.0, np.float32), np.zeros((20, 2000), np.float32))
    rec, ready = tp.filter_bank_records()
    from mkids_sdr_amd import template
    with pytest.raises(ValueError, match='second pass'):
        template_ref.make_template(*template.iq_from_phase(rec[0, :ready[0]]))
    assert template_ref.make_template(*template.iq_from_phase(rec[1, :ready[1]]))['count'] >= 10


def _old_optimal_filter(template, noise, ncoeff=100, pre=100):
    """oracle.template_ref.optimal_filter before it defined the window that leaves the record."""
    t = np.asarray(template, np.float64)
    J = np.asarray(noise, np.float64)
    pstart = int(np.argmax(t))
    s = np.deg2rad(t[pstart - pre:pstart - pre + 800])
    H = np.fft.fft(s) / J
    H[0] = 0.0
    g = np.real(np.fft.ifft(H))
    g /= np.dot(g, s)
    return g[pre - 10:pre - 10 + ncoeff].copy()


@pytest.mark.parametrize('peak,pre,ncoeff', tp.FILTER_WINDOW_CASES)
def test_optimal_filter_zero_padding(peak, pre, ncoeff):
    """A window that leaves the record reads zeros outside [0, 2000), and weights at m >= 800 are
    zero: against the definition evaluated directly in float64 (tp.direct_filter, a plain DFT).
    A window inside the record gives bit for bit what the earlier code gave."""
    t, J = tp.filter_inputs(peak)
    g = template_ref.optimal_filter(t, J, ncoeff=ncoeff, pre=pre)
    want = tp.direct_filter(t, J, pre, ncoeff)
    assert g.shape == (ncoeff,)
    np.testing.assert_allclose(g, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    inside = min(max(810 - pre, 0), ncoeff)       # weights g[m] with m = pre - 10 + i < 800
    assert not g[inside:].any() and (inside == 0 or g[:inside].any())
    p0 = int(np.argmax(t)) - pre
    if p0 >= 0 and p0 + 800 <= 2000 and pre - 10 + ncoeff <= 800:
        assert np.array_equal(g, _old_optimal_filter(t, J, ncoeff=ncoeff, pre=pre))
    else:
        assert p0 < 0 or p0 + 800 > 2000 or ncoeff > 810 - pre
