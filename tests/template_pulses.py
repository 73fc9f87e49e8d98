"""Pulse sets for MakeTemplate (oracle/template_ref.py, k_template.hip) — TEST INFRASTRUCTURE.

`fake_pulses` follows the reference's own generator FakeTemplateData (pulses.py:429-481): I = 2 -
noise + 0.25 s(t), Q = s(t) + noise, s = (1 - e^{-t/0.1}) e^{-t/65} after sample 1000, I and Q
rolled independently by round(N(0,1)*10) (as the reference does), float32 rows of 2000. A good
pulse peaks at atan2(1, 2.25) = 24 deg.

On top of that, `place` puts a pulse of a chosen category at a chosen index, and `theta` rotates
the whole set about the origin, so that the resting phase sits at theta and the unwrap has work to
do. The categories, with the decision each is built to draw from the oracle (dec1 = first pass,
dec2 = second pass, codes of template_ref):

  good     amplitude 1                                              accepted in both passes
  step     good + a 0.3 step in Q from sample 1500, not rolled      bad baseline in both
  weak     amplitude 0.2 (peak 5.4 deg)                             pass 1: peak < 15
  wide     amplitude 3, I gain -1.4 (I = -2.2, Q = 3: 126 deg; the
           phasor passes the Q axis)                                pass 1: peak > 120
  late35   both rolled by +35                                       pass 1: ploc 1036 out of 980..1020;
                                                                    pass 2: |ploc| > 30
  early60  both rolled by -60                                       pass 2: |ploc| > 30
  late24   both rolled by +24, fall time 30 instead of 65           pass 1: ploc 1025 out; pass 2: |ploc| <= 30
  tall     amplitude 3, I gain -0.75 (I = -0.25, Q = 3: 95 deg)     pass 1: accepted; pass 2: outside
                                                                    pm +- 4 pdev (needs enough peaks,
                                                                    see EXPECTED)

The two passes do not measure location alike. Pass 1 takes the first index of max(P3[980:1050]),
one sample after the onset. Pass 2 takes argmax(convolve(tP[900:1500], P3)) - 1160, and a
convolution (not a correlation) of two pulses that rise at once and fall with 65 samples peaks
about 65 samples after the sum of the onsets: a pulse displaced by d gets ploc2 = d + 10 or so
(measured: 2..18 for the unplaced pulses, which are rolled by up to +-9). Hence:
  - no plain displaced pulse is rejected by pass 1 and accepted by pass 2 (ploc1 > 1020 needs
    d >= 20, ploc2 <= 30 needs d <= 20): `late24` falls faster, which pulls the peak of its
    convolution back by about 22 samples, to ploc2 = 12;
  - a pulse displaced to the left cannot be rejected by pass 1 for its location: the search
    window starts at 980, so ploc1 >= 980 always (short of an exact tie of two doubles), and
    the reference finds the decaying tail there. At -60 the tail is 13 deg and pass 1 rejects
    the pulse as too low; pass 2 finds ploc2 = -47.

What pass 2 makes of `weak`, `wide` and `late24` (whose "peak" P3[1000 + ploc2] is read before
its onset and is about 0) depends on pdev and so on the rest of the set; the expected codes per
set are in EXPECTED below, and tests/test_template.py asserts them on the oracle. Placed pulses
are rolled only as their category says; the unplaced (good) pulses of a category set are rolled by
round(N(0,1) * roll_sigma) with roll_sigma = 3, so that none of them meets a threshold by accident.
"""
import functools

import numpy as np

from oracle import template_ref as tr

#            amp, I gain, roll, step, fall time
CATEGORIES = {
    'good':    (1.0, 0.25, None, False, 65.0),
    'step':    (1.0, 0.25, 0, True, 65.0),
    'weak':    (0.2, 0.25, 0, False, 65.0),
    'wide':    (3.0, -1.4, 0, False, 65.0),
    'late35':  (1.0, 0.25, 35, False, 65.0),
    'early60': (1.0, 0.25, -60, False, 65.0),
    'late24':  (1.0, 0.25, 24, False, 30.0),
    'tall':    (3.0, -0.75, 0, False, 65.0),
}


def fake_pulses(n, seed, bad_every=0, big_every=0, place=None, theta=0.0, roll_sigma=10.0):
    """place: {index: category}; theta in degrees (float64 rotation, then the float32 cast)."""
    rng = np.random.default_rng(seed)
    I = np.zeros((n, 2000), np.float32)
    Q = np.zeros((n, 2000), np.float32)
    idx = np.arange(1000, dtype='float32')
    shape = (1.0 - np.exp(-idx / 0.1)) * np.exp(-idx / 65.0)
    place = place or {}
    c, s = np.cos(np.deg2rad(float(theta))), np.sin(np.deg2rad(float(theta)))
    for j in range(n):
        i = np.zeros(2000)
        q = np.zeros(2000)
        amp = 10.0 if (big_every and j % big_every == 3) else 1.0
        gain, roll, step, sh = 0.25, None, bool(bad_every and j % bad_every == 5), shape
        if j in place:
            amp, gain, roll, step, fall = CATEGORIES[place[j]]
            sh = (1.0 - np.exp(-idx / 0.1)) * np.exp(-idx / np.float32(fall))
        i[1000:2000] = sh * gain * amp
        q[1000:2000] = sh * amp
        i += 2.0 - rng.normal(size=2000) * .01
        q += rng.normal(size=2000) * .01
        if step:                                  # baseline step: fails the baseline check
            q[1500:] += 0.3
        ri = int((rng.normal() * roll_sigma) + 0.5)
        rq = int((rng.normal() * roll_sigma) + 0.5)
        if roll is not None:
            ri = rq = roll
        i = np.roll(i, ri)
        q = np.roll(q, rq)
        if theta:
            i, q = i * c - q * s, i * s + q * c
        I[j], Q[j] = i, q
    return I, Q


A, BAD, LOW, HIGH, PLOC1, OUTL, PLOC2 = (tr.ACCEPT, tr.BAD_BASELINE, tr.PEAK_LOW, tr.PEAK_HIGH, tr.PLOC1_OUT,
                                         tr.PEAK_OUTLIER, tr.PLOC2_OUT)

# {P: [(index, category, dec1 or None past the first-pass cap, dec2)]}; every other pulse is good and
# accepted twice. pdev is the std of all first-pass peaks > 15 deg, the wide and the tall one
# included, so it shrinks as P grows: with one peak at distance W from the median and one at D
# among n, 4 pdev ~ 4 sqrt((W^2 + D^2) / n).
#   P = 24   n = 21, W = 102: 4 pdev ~ 89, and no peak in 15..120 can be an outlier next to `wide`
#            (it would need D > 4 W / sqrt(n - 16)); the set leaves `tall` out. `wide` is the pass-2
#            outlier (126 > 24 + 89) and `weak` (5.4 > 24 - 89) is accepted in pass 2.
#   P >= 99  n >= 95, W = 102, D = 71: 4 pdev <= 51: `tall` and `wide` are outliers, `weak`
#            (24 - 5.4 = 18.6 < 4 pdev at every P here) is accepted in pass 2.
EXPECTED = {
    24: [(2, 'step', BAD, BAD), (5, 'weak', LOW, A), (9, 'wide', HIGH, OUTL), (12, 'late35', PLOC1, PLOC2),
         (15, 'early60', LOW, PLOC2), (19, 'late24', PLOC1, A)],
}
for _P in (99, 100, 101, 257):
    EXPECTED[_P] = [(2, 'step', BAD, BAD), (5, 'weak', LOW, A), (9, 'wide', HIGH, OUTL),
                    (12, 'late35', PLOC1, PLOC2), (15, 'early60', LOW, PLOC2), (19, 'late24', PLOC1, A),
                    (23, 'tall', A, OUTL), (_P - 1, 'late35', PLOC1, PLOC2), (_P - 2, 'step', BAD, BAD)]
# the last three pulses lie past the first-pass cap of 1000 and are of three categories
# (n = 995: 4 pdev = 16.3, so `weak` and the near-zero "peak" of `late24` are outliers here)
EXPECTED[1003] = [(2, 'step', BAD, BAD), (5, 'weak', LOW, OUTL), (9, 'wide', HIGH, OUTL),
                  (12, 'late35', PLOC1, PLOC2), (15, 'early60', LOW, PLOC2), (19, 'late24', PLOC1, OUTL),
                  (23, 'tall', A, OUTL)] + [(999, 'late35', PLOC1, PLOC2), (1000, 'step', None, BAD),
                                      (1001, 'tall', None, OUTL), (1002, 'late35', None, PLOC2)]


def category_set(P, theta=0.0):
    """(I, Q) of the category mix at P pulses (EXPECTED[P]) at resting phase theta degrees."""
    place = {j: cat for j, cat, _, _ in EXPECTED[P]}
    return fake_pulses(P, 100 + P, place=place, theta=theta, roll_sigma=3.0)


def expected_decisions(P):
    """dec1 [min(P, 1000)], dec2 [P] that category_set(P, any theta) must draw from the oracle."""
    d1 = np.zeros(min(P, 1000), np.int8)
    d2 = np.zeros(P, np.int8)
    for j, _, a, b in EXPECTED[P]:
        if a is not None:
            d1[j] = a
        d2[j] = b
    return d1, d2


# phase-record route (template.iq_from_phase): negative-going pulses of 0.4 rad (23 deg) on a
# resting phase `rest` (rad), noise sigma 0.02, wrapped into (-pi, pi] as a phase record is.
# At rest = +3.1 the noise alone crosses pi at about every 50th sample; at rest = -3.1 the pulse
# crosses it as well. Good pulses are rolled by -3..3. With pdev near 1.2 deg (the noise) pass 2
# rejects about a third of the good pulses as outliers: it reads the "peak" at 1000 + ploc2, off the
# true peak, and so it does with the displaced ones before it looks at their location. `step` is here an offset of the first 100 samples (a step at 1500 is absorbed by the
# fit at this noise).
PHASE_EXPECTED = [(3, 'step', BAD, BAD), (7, 'weak', LOW, None), (11, 'late35', PLOC1, OUTL),
                  (13, 'late24', PLOC1, OUTL)]


def phase_records(P, seed, rest):
    rng = np.random.default_rng(seed)
    t = np.arange(1000, dtype=np.float64)
    place = {j: cat for j, cat, _, _ in PHASE_EXPECTED}
    rec = np.zeros((P, 2000), np.float32)
    for j in range(P):
        amp, _, roll, step, fall = CATEGORIES[place.get(j, 'good')]
        ph = np.zeros(2000)
        ph[1000:] = -0.4 * amp * (1.0 - np.exp(-t / 0.1)) * np.exp(-t / fall)
        ph += rng.normal(size=2000) * 0.02
        if step:                                 # the first 100 samples sit 0.1 rad (5 sigma) off
            ph[:100] -= 0.1
        r = int(rng.integers(-3, 4))
        ph = np.roll(ph, r if roll is None else roll) + rest
        rec[j] = np.angle(np.exp(1j * ph))       # into (-pi, pi]
    return rec


def one_good_among_flat(P=24, seed=9):
    """One good pulse (row 0) followed by flat noisy rows: the first pass accepts row 0 alone, pdev
    is 0, and the second re-reference moves its peak off pm by float32 rounding, so the second pass
    accepts nothing. P = 1 is the good pulse alone."""
    I, Q = fake_pulses(1, seed, roll_sigma=0.0)
    rng = np.random.default_rng(seed + 1)
    fI = (2.0 - rng.normal(size=(P - 1, 2000)) * .01).astype(np.float32)
    fQ = (rng.normal(size=(P - 1, 2000)) * .01).astype(np.float32)
    return np.concatenate((I, fI)), np.concatenate((Q, fQ))


def ulp_jitter(k, seed):
    """phase_hook for template_ref.make_template: every float32 sample moved by a random whole
    number of ulps in -k..+k."""
    rng = np.random.default_rng(seed)

    def hook(p):
        p = np.asarray(p, np.float32)
        n = rng.integers(-k, k + 1, size=p.shape)
        step = np.spacing(np.abs(p)).astype(np.float32)
        return (p + n.astype(np.float32) * step).astype(np.float32)
    return hook


# ---- the sets the GPU tests run, their oracle results and their bars ----------------------------

CATEGORY_CASES = ([(P, 0) for P in (24, 99, 100, 101, 257)]
                  + [(P, th) for P in (257, 24) for th in (168, 180, -170)]
                  + [(1003, 0), (1003, 168)])
PHASE_CASES = [(64, 3.1), (64, -3.1)]

JITTER_ULP = 2      # no document or header of the ROCm installation states the error of the device
JITTER_DRAWS = 3    # atan2f, so the amplitude is 2 ulp
# the project's bars (tests/test_template.py::test_device_template_matches_oracle)
BARS = dict(template=2e-5, noise=2e-4, pm=1e-4, pdev=1e-4)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(kind, P, where):
    """(I, Q, oracle result) of one set, computed once and read-only: kind 'cat' is
    category_set(P, theta = where), kind 'phase' is phase_records(P, rest = where) through
    template.iq_from_phase."""
    if kind == 'cat':
        I, Q = category_set(P, where)
    else:
        from mkids_sdr_amd import template
        I, Q = template.iq_from_phase(phase_records(P, 5, where))
    _frozen(I, Q)
    ref = tr.make_template(I, Q)
    _frozen(*(v for v in ref.values() if isinstance(v, np.ndarray)))
    return I, Q, ref


@functools.lru_cache(maxsize=None)
def jitter_runs(kind, P, where):
    """The oracle on the same set with its float32 arctan2 output moved by -k..+k ulp per sample,
    JITTER_DRAWS times."""
    I, Q, _ = case(kind, P, where)
    return tuple(tr.make_template(I, Q, phase_hook=ulp_jitter(JITTER_ULP, 1000 + d)) for d in range(JITTER_DRAWS))


def deviations(ref, other):
    return dict(template=float(np.abs(other['template'] - ref['template']).max()),
                noise=float((np.abs(other['noise'] - ref['noise']) / ref['noise']).max()),
                pm=abs(other['pm'] - ref['pm']), pdev=abs(other['pdev'] - ref['pdev']))


def jitter_deviation(kind, P, where):
    _, _, ref = case(kind, P, where)
    devs = [deviations(ref, r) for r in jitter_runs(kind, P, where)]
    return {k: max(d[k] for d in devs) for k in BARS}


def bars(kind, P, where):
    """Bars of a device result against the oracle: the project's for a set at rest at phase 0; for
    a set at rest near +-pi, where float32 rounding of the phase is amplified by the wraps, the
    larger of the project's and 4 x the largest deviation of the jittered oracle from the oracle
    (three random draws underestimate the worst one)."""
    if kind == 'cat' and where == 0:
        return dict(BARS)
    dev = jitter_deviation(kind, P, where)
    return {k: max(BARS[k], 4.0 * dev[k]) for k in BARS}


# ---- optimal filter: window cases and the definition evaluated directly -------------------------

# (template peak rolled to this sample, or None for the template as it is (peak near 992), pre, ncoeff)
FILTER_WINDOW_CASES = [(None, 100, 100),    # window inside the record
                       (None, 10, 100), (None, 300, 1),
                       (None, 100, 800),    # weights 710.. are g[800..]: zero
                       (None, 1000, 100),   # window starts at -8; every weight asked for is past g[799]
                       (50, 100, 100),      # window starts at -50
                       (1500, 100, 100)]    # window ends at 2200


@functools.lru_cache(maxsize=None)
def filter_inputs(peak=None):
    """(template, noise) of the 257-pulse category set from the oracle, the template rolled so
    that it peaks at `peak`."""
    _, _, ref = case('cat', 257, 0)
    t = ref['template']
    if peak is not None:
        t = np.roll(t, peak - int(np.argmax(t)))
    return _frozen(t.copy(), ref['noise'].copy())


@functools.lru_cache(maxsize=None)
def coloured_filter_inputs():
    """A synthetic template (the generator's pulse shape at sample 1000) and a clearly coloured
    noise PSD: 1/f plus a floor, symmetric in frequency like the PSD of a real record."""
    idx = np.arange(1000, dtype=np.float64)
    t = np.zeros(2000)
    t[1000:] = (1.0 - np.exp(-idx / 0.1)) * np.exp(-idx / 65.0)
    f = np.abs(np.fft.fftfreq(800)) * 800.0
    return _frozen(t, 1e-3 / (f + 1.0) + 2e-6)


def direct_filter(template, noise, pre, ncoeff):
    """mkid_optimal_filter's definition (include/mkidgpu.h) term by term in float64, with a plain
    800 x 800 DFT matrix instead of an FFT."""
    t = np.asarray(template, np.float64)
    p0 = int(np.argmax(t)) - pre
    s = np.array([np.deg2rad(t[p0 + n]) if 0 <= p0 + n < 2000 else 0.0 for n in range(800)])
    n = np.arange(800)
    W = np.exp(-2j * np.pi * ((n[:, None] * n[None, :]) % 800) / 800.0)
    H = (W @ s) / np.asarray(noise, np.float64)
    H[0] = 0.0
    g = np.real(np.conj(W) @ H) / 800.0
    g /= np.dot(g, s)
    return np.array([g[pre - 10 + i] if pre - 10 + i < 800 else 0.0 for i in range(ncoeff)])


# ---- a hand-built capture bank for template.filters_from_bank -----------------------------------

def filter_bank_records(R=24):
    """(records [3][R][2000] float32 phase, ready [3]): channel 0 holds R records of which only the
    first is a pulse (make_template finds no pulse in pass 2), channel 1 a healthy set, channel 2
    five records (below min_records = 20)."""
    rng = np.random.default_rng(31)
    t = np.arange(1000, dtype=np.float64)
    rec = np.zeros((3, R, 2000), np.float32)
    flat = rng.normal(size=(R, 2000)) * 0.005
    flat[0, 1000:] -= 0.4 * (1.0 - np.exp(-t / 0.1)) * np.exp(-t / 65.0)
    rec[0] = flat
    rec[1] = phase_records(R, 6, 0.5)
    rec[2, :5] = phase_records(5, 7, 0.5)
    return rec, np.array([R, R, 5], np.int32)
