"""Laser lines, energy calibration, the energy cube and the quick-look through the host twins
(mkid_spectrum_lines_host, mkid_energy_cube_host: the loops of csrc/wavecal_common.h, no device)
against the restatements of tests/wavecal_cases.py. Integers and the cube compare exactly; the float
part compares against bars derived per fit (wavecal_cases' docstring), of which the host twin must
stay within a tenth.

Recorded here (x86-64, glibc): the host twin's float outputs are bit-identical to the restatement
over the whole case table (largest ratio to the bar 0), the largest derived bar of a line centre for
fit_half = 12 in the recovery set is 1.4e-9 bins with cond(A) <= 3.4e3, and the recovery figures of
seed 20261 are centre error / (sigma / sqrt N) std 1.56, max 4.84, sigma error mean +0.9 %, max 5.2 %.
"""
import math
import struct

import numpy as np
import pytest

import observe_cases as oc
import wavecal_cases as wc
from mkids_sdr_amd import _lib, quicklook, wavecal

_SEEN = {}


@pytest.mark.parametrize('nbins', wc.NBINS)
def test_case_table(nbins):
    """Integer outputs bit-identical to the restatement, floats within a tenth of the derived bar,
    for every shape and every (P, w, g) of the table."""
    rows = wc.rows_for(nbins)
    sp = wc.spectra_of([r for _, r in rows], nbins)
    before = sp.copy()
    status, worst = set(), 0.0
    for P, w, g, min_sep, min_peak, E in wc.param_table(nbins):
        rc, lines, cal, cal_f = wc.lines_host(sp, 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
        assert rc == 0
        for i, (name, _) in enumerate(rows):
            ref = wc.lines_ref(sp[i, 1:nbins + 1], 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
            wc.check_ints(lines[i], cal[i], ref)
            worst = max(worst, wc.float_ratio(lines[i], cal[i], cal_f[i], ref))
            status.add(int(cal[i]['status']))
            if name == 'equal_peaks' and nbins >= 64 and P == 1 and w == 0:
                assert lines[i][0]['bin'] == nbins // 4            # the lower of two equal peaks
            if name == 'plateaus' and nbins >= 64 and P >= 1 and w == 0:
                assert nbins // 3 in [int(b) for b in lines[i]['bin']]   # a plateau's lowest bin
            if name == 'negative_int32' and w == 64 and nbins >= 257:
                assert lines[i]['peak_s'].max() > 2 ** 40              # int64 sums
    print('nbins %d: largest ratio to the bar %.3g' % (nbins, worst))
    assert worst <= 0.1
    assert np.array_equal(sp, before)
    _SEEN[nbins] = status


def test_every_status_bit_is_reached():
    seen = set()
    for nbins in (64, 257):
        if nbins not in _SEEN:
            test_case_table(nbins)
        seen |= _SEEN[nbins]
    bits = [_lib.CAL_FEW_LINES, _lib.CAL_FIT_FAILED, _lib.CAL_FIT_FAILED << 1, _lib.CAL_FIT_FAILED << 2, _lib.CAL_BAD_SLOPE]
    assert 0 in seen
    for b in bits:
        assert any(s & b for s in seen), b


def test_selection_rules():
    """Peaks closer than min_sep give way to the larger; peaks at bin 0 and nbins - 1 are lines."""
    nbins = 64
    r = np.zeros(nbins, np.int64)
    r[[30, 32, 34]] = [90, 80, 70]
    r[[0, 63]] = [60, 61]
    sp = wc.spectra_of([r], nbins)
    bins = lambda min_sep, P=3: [int(b) for b in wc.lines_host(sp, 0, 1, nbins, wc.ENERGIES[P], 0, min_sep, 1, 2)[1][0]['bin']]
    assert bins(1) == [30, 32, 34]
    assert bins(3) == [30, 34, 63]      # 32 is closer than 3 to 30, 34 is not
    assert bins(5) == [0, 30, 63]
    assert bins(64, 2) == [30, -1]      # nothing else is far enough: one line found
    rc, lines, cal, _ = wc.lines_host(sp, 0, 1, nbins, wc.ENERGIES[2], 0, 64, 1, 2)
    assert cal[0]['n_found'] == 1 and cal[0]['status'] & _lib.CAL_FEW_LINES


# ---- does it recover lines? ------------------------------------------------------------------------
SEED, NCH, NB, SIG, NPH = 20261, 300, 512, 8.0, 20000
PARAMS = dict(w=2, min_sep=32, min_peak=10, g=12)


@pytest.fixture(scope='module')
def recovery():
    rng = np.random.default_rng(SEED)
    centres = np.array([120.0, 260.0, 400.0])[None, :] + rng.uniform(-10, 10, (NCH, 3))
    rows = []
    for c in range(NCH):
        n = rng.poisson(10.0, NB).astype(np.int64)
        for p in range(3):
            x = rng.normal(centres[c, p], SIG, NPH)
            n += np.histogram(x, bins=NB, range=(0, NB))[0]
        rows.append(n)
    sp = wc.spectra_of(rows, NB)
    rc, lines, cal, cal_f = wc.lines_host(sp, 0.0, 1.0, NB, wc.ENERGIES[3], PARAMS['w'], PARAMS['min_sep'],
                                          PARAMS['min_peak'], PARAMS['g'])
    assert rc == 0
    return dict(centres=centres, sp=sp, lines=lines, cal=cal, cal_f=cal_f)


def test_recovers_lines(recovery):
    lines, cal = recovery['lines'], recovery['cal']
    assert np.all(cal['n_found'] == 3) and np.all(cal['status'] == 0)
    z = (lines['mu'] - recovery['centres']) / (SIG / math.sqrt(NPH))
    ds = lines['sigma'] / SIG - 1
    print('centre error / (sigma / sqrt N): std %.3f max %.3f; sigma error mean %+.4f max %.4f'
          % (z.std(), np.abs(z).max(), ds.mean(), np.abs(ds).max()))
    assert z.std() <= 2 and np.abs(z).max() <= 8 and np.abs(ds).max() <= 0.15


def test_fit_is_the_weighted_least_squares_parabola(recovery):
    """The restatement shares its written-out solution with the code, so the solution itself is
    checked against numpy's weighted polyfit (QR on the scaled Vandermonde matrix; its weights
    multiply the residuals, so w = n gives W = n^2). Both solve a system of condition <= 1e4 in
    float64: agreement to 1e-9 relative in centre offset and width is far inside that, and far
    outside any slip in a formula."""
    g = PARAMS['g']
    for c in range(0, NCH, 20):
        n = wc.counts_of(recovery['sp'][c, 1:NB + 1])
        for f in recovery['lines'][c]:
            m = int(f['bin'])
            b = np.arange(m - g, m + g + 1)
            a2, a1, a0 = np.polyfit((b - m).astype(float), np.log(n[b]), 2, w=n[b].astype(float))
            assert abs((f['mu'] - m - 0.5) - (-a1 / (2 * a2))) <= 1e-9 * g
            assert abs(f['sigma'] / math.sqrt(-1 / (2 * a2)) - 1) <= 1e-9
            assert abs(f['amp'] / math.exp(a0 - a1 * a1 / (4 * a2)) - 1) <= 1e-9


def test_recovery_bars_are_small(recovery):
    """The derived bar of a line centre with fit_half = 12: far below 1e-8 bins (a larger one would
    mean a wrong derivation), and the host twin inside a tenth of every bar."""
    worst, bar, cond = 0.0, 0.0, 0.0
    for c in range(0, NCH, 15):
        ref = wc.lines_ref(recovery['sp'][c, 1:NB + 1], 0.0, 1.0, NB, wc.ENERGIES[3], PARAMS['w'], PARAMS['min_sep'],
                           PARAMS['min_peak'], PARAMS['g'])
        wc.check_ints(recovery['lines'][c], recovery['cal'][c], ref)
        worst = max(worst, wc.float_ratio(recovery['lines'][c], recovery['cal'][c], recovery['cal_f'][c], ref))
        bar = max(bar, max(f['dmu_x'] for f in ref['lines']))
        cond = max(cond, max(f['cond'] for f in ref['lines']))
    print('largest centre bar %.3g bins, cond(A) <= %.3g, largest ratio %.3g' % (bar, cond, worst))
    assert 0 < bar < 1e-8 and worst <= 0.1


def test_resolving_power(recovery):
    """R at every line against E / (FWHM |dE/dh| sigma_true) of the channel's own polynomial: R is
    inversely proportional to the fitted sigma, so it is recovered within the sigma bound; the slope
    is taken at the fitted centre, which moves it by less than |c2| 2 (8 sigma / sqrt N) / |slope|."""
    cal, lines = recovery['cal'], recovery['lines']
    E = np.array(wc.ENERGIES[3])
    slope = cal['c'][:, 1:2] + 2 * cal['c'][:, 2:3] * recovery['centres']
    r_true = E[None, :] / (wc.FWHM * np.abs(slope) * SIG)
    dslope = np.abs(cal['c'][:, 2:3]) * 2 * (8 * SIG / math.sqrt(NPH)) / np.abs(slope)
    assert np.all(np.abs(r_true / cal['r'] - 1) <= 0.15 + dslope + 0.15 * dslope)
    assert np.all(cal['r'] > 0) and np.all(np.isfinite(cal['r']))


# ---- calibration -----------------------------------------------------------------------------------
def _smooth_three(lo, step):
    nbins = 512
    sp = wc.spectra_of([wc.gauss_row(nbins, [100.3, 250.7, 420.1], 7.0, 50000.0)], nbins)
    rc, lines, _, _ = wc.lines_host(sp, lo, step, nbins, wc.ENERGIES[3], 2, 32, 10, 12)
    assert rc == 0 and np.all(np.isfinite(lines[0]['mu']))
    return nbins, sp, lines[0]['mu'].copy()


@pytest.mark.parametrize('P', [1, 2, 3])
def test_known_polynomial(P):
    """Energies taken from a known polynomial at the fitted centres give that polynomial back: a
    quadratic for three lines, a line for two, a proportionality for one. The centres do not depend
    on the energies, so a first call gives them. Tolerance: E_p = q(mu_p) carries at most 4 roundings,
    which reach c_i through dc_i / dE_p (c is linear in E: the columns are the polynomials of unit
    energies), and Newton's form adds about ten more roundings of terms no larger than
    sum_p |dc_i / dE_p| |E_p|; 16 ulp of that sum covers both."""
    lo, step = -3.0, 0.005      # negative heights: mu from -2.5 to -0.9, energies descending in bin order
    nbins, sp, mu = _smooth_three(lo, step)
    q = {1: [0.0, -1.7, 0.0], 2: [0.3, -1.2, 0.0], 3: [0.2, -1.5, -0.11]}[P]
    mu = mu[:P] if P < 3 else mu
    sp_p = sp if P == 3 else wc.spectra_of([np.where(np.arange(nbins) < [0, 180, 340][P], sp[0, 1:nbins + 1], 0)], nbins)
    E = [q[0] + m * (q[1] + m * q[2]) for m in mu]
    rc, lines, cal, cal_f = wc.lines_host(sp_p, lo, step, nbins, E, 2, 32, 10, 12)
    assert rc == 0 and cal[0]['status'] == 0 and np.array_equal(lines[0]['mu'], mu)
    unit = np.array([wc.poly_ref([1.0 if k == p else 0.0 for k in range(P)], list(mu)) for p in range(P)])   # [p][i]
    for i in range(3):
        tol = 16 * 2.0 ** -52 * float(np.sum(np.abs(unit[:, i]) * np.abs(E)))
        assert abs(cal[0]['c'][i] - q[i]) <= tol, (i, cal[0]['c'][i], q[i], tol)
    assert cal_f[0][3] == 1.0 and np.array_equal(cal_f[0][:3], cal[0]['c'].astype(np.float32))
    ec = wavecal.EnergyCal(lines, cal, cal_f, E)
    h = np.float32(mu[0])
    assert abs(float(ec.energy(0, h)) - E[0]) <= 1e-5 * abs(E[0])        # the fp32 rule at a line
    assert np.all(np.isnan(cal[0]['r'][P:])) and np.all(cal[0]['r'][:P] > 0)


def test_non_monotonic_is_flagged():
    nbins, sp, mu = _smooth_three(0.0, 1.0)
    rc, lines, cal, cal_f = wc.lines_host(sp, 0.0, 1.0, nbins, [1.26, 3.06, 1.88], 2, 32, 10, 12)
    assert rc == 0 and cal[0]['status'] == _lib.CAL_BAD_SLOPE and cal[0]['n_found'] == 3
    assert np.all(np.isnan(cal[0]['c'])) and np.all(np.isnan(cal[0]['r'])) and cal_f[0][3] == 0.0
    assert np.all(np.isnan(cal_f[0][:3])) and np.all(np.isfinite(lines[0]['mu']))
    ec = wavecal.spectrum_lines_host(sp, 0.0, 1.0, nbins, [1.26, 3.06, 1.88])
    assert not ec.usable()[0] and np.isnan(ec.energy(0, 1.0)) and np.all(np.isnan(ec.resolving_power()))


def test_wavecal_module_matches_the_twin(recovery):
    ec = wavecal.spectrum_lines_host(recovery['sp'], 0.0, 1.0, NB, wc.ENERGIES[3], **{
        'smooth': PARAMS['w'], 'min_sep': PARAMS['min_sep'], 'min_peak': PARAMS['min_peak'], 'fit_half': PARAMS['g']})
    assert wc.same_bits(ec.lines, recovery['lines']) and wc.same_bits(ec.cal, recovery['cal'])
    assert wc.same_bits(ec.cal_f, recovery['cal_f']) and ec.usable().all()
    assert wc.same_bits(ec.resolving_power(), recovery['cal']['r'])
    rng = np.random.default_rng(2)
    ch, h = rng.integers(0, NCH, 500), rng.uniform(0, 512, 500).astype(np.float32)
    h[:5] = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    assert wc.same_bits(ec.energy(ch, h), wc.energy_ref(h, ec.cal_f[ch]))


# ---- the cube --------------------------------------------------------------------------------------
CUBE = wc.cube_case()


@pytest.mark.parametrize('mode,vlo,vinv,nb', wc.CUBE_MODES, ids=['energy', 'wavelength', 'energy257'])
def test_cube_matches_restatement(mode, vlo, vinv, nb):
    c = CUBE
    rc, cube, energy = wc.cube_host(c['ev'], c['h'], c['j0'], c['j_defer'], c['C'], c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    assert rc == 0
    rcube, renergy = wc.cube_ref(c['ev'], c['h'], c['j0'], c['j_defer'], c['C'], c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    assert np.array_equal(cube, rcube) and wc.same_bits(energy, renergy)
    ch, jg = oc.decode(c['ev'], c['j0'])
    pix = ch < c['C']
    held = pix & ~np.isfinite(c['h']) & (jg >= c['j_defer'])
    settled_nan = pix & ~np.isfinite(c['h']) & (jg < c['j_defer'])
    assert held.sum() > 20 and settled_nan.sum() > 20 and (~pix).sum() > 100
    assert cube.sum() == (pix & ~held).sum()
    assert np.all(energy[~pix] == np.float32(-1234.5))                       # untouched
    assert np.all(energy[pix].view(np.uint32)[np.isnan(energy[pix])] == 0x7FC00000)
    assert cube[3].sum() == cube[3, nb + 2] > 0 and cube[4].sum() == cube[4, nb + 2] > 0     # not usable
    if mode == _lib.CUBE_ENERGY:
        assert cube[6].sum() == cube[6, nb + 2] > 0                          # e = +-inf or inf - inf
    if mode == _lib.CUBE_WAVELENGTH:
        assert cube[5].sum() == cube[5, nb + 2] > 0                          # e = 0: hc / e = inf
        fin = np.isfinite(c['h']) & (ch == 7)
        assert cube[7, 0] == fin.sum() > 0                                   # e < 0: below vlo
    # row totals equal the spectra's over the same list
    lo, inv = oc.bins(c['C'], 64, np.random.default_rng(1))
    _, spectra, _, _ = oc.spectra_host(c['ev'], c['h'], c['j0'], c['j_defer'], c['C'], lo, inv, 64, defer=True,
                                       cap_def=len(c['ev']))
    assert np.array_equal(cube.sum(axis=1), spectra.sum(axis=1))


def test_cube_chunking_cap_and_empty():
    c = CUBE
    mode, vlo, vinv, nb = wc.CUBE_MODES[1]
    args = (c['j0'], c['j_defer'], c['C'], c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    _, whole, ewhole = wc.cube_host(c['ev'], c['h'], *args)
    rng = np.random.default_rng(8)
    n = len(c['ev'])
    for cuts in ([0, n], [0] + sorted(rng.integers(0, n + 1, 7)) + [n], [0, 1, 2, 3, n]):
        cube = np.zeros_like(whole)
        energy = np.full(n, np.float32(-1234.5), np.float32)
        for a, b in zip(cuts[:-1], cuts[1:]):
            rc, _, e = wc.cube_host(c['ev'][a:b], c['h'][a:b], *args, cube=cube)
            assert rc == 0
            energy[a:b] = e[:b - a]
        assert np.array_equal(cube, whole) and wc.same_bits(energy, ewhole)
    o = rng.permutation(n)
    assert np.array_equal(wc.cube_host(c['ev'][o], c['h'][o], *args)[1], whole)
    # n below the list's length (the counted form's cap): only the first n packets
    rc, part, _ = wc.cube_host(c['ev'], c['h'], *args, n=1000)
    assert rc == 0 and np.array_equal(part, wc.cube_ref(c['ev'][:1000], c['h'][:1000], *args)[0])
    rc, none, _ = wc.cube_host(None, None, *args, n=0)
    assert rc == 0 and not none.any()
    rc, cube2, e2 = wc.cube_host(c['ev'], c['h'], *args, want_energy=False)   # d_energy is optional
    assert rc == 0 and e2 is None and np.array_equal(cube2, whole)


# ---- quick-look ------------------------------------------------------------------------------------
def _image_worker(data, total_pix, sky_subtraction, bintype):
    """ArconsDashboard.py image_Worker.run with setup_thread, subtract_sky and calc_mean_energy
    (:1303-1360, 1449-1472), line by line in Python floats and ints."""
    h, c, Emin, Emax = 4.13567E-15, 3.0E17, 0.92, 3.18
    if bintype == 'energy':
        binmin, binmax = Emin, Emax
    else:
        binmax, binmin = h * c / Emin, h * c / Emax
    dE = (binmax - binmin) / 10.
    E = [binmin + dE / 2.]
    for _ in range(9):
        E.append(E[-1] + dE)
    numbers = struct.unpack(total_pix * '10I', data)
    C = [[numbers[p * 10 + k] for p in range(total_pix)] for k in range(10)]
    meds = [float(np.median(C[k])) for k in range(10)]
    if sky_subtraction:
        C = [[x - int(meds[k]) for x in C[k]] for k in range(10)]
    pc = [sum(C[k][m] for k in range(10)) for m in range(total_pix)]
    me = []
    for p in range(total_pix):
        num = C[0][p] * E[0]
        for k in range(1, 10):
            num = num + C[k][p] * E[k]
        v = num / pc[p] if pc[p] != 0 else math.nan
        if bintype != 'energy' and pc[p] != 0:
            v = h * c / v if v != 0 else math.inf
        me.append(v)
    return C, meds, pc, me, E, dE


def _snr(totalcounts, medians, npix, sky):
    SNR, total_signal, total_n = [0] * 10, 0, 0
    for i in range(len(medians)):
        signal = totalcounts[i] if sky else totalcounts[i] - npix * medians[i]
        noise = npix * medians[i]
        if signal < 0:
            signal = 0
        if noise == 0:
            noise = 1
        total_signal += signal
        total_n += noise
        SNR[i] = signal / math.sqrt(noise)
    return SNR, total_signal / math.sqrt(total_n)


@pytest.mark.parametrize('npix', [64, 63])
@pytest.mark.parametrize('sky', [False, True])
@pytest.mark.parametrize('bintype', ['wavelength', 'energy'])
def test_quicklook_equals_image_worker(npix, sky, bintype):
    rng = np.random.default_rng(npix + 2 * sky)
    cube = rng.poisson(30.0, (npix, 13)).astype(np.int32)
    cube[:, 4] += rng.integers(0, 2000, npix).astype(np.int32)     # a bright slice
    cube[5, 1:11] = 0                                               # a pixel with no counts
    cube[7, 3] = -5                                                 # a count past 2^31 as uint32
    data = quicklook.data_bin(cube)
    assert struct.unpack(npix * '10I', data) == tuple(int(x) for x in cube[:, 1:11].astype(np.int64).ravel() % 2 ** 32)
    C, meds, pc, me, E, dE = _image_worker(data, npix, sky, bintype)
    got = quicklook.image(cube, sky_subtraction=sky, bintype=bintype)
    centres, gdE = quicklook.slice_centres(bintype)
    assert list(centres) == E and gdE == dE
    assert np.array_equal(got['counts'], np.array(C).T) and list(got['medians']) == meds
    assert list(got['pc']) == pc
    assert np.array_equal(got['me'], np.array(me), equal_nan=True)
    if not sky:
        assert pc[5] == 0 and math.isnan(got['me'][5])
    sel = [1, 2, 9, 17]
    tot = [int(sum(C[k][p] for p in sel)) for k in range(10)]
    snr, integ = quicklook.calculate_snr(tot, meds, len(sel), sky)
    rsnr, rinteg = _snr(tot, meds, len(sel), sky)
    assert list(snr) == rsnr and integ == rinteg
    mode, lo, hi, nb = quicklook.slice_bins(bintype)
    assert nb == 10 and (lo, hi) == quicklook.slice_range(bintype)
    assert mode == (_lib.CUBE_ENERGY if bintype == 'energy' else _lib.CUBE_WAVELENGTH)


# ---- MKID_E_ARG ------------------------------------------------------------------------------------
def test_lines_argument_errors():
    nbins = 64
    sp = wc.spectra_of([r for _, r in wc.rows_for(nbins)][:3], nbins)
    ok = dict(spectra=sp, lo=0.0, step=1.0, nbins=nbins, E=[1.0, 2.0], w=2, min_sep=4, min_peak=10, g=6)
    call = lambda **kw: wc.lines_host(**{**ok, **{k: v for k, v in kw.items() if k not in ('null', 'nch')}},
                                      null=kw.get('null', ()), nch=kw.get('nch'))[0]
    assert call() == 0
    for name in ('spectra', 'lo', 'step', 'E', 'lines', 'cal', 'cal_f'):
        assert call(null=(name,)) == _lib.MKID_E_ARG, name
    bad = [dict(nch=0), dict(nch=-1), dict(nbins=0), dict(nbins=16385), dict(E=[]), dict(E=[1.0, 2.0, 3.0, 4.0]),
           dict(w=-1), dict(w=65), dict(min_sep=0), dict(g=0), dict(g=65), dict(E=[1.0, 1.0]), dict(E=[0.0, 1.0]),
           dict(E=[-1.0, 1.0]), dict(E=[np.nan, 1.0]), dict(E=[np.inf, 1.0]), dict(E=[2.0, 1.0, 2.0])]
    for kw in bad:
        assert call(**kw) == _lib.MKID_E_ARG, kw
    assert call(min_peak=-5) == 0 and call(min_peak=2 ** 62) == 0 and call(E=[2.0, 1.0]) == 0 and call(w=0, g=64) == 0


def test_cube_argument_errors():
    c = CUBE
    mode, vlo, vinv, nb = wc.CUBE_MODES[0]
    base = dict(ev=c['ev'], h=c['h'], j0=c['j0'], j_defer=c['j_defer'], C=c['C'], cal_f=c['cal_f'], mode=mode, hc=wc.HC,
                vlo=vlo, vinv=vinv, nb=nb)
    call = lambda **kw: wc.cube_host(**{**base, **kw})[0]
    assert call() == 0
    for name in ('ev', 'h', 'cal_f', 'cube'):
        assert call(null=(name,)) == _lib.MKID_E_ARG, name
    for kw in (dict(n=-1), dict(j0=-1), dict(C=0), dict(C=4097), dict(mode=2), dict(mode=-1), dict(nb=0), dict(nb=16385)):
        assert call(**kw) == _lib.MKID_E_ARG, kw
    assert call(null=('ev', 'h'), n=0) == 0 and call(null=('energy',)) == 0
    assert call(vinv=np.float32(np.nan), hc=np.float32(np.inf), vlo=np.float32(-np.inf)) == 0   # any float is defined
