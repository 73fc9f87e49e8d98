"""mkid_spectrum_lines and mkid_energy_cube on the device (k_wavecal.hip) against the host twins and
the restatements of tests/wavecal_cases.py, which tests/test_wavecal_host.py holds against each
other: integers, the cube and the energies exactly, the float part within the bars derived per fit.
Then a streamed run with pulses of three heights through observe.Observation: calibrate, a second
run with energy=cal, and an Observation without the argument against one that never had it.

Recorded on an MI355X (profiles/wavecal/new_gputests.txt): the largest ratio of a device float to its
bar is 2.9e-4 over the case table, 2.3e-5 on the 65-channel recovery set and 0.027 on the streamed
run's sparse spectra, where 6 of the 64 channels calibrate.
"""
import numpy as np
import pytest

import observe_cases as oc
import wavecal_cases as wc
from mkids_sdr_amd import _lib, observe, quicklook, wavecal

pytestmark = pytest.mark.gpu
C = 64


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(C, max_chunk=2 ** 14)
    yield ch
    ch.close()


def _dev(a):
    import torch
    a = np.array(a, order='C')       # a writable copy
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    torch.cuda.synchronize()     # torch's stream made it, the context's stream reads it
    return t


def _host(*ts):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def dev_lines(ctx, sp, lo, step, nbins, E, w, min_sep, min_peak, g):
    """mkid_spectrum_lines -> (lines [nch][P], cal [nch], cal_f [nch][4], spectra afterwards)."""
    import torch
    nch, P = sp.shape[0], len(E)
    d_sp = _dev(sp)
    d_lines = torch.full((nch * P * wc.LINE_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    d_cal = torch.full((nch * wc.CAL_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    d_cal_f = torch.full((nch, 4), -9.0, dtype=torch.float32, device='cuda')
    lo32 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (nch,)))
    st32 = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (nch,)))
    d_lo, d_step = _dev(lo32), _dev(st32)
    ctx.spectrum_lines_device(d_sp, d_lo, d_step, nch, nbins, E, w, min_sep, min_peak, g, d_lines, d_cal, d_cal_f)
    lines, cal, cal_f, after = _host(d_lines, d_cal, d_cal_f, d_sp)
    return lines.view(wc.LINE_DT).reshape(nch, P), cal.view(wc.CAL_DT), cal_f, after


INT_FIELDS = ('bin', 'nfit', 'peak_s', 'counts')
# one (P, w, g, ...) of the table per nbins and nch beyond the full table at nch = 3, to keep the runs short
NCH_PARAMS = {1: [0, 7, 17], 65: [4, 11, 18, 19]}


@pytest.mark.parametrize('nbins', [1, 3, 257, 16384])
@pytest.mark.parametrize('nch', [1, 3, 65])
def test_lines_parity(ctx, nbins, nch):
    """Channel i holds row (i + nch) mod R of the case table's R shapes, so a shape sits at different
    indices for different nch. Integers bit-equal to the host twin, floats within the derived bar of
    the restatement, rows of equal content bit-equal whatever their index, a second run bit-equal,
    the spectrum unchanged. The status bits that are read from floats, and the floats, are compared
    in the channels whose fits are determined within their bars (wavecal_cases' docstring: a flat
    window's curvature is rounding noise, and its sign turns with the last bit of log)."""
    rows = wc.rows_for(nbins)
    R = len(rows)
    idx = [(i + nch) % R for i in range(nch)]
    if nch == 3:                       # every shape passes through the three-channel call
        groups = [[(k + i) % R for i in range(3)] for k in range(0, R, 3)]
        params = wc.param_table(nbins)
    else:
        groups = [idx]
        params = [wc.param_table(nbins)[k] for k in NCH_PARAMS[nch]]
    worst = 0.0
    refs = {}
    seen = {True: 0, False: 0}
    for grp in groups:
        sp = wc.spectra_of([rows[r][1] for r in grp], nbins)
        for P, w, g, min_sep, min_peak, E in params:
            lines, cal, cal_f, after = dev_lines(ctx, sp, 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
            assert np.array_equal(after, sp)
            rc, hl, hc, hf = wc.lines_host(sp, 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
            assert rc == 0
            for f in INT_FIELDS:
                assert np.array_equal(lines[f], hl[f]), f
            assert np.array_equal(cal['n_found'], hc['n_found'])
            first = {}
            for i, r in enumerate(grp):
                key = (r, P, w, g, min_sep, min_peak, tuple(E))
                if key not in refs:
                    refs[key] = wc.lines_ref(sp[i, 1:nbins + 1], 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
                det = refs[key]['cal']['determined']
                wc.check_ints(lines[i], cal[i], refs[key], status=det)
                seen[det] += 1
                if det:
                    assert cal[i]['status'] == hc[i]['status']
                    worst = max(worst, wc.float_ratio(lines[i], cal[i], cal_f[i], refs[key]))
                if r in first:         # the same row at another index of the same call
                    j = first[r]
                    assert wc.same_bits(lines[i], lines[j]) and wc.same_bits(cal[i], cal[j]) and wc.same_bits(cal_f[i], cal_f[j])
                first.setdefault(r, i)
            if nch != 3 and (P, w, g) == params[0][:3]:
                again = dev_lines(ctx, sp, 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
                assert wc.same_bits(again[0], lines) and wc.same_bits(again[1], cal) and wc.same_bits(again[2], cal_f)
                # channel 0's row alone, as a one-channel call: the same bits
                one = dev_lines(ctx, sp[:1], 0.25, 0.5, nbins, E, w, min_sep, min_peak, g)
                assert wc.same_bits(one[0][0], lines[0]) and wc.same_bits(one[1][0], cal[0]) and wc.same_bits(one[2][0], cal_f[0])
    print('nbins %d nch %d: largest ratio of a device float to its bar %.3g (%d channels determined, %d not)'
          % (nbins, nch, worst, seen[True], seen[False]))
    assert worst <= 1.0 and seen[True] >= 4 * seen[False]


def test_lines_recovery_set_on_the_device(ctx):
    """65 channels of three Poisson lines (the recovery set's shape): all found, the floats within
    their bars, and the calibration table equal to the float32 of the device's own coefficients."""
    rng = np.random.default_rng(31)
    nb, sig, nph = 512, 8.0, 20000
    centres = np.array([120.0, 260.0, 400.0])[None, :] + rng.uniform(-10, 10, (65, 3))
    rows = []
    for c in range(65):
        n = rng.poisson(10.0, nb).astype(np.int64)
        for p in range(3):
            n += np.histogram(rng.normal(centres[c, p], sig, nph), bins=nb, range=(0, nb))[0]
        rows.append(n)
    sp = wc.spectra_of(rows, nb)
    lo, step = rng.uniform(-3, -2, 65).astype(np.float32), rng.uniform(0.004, 0.006, 65).astype(np.float32)
    E = wc.ENERGIES[3][::-1]
    lines, cal, cal_f, _ = dev_lines(ctx, sp, lo, step, nb, E, 2, 32, 10, 12)
    assert np.all(cal['status'] == 0) and np.all(cal['n_found'] == 3)
    worst = 0.0
    for c in range(65):
        ref = wc.lines_ref(sp[c, 1:nb + 1], lo[c], step[c], nb, E, 2, 32, 10, 12)
        assert ref['cal']['determined']
        wc.check_ints(lines[c], cal[c], ref)
        worst = max(worst, wc.float_ratio(lines[c], cal[c], cal_f[c], ref))
    print('recovery set: largest ratio of a device float to its bar %.3g' % worst)
    assert worst <= 1.0
    z = ((lines['mu'] - lo[:, None]) / step[:, None] - centres) / (sig / np.sqrt(nph))
    assert z.std() <= 2 and np.abs(z).max() <= 8 and np.abs(lines['sigma'] / step[:, None] / sig - 1).max() <= 0.15


def test_lines_argument_errors(ctx):
    import torch
    nbins = 64
    sp = wc.spectra_of([r for _, r in wc.rows_for(nbins)][:3], nbins)
    d_sp, d_lo, d_step = _dev(sp), _dev(np.zeros(3, np.float32)), _dev(np.ones(3, np.float32))
    d_lines = torch.zeros(3 * 3 * 48, dtype=torch.uint8, device='cuda')
    d_cal = torch.zeros(3 * 56, dtype=torch.uint8, device='cuda')
    d_cal_f = torch.full((3, 4), -9.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    ok = dict(d_spectra=d_sp, d_lo=d_lo, d_step=d_step, nch=3, nbins=nbins, energies=[1.0, 2.0], smooth=2, min_sep=4,
              min_peak=10, fit_half=6, d_lines=d_lines, d_cal=d_cal, d_cal_f=d_cal_f)
    bad = [dict(d_spectra=None), dict(d_lo=None), dict(d_step=None), dict(d_lines=None), dict(d_cal=None),
           dict(d_cal_f=None), dict(nch=0), dict(nbins=0), dict(nbins=16385), dict(energies=[]),
           dict(energies=[1.0, 2.0, 3.0, 4.0]), dict(energies=[1.0, 1.0]), dict(energies=[-1.0, 1.0]),
           dict(energies=[np.nan]), dict(smooth=-1), dict(smooth=65), dict(min_sep=0), dict(fit_half=0), dict(fit_half=65)]
    for kw in bad:
        with pytest.raises(_lib.MkidError) as e:
            ctx.spectrum_lines_device(**{**ok, **kw})
        assert e.value.code == _lib.MKID_E_ARG, kw
    assert np.all(_host(d_cal_f)[0] == -9.0)           # nothing was launched
    ctx.spectrum_lines_device(**ok)
    assert np.all(_host(d_cal_f)[0][:, 3] >= 0)


# ---- the cube --------------------------------------------------------------------------------------
CUBE = wc.cube_case(C, 3000)


def dev_cube(ctx, ev, h, j0, j_defer, cal_f, mode, hc, vlo, vinv, nb, cube=None, count=None, cap=None, energy=True):
    import torch
    n = len(ev)
    d_ev, d_h = (_dev(ev), _dev(np.asarray(h, np.float32))) if n else (None, None)
    d_cube = _dev(np.zeros((ctx.C, nb + 3), np.int32) if cube is None else cube)
    d_e = _dev(np.full(max(n, 1), np.float32(-1234.5), np.float32)) if energy else None
    d_cal = _dev(cal_f)
    if count is None:
        ctx.energy_cube_device(d_ev, d_h, n, j0, j_defer, d_cal, mode, hc, vlo, vinv, nb, d_cube, d_e)
    else:
        ctx.energy_cube_counted(d_ev, d_h, _dev(np.array([count], np.int64)), cap, j0, j_defer, d_cal, mode, hc, vlo,
                                vinv, nb, d_cube, d_e)
    torch.cuda.synchronize()
    return d_cube.cpu().numpy(), (d_e.cpu().numpy()[:n] if energy else None)


@pytest.mark.parametrize('mode,vlo,vinv,nb', wc.CUBE_MODES, ids=['energy', 'wavelength', 'energy257'])
def test_cube_parity(ctx, mode, vlo, vinv, nb):
    c = CUBE
    args = (c['j0'], c['j_defer'], c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    hargs = (c['j0'], c['j_defer'], C, c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    rc, hcube, henergy = wc.cube_host(c['ev'], c['h'], *hargs)
    assert rc == 0 and hcube.sum() > 2000
    cube, energy = dev_cube(ctx, c['ev'], c['h'], *args)
    assert np.array_equal(cube, hcube) and wc.same_bits(energy, henergy)
    # any order
    o = np.random.default_rng(3).permutation(len(c['ev']))
    cube, energy = dev_cube(ctx, c['ev'][o], c['h'][o], *args)
    assert np.array_equal(cube, hcube) and wc.same_bits(energy, henergy[o])
    # without d_energy
    assert np.array_equal(dev_cube(ctx, c['ev'], c['h'], *args, energy=False)[0], hcube)


def test_cube_four_calls_with_the_deferred_passed_again(ctx):
    """The list cut into four calls, each call's deferred packets passed again with the next call (as
    a streamed step joins them), the last call with nothing deferred: every packet lands once."""
    c = CUBE
    mode, vlo, vinv, nb = wc.CUBE_MODES[1]
    n = len(c['ev'])
    ch, jg = oc.decode(c['ev'], c['j0'])
    cuts = [0, n // 4, n // 2, 3 * n // 4, n]
    cube = np.zeros((C, nb + 3), np.int32)
    hcube = np.zeros((C, nb + 3), np.int32)
    held_ev, held_h = np.zeros(0, np.uint64), np.zeros(0, np.float32)
    for k in range(4):
        ev = np.concatenate([held_ev, c['ev'][cuts[k]:cuts[k + 1]]])
        h = np.concatenate([held_h, c['h'][cuts[k]:cuts[k + 1]]])
        jd = c['j_defer'] if k < 3 else (1 << 62)
        cube, energy = dev_cube(ctx, ev, h, c['j0'], jd, c['cal_f'], mode, wc.HC, vlo, vinv, nb, cube=cube)
        rc, hcube, henergy = wc.cube_host(ev, h, c['j0'], jd, C, c['cal_f'], mode, wc.HC, vlo, vinv, nb, cube=hcube)
        assert rc == 0 and np.array_equal(cube, hcube) and wc.same_bits(energy, henergy)
        e_ch, e_jg = oc.decode(ev, c['j0'])
        held = (e_ch < C) & ~np.isfinite(h) & (e_jg >= jd)
        held_ev, held_h = ev[held], h[held]
        assert k == 3 or held.sum() > 0
    assert cube.sum() == (ch < C).sum()
    whole = wc.cube_host(c['ev'], c['h'], c['j0'], 1 << 62, C, c['cal_f'], mode, wc.HC, vlo, vinv, nb)[1]
    assert np.array_equal(cube, whole)


def test_cube_one_row_calls_counted_and_empty(ctx):
    c = CUBE
    mode, vlo, vinv, nb = wc.CUBE_MODES[0]
    args = (c['j0'], c['j_defer'], c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    hargs = (c['j0'], c['j_defer'], C, c['cal_f'], mode, wc.HC, vlo, vinv, nb)
    m = 40
    cube = np.zeros((C, nb + 3), np.int32)
    for i in range(m):                                   # 1-row calls
        cube, e = dev_cube(ctx, c['ev'][i:i + 1], c['h'][i:i + 1], *args, cube=cube)
    assert np.array_equal(cube, wc.cube_host(c['ev'][:m], c['h'][:m], *hargs)[1])
    # counted: a count below, at and above the capacity, and a negative one
    for count, cap in ((1000, 3000), (3000, 3000), (5000, 2500), (-3, 3000), (0, 3000)):
        k = max(0, min(count, cap))
        cube, energy = dev_cube(ctx, c['ev'], c['h'], *args, count=count, cap=cap)
        rc, hcube, henergy = wc.cube_host(c['ev'][:k], c['h'][:k], *hargs)
        assert np.array_equal(cube, hcube), (count, cap)
        assert wc.same_bits(energy[:k], henergy[:k]) and np.all(energy[k:] == np.float32(-1234.5))
    cube, _ = dev_cube(ctx, np.zeros(0, np.uint64), np.zeros(0, np.float32), *args)
    assert not cube.any()


def test_cube_argument_errors(ctx):
    import torch
    c = CUBE
    mode, vlo, vinv, nb = wc.CUBE_MODES[0]
    d_ev, d_h, d_cal = _dev(c['ev']), _dev(c['h']), _dev(c['cal_f'])
    d_cube = torch.zeros((C, nb + 3), dtype=torch.int32, device='cuda')
    d_n = _dev(np.array([5], np.int64))
    ok = dict(d_events=d_ev, d_heights=d_h, n=len(c['ev']), j0=c['j0'], j_defer=c['j_defer'], d_cal_f=d_cal, mode=mode,
              hc=wc.HC, vlo=vlo, vinv=vinv, nb=nb, d_cube=d_cube)
    for kw in (dict(d_events=None), dict(d_heights=None), dict(d_cal_f=None), dict(d_cube=None), dict(n=-1), dict(j0=-1),
               dict(mode=2), dict(nb=0), dict(nb=16385)):
        with pytest.raises(_lib.MkidError) as e:
            ctx.energy_cube_device(**{**ok, **kw})
        assert e.value.code == _lib.MKID_E_ARG, kw
    okc = {k: v for k, v in ok.items() if k != 'n'}
    with pytest.raises(_lib.MkidError) as e:
        ctx.energy_cube_counted(d_count=None, cap=10, **okc)
    assert e.value.code == _lib.MKID_E_ARG
    with pytest.raises(_lib.MkidError) as e:
        ctx.energy_cube_counted(d_count=d_n, cap=-1, **okc)
    assert e.value.code == _lib.MKID_E_ARG
    assert not _host(d_cube)[0].any()
    ctx.energy_cube_device(**{**ok, 'n': 0, 'd_events': None, 'd_heights': None})
    assert not _host(d_cube)[0].any()


# ---- Observation -----------------------------------------------------------------------------------
S, K, NCOEFF, PRE, NBINS = 2 ** 15, 12, 40, 24, 128
J = S // (2 * C)
AMPS_DEG = (35.0, 60.0, 85.0)
TAU_FALL, WINDOW, PER_CH = 8.0, 60, 70.0     # short pulses: 70 a channel in 3072 rows, about half of them clean
LO, STEP = -2.0, 2.0 / NBINS                 # heights are about minus the pulse amplitude in radians
LINE_ARGS = dict(smooth=2, min_sep=8, min_peak=6, fit_half=4)


def three_height_stream():
    """K chunks of S samples; chunk k carries pulses of amplitude AMPS_DEG[k mod 3] only (three cases
    of one seed: the same tones, noise and pulse times, another amplitude). A packet is stamped about
    7 rows after the phase minimum and 18 after the first moved row, so the filter takes the mean of
    the three rows around the minimum less the mean of the window's first five rows: a height is
    minus the pulse's depth in radians, and a channel's pulse-height spectrum holds three lines."""
    import signals
    cases = [signals.make_case(C, K * S, seed=7, pulses_per_ch=PER_CH, amp_deg=(a, a), tau_fall=TAU_FALL,
                               window_phase=WINDOW) for a in AMPS_DEG]
    iq = np.concatenate([cases[k % 3].iq[k * S:(k + 1) * S] for k in range(K)])
    quiet = signals.make_case(C, S, seed=7, pulses_per_ch=0)
    thr = signals.thresholds_from_quiet(quiet, signals.oracle_chain(quiet).process(quiet.iq)['raw'])
    shape = np.zeros(NCOEFF)
    shape[:5], shape[PRE - 8:PRE - 5] = -1 / 5, 1 / 3
    coeff = np.tile(shape.astype(np.float32), (C, 1))
    return cases[0], iq, thr, coeff


def run_observation(case, iq, thr, coeff, debug=False, pass_energy=False, **kw):
    """The streamed run: K process_device calls, each followed by Observation.step. -> dict of the
    products on the host, and the Observation's calibration when asked."""
    import torch
    from mkids_sdr_amd.channelizer import Channelizer
    x = torch.from_numpy(iq.reshape(-1)).to('cuda')
    cap = J * C
    ch = Channelizer(C, max_chunk=S, sample_rate=2 * C * 600)
    try:
        ch.set_pfb(case.pfb)
        ch.set_bins(case.bins)
        ch.set_dds(case.lut_i, case.lut_q)
        ch.set_lpf(case.lpf12)
        ch.set_fir(case.fir12)
        ch.set_centers(case.ic, case.qc)
        ch.set_thresholds(thr)
        ch.set_pulse_filter(coeff, PRE)
        if pass_energy:
            obs = observe.Observation(ch, 6, NBINS, LO, STEP, cap, cap, debug=debug, photon_rows=8, **kw)
        else:
            obs = observe.Observation(ch, 6, NBINS, LO, STEP, cap, cap, debug=debug, photon_rows=8)
        bufs = [(torch.empty((J, C), dtype=torch.float32, device='cuda'), torch.empty(cap, dtype=torch.int64, device='cuda'),
                 torch.zeros(2, dtype=torch.int64, device='cuda')) for _ in range(K)]
        torch.cuda.synchronize()
        for k, (d_ph, d_ev, d_cnt) in enumerate(bufs):
            ch.process_device(x[2 * k * S:2 * (k + 1) * S], S, d_ph, d_ev, cap, d_cnt)
            obs.step(d_ph, J, k * J, d_ev, d_cnt)
        torch.cuda.synchronize()
        out = dict(image=obs.image(), spectra=obs.spectra(), outside=obs.outside(), pending=obs.pending(),
                   ndef=obs.deferred_counts(), fill=obs.fill_counts(), dropped=obs.dropped(), steps=obs.steps,
                   words=obs.d_words.cpu().numpy(), row_height=obs.d_row_height.cpu().numpy(),
                   step_energies=obs.step_energies)
        if obs.energy is not None:
            out['cube'] = obs.cube()
            out['rule'] = (obs.cube_mode, obs.hc, obs.vlo, obs.vinv, obs.nb)
        else:
            with pytest.raises(ValueError):
                obs.cube()
            out['cal'] = obs.calibrate(AMPS_E, **LINE_ARGS)
        return out
    finally:
        ch.close()


AMPS_E = [3.06, 1.88, 1.26]       # heights are negative: the largest pulse is the lowest bin


@pytest.fixture(scope='module')
def stream(gpu):
    return three_height_stream()


@pytest.fixture(scope='module')
def first_run(stream):
    return run_observation(*stream)


def test_observation_calibrate_then_cube(stream, first_run):
    cal = first_run['cal']
    # the calibration is the host twin's on the run's own spectra
    la = (LINE_ARGS['smooth'], LINE_ARGS['min_sep'], LINE_ARGS['min_peak'], LINE_ARGS['fit_half'])
    rc, hl, hc, hf = wc.lines_host(first_run['spectra'], LO, STEP, NBINS, AMPS_E, *la)
    assert rc == 0
    for f in INT_FIELDS:
        assert np.array_equal(cal.lines[f], hl[f]), f
    worst = 0.0
    for c in range(C):
        ref = wc.lines_ref(first_run['spectra'][c, 1:NBINS + 1], LO, STEP, NBINS, AMPS_E, *la)
        wc.check_ints(cal.lines[c], cal.cal[c], ref, status=ref['cal']['determined'])
        if ref['cal']['determined']:           # a handful of counts a line: flat windows occur
            assert cal.status[c] == hc['status'][c]
            worst = max(worst, wc.float_ratio(cal.lines[c], cal.cal[c], cal.cal_f[c], ref))
    assert worst <= 1.0
    usable = cal.usable()
    print('usable channels: %d of %d; largest ratio %.3g' % (usable.sum(), C, worst))
    # about 23 packets a channel in three lines widened by pile-up: the CPU oracle's phase gives three
    # fitted lines in 6 of the 64 channels, and every status bit but the slope's in the others
    assert usable.sum() >= 1 and (~usable).sum() >= 1
    second = run_observation(*stream, debug=True, pass_energy=True, energy=cal,
                             energy_bins=(_lib.CUBE_ENERGY, 0.0, 4.0, 10))
    mode, hc_, vlo, vinv, nb = second['rule']
    assert (mode, nb) == (_lib.CUBE_ENERGY, 10) and vlo == np.float32(0) and vinv == np.float32(1) / np.float32(0.4)
    cube = np.zeros((C, nb + 3), np.int32)
    for (joined, h, j0, jd), energies in zip(second['steps'], second['step_energies']):
        cube, e = wc.cube_ref(joined, h, j0, jd, C, cal.cal_f, mode, hc_, vlo, vinv, nb, cube=cube)
        assert wc.same_bits(energies, e)                # every packet of the run is a pixel's
        assert wc.same_bits(e, cal.energy(oc.decode(joined, j0)[0], h))
    assert np.array_equal(second['cube'], cube)
    assert np.array_equal(second['cube'].sum(axis=1), second['spectra'].sum(axis=1))
    assert second['cube'][usable][:, 1:nb + 1].sum() > 0            # photons with an energy inside the bins
    assert np.all(second['cube'][~usable][:, :nb + 2] == 0)         # no calibration: "no energy"
    # the cube changes nothing else: every other product equals the first run's
    for k in ('image', 'spectra', 'outside', 'pending', 'ndef', 'fill', 'dropped', 'words'):
        assert np.array_equal(first_run[k], second[k]), k
    assert wc.same_bits(first_run['row_height'], second['row_height'])
    # the quick-look on the cube
    ql = quicklook.image(second['cube'])
    assert np.array_equal(ql['pc'], second['cube'][:, 1:nb + 1].sum(axis=1))
    assert len(quicklook.data_bin(second['cube'])) == C * 10 * 4


def test_observation_without_energy_is_unchanged(stream, first_run):
    """energy=None passed explicitly against an Observation that never had the argument: spectra,
    image, rows and every count bit-equal, and no cube."""
    again = run_observation(*stream, pass_energy=True, energy=None, energy_bins=None, hc=None)
    for k in ('image', 'spectra', 'outside', 'pending', 'ndef', 'fill', 'dropped', 'words'):
        assert np.array_equal(first_run[k], again[k]), k
    assert wc.same_bits(first_run['row_height'], again['row_height'])
    assert first_run['image'].sum() > 3 * C and 'cube' not in again
