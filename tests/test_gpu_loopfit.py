"""mkid_fit_loops on the device (k_loopfit.hip) against the restatement of tests/loopfit_cases.py, which
tests/test_loopfit_host.py holds bit for bit against the host twin.

The window's integers and the status bits read from the inputs are equal everywhere. The floats are
compared by certificate, not by path, because the device's sin, cos and atan2 are not the host's:
chi^2 of the device's parameters, evaluated by the restatement's model, lies within BARS['chisq'] of
the restatement's chi^2, and each parameter within its bar (loopfit_cases.BARS: ten times what moving
every sin, cos, atan2 result of the restatement by one ulp changes over the table). Channels in which
that perturbed restatement itself changes best_start, evals or the max_iter bit are left out of the
parameter comparison only; the table has none (test_loopfit_host.py holds it under 5 %).

Recorded on an MI355X (profiles/loopfit/new_gputests.txt): 13 tests in 10.9 s; the largest ratio of a
device difference to its bar is 0.030 (Qoff of one channel of 'many24'), the next 3.1e-3 and 1.3e-3
(f0); best_start and evals equal the restatement's in every channel. Through the shim the fitted f0
lie within 3.2e-5 linewidths and the fitted Q within 7.3e-5 of the four resonators set.
"""
import numpy as np
import pytest

import loopfit_cases as lc
from mkids_sdr_amd import _lib, loopfit

pytestmark = pytest.mark.gpu
C = 64


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(C, max_chunk=2 ** 14)
    yield ch
    ch.close()


def dev_fit(ctx, freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=lc.FTOL, want_all=True):
    """mkid_fit_loops into pre-filled outputs -> (fits [nch], chisq_all [nch][S] or None)."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    nch, fsteps = freq.shape
    S = draws.shape[1]
    t = [up(a) for a in (freq, I, Q, isd, qsd, draws, qguess)]
    d_fits = torch.full((nch * lc.FIT_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    d_all = torch.full((nch, S), -7.0, dtype=torch.float64, device='cuda') if want_all else None
    torch.cuda.synchronize()     # torch's stream made them, the context's stream reads them
    ctx.fit_loops_device(*t, nch, fsteps, S, max_iter, ftol, d_fits, d_all)
    torch.cuda.synchronize()
    fits = d_fits.cpu().numpy().view(lc.FIT_DT)
    return fits, None if d_all is None else d_all.cpu().numpy()


def compare(fits, call, ref, rcall, pert, data, kw, label):
    """The rules of the module docstring -> the largest ratio of a float difference to its bar."""
    for k in ('cidx', 'low', 'high', 'n'):
        assert np.array_equal(fits[k], ref[k]), (label, k, fits[k], ref[k])
    read_bits = _lib.LOOP_NONFINITE | _lib.LOOP_FLAT
    assert np.array_equal(fits['status'] & read_bits, ref['status'] & read_bits), label
    assert np.array_equal(fits['status'] & _lib.LOOP_NO_FIT, ref['status'] & _lib.LOOP_NO_FIT), label
    assert np.all(fits['pad'] == 0)
    failed = ref['status'] & lc.FAIL_BITS != 0
    for k in lc.FLOAT_FIELDS:
        assert np.all(np.isnan(fits[k][failed])), (label, k)
    assert np.all(fits['best_start'][failed] == -1) and np.all(fits['evals'][failed] == 0)
    assert np.all(np.isnan(call[failed]))
    worst = 0.0
    same_path = lc.comparable(ref, pert)
    for c in np.where(~failed)[0]:
        assert 0 <= fits['best_start'][c] < call.shape[1] and 1 <= fits['evals'][c] <= kw['max_iter']
        # the winner is the lowest of the device's own starts, ties to the lower start
        assert fits['best_start'][c] == int(np.nanargmin(call[c])) and fits['chisq'][c] == np.nanmin(call[c])
        chi = lc.chisq_of(fits, c, data, kw)
        r_own = abs(fits['chisq'][c] - chi) / chi / lc.BARS['chisq']
        r_chi = abs(chi - ref['chisq'][c]) / ref['chisq'][c] / lc.BARS['chisq']
        ratios = {'own chisq': r_own, 'chisq': r_chi}
        if same_path[c]:
            for i in range(lc.NP):
                ratios['p%d' % i] = lc.rel_change(fits['p'][c, i], ref['p'][c, i]) / lc.BARS['p%d' % i]
            for k in ('qc', 'qi', 'dipdb'):
                ratios[k] = lc.rel_change(fits[k][c], ref[k][c]) / lc.BARS[k]
        top = max(ratios, key=ratios.get)
        print('%s ch %d: largest ratio to its bar %.3g (%s); start %d / %d, evals %d / %d' %
              (label, c, ratios[top], top, fits['best_start'][c], ref['best_start'][c], fits['evals'][c], ref['evals'][c]))
        worst = max(worst, ratios[top])
        assert ratios[top] <= 1.0, (label, c, ratios)
    return worst


@pytest.mark.parametrize('name', list(lc.CASES))
def test_device_against_restatement(ctx, name):
    cs = lc.case(name)
    d = cs['data']
    fits, call = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    compare(fits, call, cs['ref'][0], cs['ref'][1], cs['pert'][0], d, cs['kw'], name)
    again, call2 = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    assert again.tobytes() == fits.tobytes() and lc.same_bits(call, call2)       # a pure function
    alone, none = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], want_all=False, **cs['kw'])
    assert none is None and alone.tobytes() == fits.tobytes()                    # d_chisq_all is optional


def test_device_chunk_invariance(ctx):
    """A channel fitted alone equals the same channel in a call of 65, bit for bit."""
    cs = lc.case('many24')
    d = cs['data']
    whole, wall = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    for c in (0, 31, 64):
        s = slice(c, c + 1)
        one, oall = dev_fit(ctx, d['freq'][s], d['I'][s], d['Q'][s], cs['draws'][s], max_iter=cs['max_iter'])
        assert one.tobytes() == whole[s].tobytes() and lc.same_bits(oall, wall[s])


def test_device_arg_errors(ctx):
    import torch
    d = lc.synth_loops(2, 16, 3, sd=True)
    dr = lc.draws_for(2, 3, 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         dict(d_freq=d['freq'], d_i=d['I'], d_q=d['Q'], d_isd=d['isd'], d_qsd=d['qsd'], d_draws=dr).items()}
    fits = torch.full((2 * lc.FIT_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    ok = dict(t, d_qguess=None, nch=2, fsteps=16, n_starts=3, max_iter=5, ftol=1e-6, d_fits=fits, d_chisq_all=None)
    torch.cuda.synchronize()
    bad = [dict(d_freq=None), dict(d_i=None), dict(d_q=None), dict(d_draws=None), dict(d_fits=None), dict(d_isd=None),
           dict(d_qsd=None), dict(nch=0), dict(fsteps=11), dict(fsteps=1025), dict(n_starts=0), dict(n_starts=17),
           dict(max_iter=0), dict(ftol=0.0), dict(ftol=float('nan'))]
    for kw in bad:
        with pytest.raises(_lib.MkidError) as e:
            ctx.fit_loops_device(**{**ok, **kw})
        assert e.value.code == _lib.MKID_E_ARG, kw
    torch.cuda.synchronize()
    assert bool((fits == 0x5A).all())          # nothing was launched
    ctx.fit_loops_device(**ok)
    torch.cuda.synchronize()
    assert not bool((fits == 0x5A).all())


def test_fit_loops_through_the_shim(gpu):
    """The 64-channel geometry with four resonators on the loop-back feedline, swept by sweepLOready
    in 24 steps: fitLoops() equals the restatement on the swept I, Q under the module's rules, each
    fitted f0 lies within half a linewidth of its resonator, and with use_centers=False neither
    iq_centers nor any register changes. The achieved f0 and Q errors are printed, not asserted."""
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
    I, Q = rs.sweepLOready(1.2e6, 24)          # +-3 linewidths (f0 / Q = 200 kHz) in 50 kHz steps

    writes = []
    write_int, write = roach.write_int, roach.write
    roach.write_int = lambda *a, **k: (writes.append(a), write_int(*a, **k))[1]
    roach.write = lambda *a, **k: (writes.append(a[:1]), write(*a, **k))[1]
    centres, regs = rs.iq_centers.copy(), dict(roach.regs)
    ic, qc = roach.cfg.ic.copy(), roach.cfg.qc.copy()
    out = rs.fitLoops()
    assert out is rs.loop_fits and writes == [] and dict(roach.regs) == regs
    assert np.array_equal(rs.iq_centers, centres) and np.array_equal(roach.cfg.ic, ic) and np.array_equal(roach.cfg.qc, qc)

    x = np.asarray(rs.f_span, np.float64)
    dr = loopfit.draws(4, 10, 0)
    kw = dict(isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10)
    ref, rcall = lc.fit_ref(x, I, Q, dr, **kw)
    pert, _ = lc.fit_ref(x, I, Q, dr, trig=lc.Trig(np.random.default_rng(31)), **kw)
    fits = np.zeros(4, lc.FIT_DT)
    for k in loopfit.FIELDS:
        fits[k] = out[k]
    compare(fits, out['chisq_all'], ref, rcall, pert, dict(freq=x, I=I, Q=Q), kw, 'shim')
    f0 = np.array([r['f0'] for r in res])
    f_err = np.abs(out['p'][:, 1] - f0) / (f0 / 2.0e4)
    print('shim: f0 errors in linewidths', f_err, 'Q errors', out['p'][:, 0] / 2.0e4 - 1.0)
    assert np.all(out['status'] & lc.FAIL_BITS == 0) and np.all(f_err < 0.5)

    rs.fitLoops(use_centers=True)
    assert writes == []
    assert np.array_equal(rs.iq_centers[:4], out['p'][:, 8] + 1j * out['p'][:, 9])
    assert np.array_equal(rs.iq_centers[4:], centres[4:])
