"""mkid_fit_mags on the device (k_magfit.hip) against the host twin mkid_fit_mags_host, which
tests/test_magfit_host.py holds bit for bit against the restatement of tests/magfit_cases.py.

The device differs from the twin through no library function (the model is +, -, x, /, sqrt, |.| and
comparisons), so every field is compared bit for bit over the whole table (two NaNs are equal): a
differing bit is a defect of the kernel (a fused operation, a sum out of order), not a tolerance to
set. The chain (loopfit.fit_sweeps) is held to the two calls made separately, and the shim to the
twin on its swept I and Q.

Recorded on an MI355X (profiles/magfit/new_gputests.txt): 18 tests in 3.5 s, no differing bit. Through
the shim (four resonators of Q = 2e4 whose loops lie off the origin) the magnitude fit's f0 lie 0.18
.. 0.80 linewidths from the resonators and its Q 26 .. 66 % low, as the magnitude model does on such
loops; the loop fit started from that Q ends within 3.2e-5 linewidths and 7.3e-5 in Q, where the
ladder of starts ends too.
"""
import numpy as np
import pytest

import magfit_cases as mc
from mkids_sdr_amd import _lib, loopfit

pytestmark = pytest.mark.gpu
C = 64


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(C, max_chunk=2 ** 14)
    yield ch
    ch.close()


def dev_fit(ctx, freq, I, Q, draws, max_iter=200, ftol=mc.FTOL, want_all=True, want_q=True):
    """mkid_fit_mags into pre-filled outputs -> (fits [nch], qout [nch] or None, chisq_all [nch][S] or None)."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    nch, fsteps = freq.shape
    S = draws.shape[1]
    t = [up(a) for a in (freq, I, Q, draws)]
    d_fits = torch.full((nch * mc.FIT_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    d_q = torch.full((nch,), -7.0, dtype=torch.float64, device='cuda') if want_q else None
    d_all = torch.full((nch, S), -7.0, dtype=torch.float64, device='cuda') if want_all else None
    torch.cuda.synchronize()     # torch's stream made them, the context's stream reads them
    ctx.fit_mags_device(*t, nch, fsteps, S, max_iter, ftol, d_fits, d_q, d_all)
    torch.cuda.synchronize()
    fits = d_fits.cpu().numpy().view(mc.FIT_DT)
    return fits, None if d_q is None else d_q.cpu().numpy(), None if d_all is None else d_all.cpu().numpy()


def twin(d, draws, kw):
    rc, fits, qout, call = mc.fit_host(d['freq'], d['I'], d['Q'], draws, **kw)
    assert rc == 0
    return fits, qout, call


@pytest.mark.parametrize('name', list(mc.CASES))
def test_device_equals_host_twin(ctx, name):
    cs = mc.case(name)
    d = cs['data']
    hf, hq, hall = twin(d, cs['draws'], cs['kw'])
    fits, qout, call = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    mc.check_equal(fits, hf)
    assert mc.same_bits(qout, hq) and mc.same_bits(call, hall)
    again, q2, c2 = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    assert again.tobytes() == fits.tobytes() and q2.tobytes() == qout.tobytes() and c2.tobytes() == call.tobytes()   # pure
    for want_all, want_q in ((False, True), (True, False), (False, False)):     # the optional outputs stay optional
        f3, q3, c3 = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], want_all=want_all, want_q=want_q, **cs['kw'])
        assert f3.tobytes() == fits.tobytes()
        assert (c3 is None) if not want_all else c3.tobytes() == call.tobytes()
        assert (q3 is None) if not want_q else q3.tobytes() == qout.tobytes()


def test_device_chunk_invariance(ctx):
    """A channel fitted alone equals the same channel in the call of 65, bit for bit."""
    cs = mc.case('many24')
    d = cs['data']
    whole, wq, wall = dev_fit(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    for c in (0, 31, 64):
        s = slice(c, c + 1)
        one, oq, oall = dev_fit(ctx, d['freq'][s], d['I'][s], d['Q'][s], cs['draws'][s], **cs['kw'])
        assert one.tobytes() == whole[s].tobytes() and oq.tobytes() == wq[s].tobytes() and mc.same_bits(oall, wall[s])


def test_device_arg_errors(ctx):
    import torch
    d = mc.synth_mags(2, 16, 3)
    dr = loopfit.mag_draws(2, 3, 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         dict(d_freq=d['freq'], d_i=d['I'], d_q=d['Q'], d_draws=dr).items()}
    fits = torch.full((2 * mc.FIT_DT.itemsize,), 0x5A, dtype=torch.uint8, device='cuda')
    qout = torch.full((2,), -7.0, dtype=torch.float64, device='cuda')
    call = torch.full((2, 3), -7.0, dtype=torch.float64, device='cuda')
    ok = dict(t, nch=2, fsteps=16, n_starts=3, max_iter=5, ftol=1e-6, d_fits=fits, d_qout=qout, d_chisq_all=call)
    torch.cuda.synchronize()
    bad = [dict(d_freq=None), dict(d_i=None), dict(d_q=None), dict(d_draws=None), dict(d_fits=None), dict(nch=0),
           dict(nch=-1), dict(fsteps=11), dict(fsteps=1025), dict(n_starts=0), dict(n_starts=17), dict(max_iter=0),
           dict(ftol=0.0), dict(ftol=-1e-3), dict(ftol=float('nan'))]
    for kw in bad:
        with pytest.raises(_lib.MkidError) as e:
            ctx.fit_mags_device(**{**ok, **kw})
        assert e.value.code == _lib.MKID_E_ARG, kw
    torch.cuda.synchronize()
    assert bool((fits == 0x5A).all()) and bool((qout == -7.0).all()) and bool((call == -7.0).all())   # nothing was launched
    ctx.fit_mags_device(**ok)
    torch.cuda.synchronize()
    assert not bool((fits == 0x5A).all()) and not bool((qout == -7.0).any()) and not bool((call == -7.0).any())


@pytest.mark.parametrize('name', ['loops65', 'special', 'many24'])
def test_chain(ctx, name):
    """Through fit_sweeps the loop results are the bytes of a separate fit_loops call whose qguess is
    the twin's qout, and the magnitude results those of fit_mags alone ('special' has failed channels,
    whose qout is 50000)."""
    cs = mc.case(name)
    d = cs['data']
    nch, S = cs['draws'].shape
    ld = loopfit.draws(nch, S, 17)
    hf, hq, hall = twin(d, cs['draws'], cs['kw'])
    mags, loops = loopfit.fit_sweeps(ctx, d['freq'], d['I'], d['Q'], cs['draws'], ld, **cs['kw'])
    alone = loopfit.fit_mags(ctx, d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    assert set(mags) == set(alone)
    for k in mags:
        assert mags[k].tobytes() == alone[k].tobytes(), k
    mc.check_equal(mags, hf)
    assert mc.same_bits(mags['qout'], hq) and mc.same_bits(mags['chisq_all'], hall)
    sep = loopfit.fit_loops(ctx, d['freq'], d['I'], d['Q'], ld, qguess=hq, **cs['kw'])
    assert set(loops) == set(sep)
    for k in loops:
        assert loops[k].tobytes() == sep[k].tobytes(), k


def test_fit_mags_through_the_shim(gpu):
    """The 64-channel geometry with four resonators on the loop-back feedline of
    tests/test_gpu_loopfit.py, swept by sweepLOready in 24 steps: fitMags() equals the twin on the
    swept I, Q and writes no register; fitLoops(mag_first=True) equals fit_loops(qguess=the twin's
    qout); fitLoops() is what it was. The fitted f0 and Q errors are printed, not asserted."""
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
    I, Q = rs.sweepLOready(1.2e6, 24)

    writes = []
    write_int, write = roach.write_int, roach.write
    roach.write_int = lambda *a, **k: (writes.append(a), write_int(*a, **k))[1]
    roach.write = lambda *a, **k: (writes.append(a[:1]), write(*a, **k))[1]
    centres, regs = rs.iq_centers.copy(), dict(roach.regs)
    x = np.asarray(rs.f_span, np.float64)
    kw = dict(max_iter=200, ftol=1e-10)

    out = rs.fitMags()
    assert out is rs.mag_fits and writes == [] and dict(roach.regs) == regs and np.array_equal(rs.iq_centers, centres)
    assert not hasattr(rs, 'loop_fits')
    rc, hf, hq, hall = mc.fit_host(x, I, Q, loopfit.mag_draws(4, 10, 0), **kw)
    assert rc == 0
    mc.check_equal(out, hf)
    assert mc.same_bits(out['qout'], hq) and mc.same_bits(out['chisq_all'], hall)
    f0 = np.array([r['f0'] for r in res])
    print('shim: status', out['status'], 'magnitude fit f0 errors in linewidths', np.abs(out['p'][:, 1] - f0) / (f0 / 2.0e4),
          'Q errors', out['p'][:, 0] / 2.0e4 - 1.0)

    ch = roach.channelizer()
    plain = {k: v.copy() for k, v in rs.fitLoops().items()}
    sep0 = loopfit.fit_loops(ch, x, I, Q, loopfit.draws(4, 10, 0), **kw)
    for k in plain:
        assert plain[k].tobytes() == sep0[k].tobytes(), k                       # the default path is what it was
    chained = rs.fitLoops(mag_first=True)
    assert chained is rs.loop_fits and writes == [] and dict(roach.regs) == regs and np.array_equal(rs.iq_centers, centres)
    sep = loopfit.fit_loops(ch, x, I, Q, loopfit.draws(4, 10, 0), qguess=hq, **kw)
    for k in chained:
        assert chained[k].tobytes() == sep[k].tobytes(), k
    mc.check_equal(rs.mag_fits, hf)
    print('shim: chained loop fit f0 errors in linewidths', np.abs(chained['p'][:, 1] - f0) / (f0 / 2.0e4), 'Q errors',
          chained['p'][:, 0] / 2.0e4 - 1.0, '; ladder Q errors', plain['p'][:, 0] / 2.0e4 - 1.0)
