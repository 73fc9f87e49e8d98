"""mkid_fit_mags_host (the loops of csrc/magfit_common.h, no device) against the float64 restatement
of tests/magfit_cases.py: every integer and every float bit for bit over the case table, with
d_chisq_all and d_qout present and absent; the restatement's own Jacobian and model against
independent statements; the MKID_E_ARG cases; chunk invariance; the d_qout rule; the recovery of
model-generated sweeps; and the host-side pieces of loopfit.py (internal_power, the .swp files).

Recovery, measured with RECOVERY_SEED (65 sweeps generated from the model, 100 steps, S = 10,
max_iter = 200; the twin is bit-identical to the restatement, so these are its figures too):
  without noise   worst Q error 1.11e-15 relative, f0 recovered exactly in all 65 (bars: 1.2e-14
                  and 10 ulp of f0: ten times the figure, and ten times the one ulp below which an
                  error of 0 was measured);
  0.1 % noise     worst Q error 0.592 %, worst f0 error 6.3e-4 of a linewidth (bars: 6 % and 6.3e-3
                  linewidths, ten times the figures, for the choice of seed). Seeds 2, 3 and 4 gave
                  0.70 %, 0.51 %, 0.60 % and 7.1e-4, 1.1e-3, 7.2e-4.
These are magnitudes drawn from the magnitude model itself. On loops whose centre lies off the
origin (loopfit_cases.synth_loops) the magnitude fit's Q is 0.18 .. 0.71 of the loop's, which is the
reference's model on such loops; the chain into the loop fit is tested for identity only.
"""
import numpy as np
import pytest

import loopfit_cases as lc
import magfit_cases as mc
from mkids_sdr_amd import _lib, loopfit

EPS = np.finfo(np.float64).eps
RECOVERY_SEED = 1


@pytest.mark.parametrize('name', list(mc.CASES))
def test_host_twin_equals_restatement(name):
    cs = mc.case(name)
    d = cs['data']
    ref, rq, rcall = cs['ref']
    rc, fits, qout, call = mc.fit_host(d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    assert rc == 0
    mc.check_equal(fits, ref)
    assert mc.same_bits(qout, rq) and mc.same_bits(call, rcall)
    for want_all, want_q in ((False, True), (True, False), (False, False)):     # both are optional
        rc, f2, q2, c2 = mc.fit_host(d['freq'], d['I'], d['Q'], cs['draws'], want_all=want_all, want_q=want_q, **cs['kw'])
        assert rc == 0 and f2.tobytes() == fits.tobytes()
        assert (c2 is None) if not want_all else mc.same_bits(c2, call)
        assert (q2 is None) if not want_q else mc.same_bits(q2, qout)


def test_result_layout():
    import ctypes
    assert ctypes.sizeof(_lib.MagFit) == 80 == mc.FIT_DT.itemsize
    assert [mc.FIT_DT.fields[k][1] for k in ('p', 'chisq', 'norm', 'cidx', 'best_start', 'evals', 'status')] == \
        [0, 48, 56, 64, 68, 72, 76]
    for name, *_ in _lib.MagFit._fields_:
        assert getattr(_lib.MagFit, name).offset == mc.FIT_DT.fields[name][1]


def test_table_covers_its_paths():
    """What the table is there for: the status bits, a fixed parameter, the cusp, both ways a start
    ends, every lane shape."""
    st = {n: mc.case(n)['ref'][0] for n in mc.CASES}
    assert list(st['special']['status'][:2]) == [_lib.LOOP_FLAT, _lib.LOOP_NONFINITE]
    assert st['special']['norm'][0] == 0.0 and np.isfinite(st['special']['norm'][1])
    assert st['special']['status'][2] == 0 and st['nofit']['status'][0] == _lib.LOOP_NO_FIT
    assert np.all(np.isfinite(mc.case('nofit')['data']['I']))
    for k in ('special', 'nofit'):
        bad = st[k]['status'] & mc.FAIL_BITS != 0
        assert np.all(np.isnan(st[k]['p'][bad])) and np.all(np.isnan(st[k]['chisq'][bad]))
        assert np.all(st[k]['best_start'][bad] == -1) and np.all(st[k]['evals'][bad] == 0)
        assert np.all(mc.case(k)['ref'][1][bad] == mc.Q_FAIL)
    assert st['samefreq']['p'][0, 1] == 5.0e9 and st['samefreq']['status'][0] == 0
    d = mc.case('cusp')['data']
    x = d['freq'][0]
    _, lo, hi, f0 = mc.problem_ref(x, False, 1.0)
    assert len(x) % 2 == 1 and f0 == x[len(x) // 2] and lo[1] < f0 < hi[1]
    J = mc.terms_ref(mc.start_ref(lo, hi, f0, 0, 0.0), x, np.ones_like(x))[2]
    assert J[0, len(x) // 2] == 0.0 and J[1, len(x) // 2] != 0.0 and np.all(np.delete(J[0], len(x) // 2) != 0.0)   # sg = 0 there only
    status = np.concatenate([s['status'] for s in st.values()])
    assert np.any(status == 0) and np.any(status == _lib.LOOP_MAX_ITER)
    shapes = {(mc.case(n)['data']['freq'].shape, mc.case(n)['draws'].shape[1]) for n in mc.CASES}
    assert {s[0][0] for s in shapes} >= {1, 3, 65} and {s[0][1] for s in shapes} >= {12, 13, 64, 65, 129, 1024}
    assert {s[1] for s in shapes} >= {1, 5, 10, 16}
    assert sum(mc.case(n)['data']['truth'] is None for n in mc.CASES) >= 4      # loops and model sets alike


def test_jacobian_against_central_differences():
    """J of the restatement (w = 1) against central differences of its own model, away from the cusp
    (no sample within 1e-3 linewidths of f0). Steps h: 1e-6 Q, 1e-9 f0 (5 Hz of a 100 kHz linewidth),
    1e-6 in carrier and depth, 1e-2 in slope, 1e3 in curve (the model is linear in the last four).
    The truncation error is h^2 / 6 of the third derivative: through t = 2 Q dx a step in Q moves t by
    1e-6 t (|t| <= 8) and a step in f0 by 2 Q 1e-9 <= 1.6e-4, and |a'''| <= 3 against max |a'| = 1, so
    at the most (1.6e-4)^2 / 6 x 3 = 1.3e-8 of the column's largest entry; the rounding error of the two
    model values, each within 8 ulp of the model's size, is 16 x 2^-52 max|model| / 2h. The bar is
    1e-7 of the column's largest entry plus that."""
    d = mc.synth_mags(3, 40, 77)
    for c in range(3):
        p = d['truth'][c].tolist()
        x = d['freq'][c]
        assert np.abs(x - p[1]).min() > 1e-3 * p[1] / p[0]
        J = mc.terms_ref(p, x, np.ones_like(x), w=1.0)[2]
        size = np.abs(mc.model_ref(p, x)).max()
        h = [1e-6 * p[0], 1e-9 * p[1], 1e-6, 1e-6, 1e-2, 1e3]
        for k in range(6):
            up, dn = list(p), list(p)
            up[k], dn[k] = p[k] + h[k], p[k] - h[k]
            num = (mc.model_ref(up, x) - mc.model_ref(dn, x)) / (up[k] - dn[k])
            scale = np.abs(J[k]).max()
            bar = 1e-7 * scale + 16 * EPS * size / (2 * h[k])
            assert bar <= 1e-4 * scale, (c, k)      # the check means something in every column
            assert np.abs(J[k] - num).max() <= bar, (c, k, np.abs(J[k] - num).max() / scale)


def test_model_equals_magdiff():
    """mag_model and the restatement's model against the reference's complex expression
    (lib/iqsweep.py:913-917), abs(2jQdx / (1 + 2jQdx)): the same function by another route (a complex
    division and a hypot against |t| / sqrt(1 + t^2)), each a few roundings of terms no larger than
    |depth| + |carrier| + max|slope dx| + max|curve dx^2|: within 16 ulp of that size."""
    d = mc.synth_mags(5, 50, 9)
    for c in range(5):
        p = d['truth'][c]
        x = d['freq'][c]
        Q, f0, carrier, depth, slope, curve = p
        dx = (x - f0) / f0
        s21 = (1j * 2.0 * Q * dx) / (1.0 + 1j * 2.0 * Q * dx)
        want = (np.abs(s21) - 1.0) * depth + carrier + slope * dx + curve * dx * dx
        size = abs(depth) + abs(carrier) + np.abs(slope * dx).max() + np.abs(curve * dx * dx).max()
        got = loopfit.mag_model(p, x)
        assert np.abs(got - want).max() <= 16 * EPS * size
        assert np.array_equal(got, mc.model_ref(p, x))


def test_arg_errors():
    d = mc.synth_mags(2, 16, 3)
    dr = loopfit.mag_draws(2, 3, 0)
    call = lambda **kw: mc.fit_host(d['freq'], d['I'], d['Q'], dr, **{**dict(max_iter=5, ftol=1e-6), **kw})
    assert call()[0] == 0
    assert call(null=('qout',))[0] == 0 and call(null=('call',))[0] == 0 and call(null=('qout', 'call'))[0] == 0
    bad = [dict(null=(n,)) for n in ('freq', 'i', 'q', 'draws', 'fits')]
    bad += [dict(nch=0), dict(nch=-1), dict(fsteps=11), dict(fsteps=1025), dict(S=0), dict(S=17), dict(max_iter=0),
            dict(max_iter=-3), dict(ftol=0.0), dict(ftol=-1e-3), dict(ftol=float('nan'))]
    for kw in bad:
        rc, fits, qout, chis = call(**kw)
        assert rc == _lib.MKID_E_ARG, kw
        assert fits.tobytes() == b'\x5a' * fits.nbytes and np.all(qout == -7.0) and np.all(chis == -7.0), kw
    with pytest.raises(ValueError):
        loopfit.fit_mags_host(d['freq'], d['I'], d['Q'][:, :5], dr)
    with pytest.raises(ValueError):
        loopfit.fit_mags_host(d['freq'], d['I'], d['Q'], dr[:1])
    with pytest.raises(_lib.MkidError):
        loopfit.fit_mags_host(d['freq'], d['I'], d['Q'], dr, max_iter=0)


def test_chunk_invariance():
    """A channel fitted alone equals the same channel among 65, bit for bit."""
    cs = mc.case('many24')
    d = cs['data']
    _, whole, wq, wall = mc.fit_host(d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    for c in range(65):
        s = slice(c, c + 1)
        rc, one, oq, oall = mc.fit_host(d['freq'][s], d['I'][s], d['Q'][s], cs['draws'][s], **cs['kw'])
        assert rc == 0 and one.tobytes() == whole[s].tobytes() and mc.same_bits(oall, wall[s]) and mc.same_bits(oq, wq[s])


def test_qout_rule():
    """d_qout is p[0] of a fitted channel and 50000.0 of a channel with a fail bit: always a valid
    qguess of the loop fit."""
    for name in ('special', 'nofit', 'many24', 'loops65'):
        cs = mc.case(name)
        d = cs['data']
        _, fits, qout, _ = mc.fit_host(d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
        bad = fits['status'] & mc.FAIL_BITS != 0
        assert np.all(qout[bad] == 50000.0) and mc.same_bits(qout[~bad], fits['p'][~bad, 0])
        assert np.all(np.isfinite(qout)) and np.all((qout >= 5e3) & (qout <= 1e6))
    assert np.any(mc.case('special')['ref'][0]['status'] & mc.FAIL_BITS != 0)


def test_python_layer():
    """loopfit.fit_mags_host returns the twin's arrays by field; mag_draws() is a pure function of its
    seed."""
    cs = mc.case('loops65')
    d = cs['data']
    out = loopfit.fit_mags_host(d['freq'], d['I'], d['Q'], cs['draws'], **cs['kw'])
    assert set(out) == set(loopfit.MAG_FIELDS) | {'qout', 'chisq_all'} and len(loopfit.MAG_PARAMS) == _lib.MAG_NPAR
    mc.check_equal(out, cs['ref'][0])
    assert mc.same_bits(out['qout'], cs['ref'][1]) and mc.same_bits(out['chisq_all'], cs['ref'][2])
    a, b = loopfit.mag_draws(7, 16, 3), loopfit.mag_draws(7, 16, 3)
    assert a.shape == (7, 16) and a.dtype == np.float64 and a.tobytes() == b.tobytes()
    assert a.tobytes() != loopfit.mag_draws(7, 16, 4).tobytes()


# ---- recovery -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('noise', [0.0, 1e-3])
def test_recovery_of_model_generated_sweeps(noise):
    """The module docstring's figures and bars."""
    d = mc.synth_mags(65, 100, RECOVERY_SEED, noise=noise)
    dr = loopfit.mag_draws(65, 10, RECOVERY_SEED)
    rc, fits, qout, call = mc.fit_host(d['freq'], d['I'], d['Q'], dr, max_iter=200, ftol=mc.FTOL)
    assert rc == 0 and np.all(fits['status'] == 0)
    s = slice(0, 65, 16)        # the restatement is the twin here as well
    ref, rq, rcall = mc.fit_ref(d['freq'][s], d['I'][s], d['Q'][s], dr[s], max_iter=200, ftol=mc.FTOL)
    mc.check_equal(fits[s], ref)
    tr = d['truth']
    q_err = np.abs(fits['p'][:, 0] / tr[:, 0] - 1.0)
    f_ulp = np.abs(fits['p'][:, 1] - tr[:, 1]) / (EPS * tr[:, 1])
    f_lw = np.abs(fits['p'][:, 1] - tr[:, 1]) / (tr[:, 1] / tr[:, 0])
    print('noise %g: Q error %.3g, f0 error %.3g ulp, %.3g linewidths' % (noise, q_err.max(), f_ulp.max(), f_lw.max()))
    if noise == 0.0:
        assert q_err.max() <= 1.2e-14 and f_ulp.max() <= 10.0
    else:
        assert q_err.max() <= 0.06 and f_lw.max() <= 6.3e-3
    # the winner is the lowest of the starts' chi^2
    assert np.array_equal(fits['best_start'], np.argmin(call, axis=1)) and mc.same_bits(fits['chisq'], call.min(1))


# ---- Pint and the .swp files ----------------------------------------------------------------------------
def test_internal_power():
    """The reference's expression (lib/iqsweep.py:275-276) on the loop fit's Q and Qc."""
    d = lc.synth_loops(3, 40, 21)
    fits = loopfit.fit_loops_host(d['freq'], d['I'], d['Q'], loopfit.draws(3, 4, 0))
    assert np.all(fits['status'] & lc.FAIL_BITS == 0)
    for atten1 in (0.0, 13.0, np.array([3.0, 10.0, 20.0])):
        power = 10.0 ** ((-atten1 - 35.0) / 10.0)
        want = 10.0 * np.log10((2.0 * fits['p'][:, 0] ** 2 / (np.pi * fits['qc'])) * power)
        got = loopfit.internal_power(fits, atten1)
        assert got.shape == (3,) and np.all(np.isfinite(got)) and np.allclose(got, want, rtol=1e-14, atol=0.0)
    assert np.allclose(loopfit.internal_power(fits, 10.0) - loopfit.internal_power(fits, 0.0), -10.0, rtol=1e-12)


def test_swp_round_trip(tmp_path):
    """save_swp -> load_swp returns the arrays exactly: two resonators of different lengths, one with
    a zero point of 0 and arbitrary floats, one with integer data and a non-zero zero point."""
    rng = np.random.default_rng(5)
    a = lc.synth_loops(1, 37, 11, sd=True)
    r0 = dict(freq=a['freq'][0], I=a['I'][0], Q=a['Q'][0], Isd=a['isd'][0], Qsd=a['qsd'][0])
    n1 = 24
    r1 = dict(freq=4.0e9 + np.cumsum(rng.uniform(1e3, 5e4, n1)), I=np.rint(rng.normal(0, 2e4, n1)),
              Q=np.rint(rng.normal(0, 2e4, n1)), Isd=rng.uniform(1, 30, n1), Qsd=rng.uniform(1, 30, n1), I0=-312.0,
              Q0=977.0, I0sd=1.5, Q0sd=2.25)
    path = str(tmp_path / 'two.swp')
    loopfit.save_swp(path, r0, r1, atten1=12.0, atten2=7.5, tstart=0.101, tend=0.099)
    for k, r in enumerate((r0, r1)):
        got = loopfit.load_swp(path, k)
        for f in ('freq', 'I', 'Q', 'Isd', 'Qsd'):
            assert got[f].dtype == np.float64 and got[f].tobytes() == np.asarray(r[f], np.float64).tobytes(), (k, f)
        assert got['fsteps'] == len(r['freq']) and got['atten1'] == 12.0 and got['atten2'] == 7.5
        assert (got['I0'], got['Q0'], got['I0sd'], got['Q0sd']) == (r.get('I0', 0.0), r.get('Q0', 0.0),
                                                                    r.get('I0sd', 0.0), r.get('Q0sd', 0.0))
        assert (got['Tstart'], got['Tend']) == (0.101, 0.099)
    one = str(tmp_path / 'one.swp')
    loopfit.save_swp(one, r0, atten1=3.0)
    assert loopfit.load_swp(one)['freq'].tobytes() == r0['freq'].tobytes() and loopfit.load_swp(one, 1)['fsteps'] == 0
    with pytest.raises(ValueError):
        loopfit.load_swp(one, 2)


def test_swp_hand_written_file(tmp_path):
    """A file in LoadSWP's layout (lib/iqsweep.py:97-139): seven header lines, one five-column table,
    resonator 1 starting at row h3 = resonator 0's step count, frequencies in GHz."""
    text = ('4.5\t0.002\t3\t14\n'
            '5.25\t0.004\t2\t6\n'
            '0.1\t0.102\n'
            '100\t1.5\n'
            '-50\t2.5\n'
            '7\t0.5\n'
            '9\t0.25\n'
            '4.499\t1100\t3\t-40\t4\n'
            '4.5000125\t1200.5\t3.5\t-45\t4.5\n'
            '4.501\t1300\t5\t-60\t6\n'
            '5.248\t17\t1\t19\t2\n'
            '5.252\t27.25\t1.25\t-1\t2.5\n')
    path = tmp_path / 'hand.swp'
    path.write_text(text)
    r0, r1 = loopfit.load_swp(str(path), 0), loopfit.load_swp(str(path), 1)
    assert np.array_equal(r0['freq'], [4.499e9, 4500012500.0, 4.501e9]) and np.array_equal(r1['freq'], [5.248e9, 5.252e9])
    assert np.array_equal(r0['I'], [1000.0, 1100.5, 1200.0]) and np.array_equal(r0['Q'], [10.0, 5.0, -10.0])
    assert np.array_equal(r0['Isd'], [3.0, 3.5, 5.0]) and np.array_equal(r0['Qsd'], [4.0, 4.5, 6.0])
    assert np.array_equal(r1['I'], [10.0, 20.25]) and np.array_equal(r1['Q'], [10.0, -10.0])
    assert np.array_equal(r1['Isd'], [1.0, 1.25]) and np.array_equal(r1['Qsd'], [2.0, 2.5])
    assert (r0['atten1'], r0['atten2'], r1['atten1']) == (14.0, 6.0, 14.0)
    assert (r0['f0'], r0['span'], r0['fsteps'], r1['f0'], r1['span'], r1['fsteps']) == (4.5, 0.002, 3, 5.25, 0.004, 2)
    assert (r0['I0'], r0['Q0'], r1['I0'], r1['Q0']) == (100.0, -50.0, 7.0, 9.0)
    assert (r0['Tstart'], r0['Tend']) == (0.1, 0.102)
    short = tmp_path / 'short.swp'
    short.write_text(text.rsplit('\n', 2)[0] + '\n')       # resonator 1 lacks a row
    with pytest.raises(ValueError):
        loopfit.load_swp(str(short), 1)
