"""mkid_pulse_fit on the device (k_heights_fit.hip) against tests/fit_ref.py, the float64 restatement.

The case table sits around the lane map's boundaries (2 L + 1 in {1, 3, 5, 7, 17, 63}, ncoeff around
multiples of 64 and of G = 64 // (2 L + 1)), each case at both polarities, with the error bars of
fit_ref.check_against: fp32 accumulation of n products in any order is within n 2^-24 sum |c x| of
the exact sum, floored at the project's 1e-5 for at most 128 products. Then: the exact integer case,
chunking (one call, four calls, 1-row calls: bit-identical), independence of a packet's place and
neighbours, the counted form, mkid_pulse_heights left as it was, the device filter handoff, the
state and argument errors and the nullable outputs. Everything works on uploaded arrays.
"""
import ctypes

import numpy as np
import pytest

import fit_ref
from mkids_sdr_amd import _lib

C = fit_ref.C_TEST
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(C, max_chunk=2 ** 14)
    yield ch
    ch.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    torch.cuda.synchronize()     # torch's stream made it, the context's stream reads it
    return t


def _outputs(n, fill=None):
    import torch
    mk = lambda dt, v: torch.empty(n, dtype=dt, device='cuda') if v is None else torch.full((n,), v, dtype=dt, device='cuda')
    f = None if fill is None else float(fill)
    outs = [mk(torch.float32, f), mk(torch.float32, f), mk(torch.int32, None if fill is None else int(fill)),
            mk(torch.float32, f)]
    torch.cuda.synchronize()     # the fills ran on torch's stream
    return outs


def _host(outs):
    import torch
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _same(a, b):
    """Bit-identical outputs (four arrays each), NaN payloads included."""
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize('s', [1, -1])
@pytest.mark.parametrize('ncoeff,pre,L', fit_ref.CASES)
def test_fit_case_table(ctx, ncoeff, pre, L, s):
    phase, coeff, ev = fit_ref.inputs(ncoeff, pre, L)
    ref = fit_ref.reference(ncoeff, pre, L, s)
    ctx.set_pulse_filter(coeff, pre)
    ctx.set_pulse_fit(L, s)
    got = ctx.pulse_fit(phase, ev)
    interior, skipped = fit_ref.check_against(ref, got, fit_ref.bar32(ref[5], ncoeff), L, s)
    print('ncoeff %d L %d s %+d: %d interior packets, %d below 16 bar' % (ncoeff, L, s, interior, skipped))


def test_fit_exact_case(ctx):
    """Integer inputs: every lag value is exact in fp32, so lag and h0 equal the restatement bit for
    bit and height and dt differ by the rounding of one division and one sum."""
    ph4, cf4, ev, pre, L = fit_ref.exact_case()
    phase = np.zeros((ph4.shape[0], C), np.float32)
    phase[:, :4] = ph4
    coeff = np.zeros((C, cf4.shape[1]), np.float32)
    coeff[:4] = cf4
    ctx.set_pulse_filter(coeff, pre)
    for s in (1, -1):
        ctx.set_pulse_fit(L, s)
        h, dt, lag, h0 = ctx.pulse_fit(phase, ev)
        rh, rdt, rlag, rh0, H, _ = fit_ref.pulse_fit(phase, ev, coeff, pre, L, s)
        assert np.array_equal(lag, rlag)
        assert np.array_equal(h0.astype(np.float64), rh0, equal_nan=True)
        ok = ~np.isnan(rh)
        assert ok.sum() > 200 and np.array_equal(np.isnan(h), ~ok) and np.array_equal(np.isnan(dt), ~ok)
        Hk = H[ok, rlag[ok] + L]
        half_ulp = 2.0 ** -24
        assert np.all(np.abs(h[ok] - rh[ok]) <= half_ulp * (np.abs(rh[ok]) + np.abs(rh[ok] - Hk)))
        assert np.all(np.abs(dt[ok] - rdt[ok]) <= half_ulp * (np.abs(rdt[ok]) + np.abs(rdt[ok] - rlag[ok])))


NCO, PRE, LS, SS = 100, 20, 3, -1


def _stream(seed=3, rows=1200, n=1500):
    rng = np.random.default_rng(seed)
    phase = rng.normal(size=(rows, C)).astype(np.float32)
    coeff = rng.normal(size=(C, NCO)).astype(np.float32)
    ts = np.sort(rng.integers(0, rows, n))
    ev = np.array([fit_ref.pack(c, t) for c, t in zip(rng.integers(0, C, n), ts)], np.uint64)
    return phase, coeff, ev, ts


def _one_call(ctx, d_phase, rows, j0, ev):
    outs = _outputs(max(len(ev), 1))
    ctx.pulse_fit_device(d_phase, rows, j0, _dev(ev) if len(ev) else None, len(ev), *outs)
    return [o[:len(ev)] for o in _host(outs)]


def test_fit_chunking(ctx):
    """4 x 300 rows as one call, as four calls with the deferred packets passed again, and the first
    400 rows as 1-row calls: every packet's outputs are the same bits. A call that does not continue
    the previous one, or that follows either setter, has no carried rows."""
    import torch
    phase, coeff, ev, ts = _stream()
    d_phase = _dev(phase)
    ctx.set_pulse_filter(coeff, PRE)
    ctx.set_pulse_fit(LS, SS)
    torch.cuda.synchronize()
    whole = _one_call(ctx, d_phase, 1200, 0, ev)
    ref = fit_ref.pulse_fit(phase, ev, coeff, PRE, LS, SS)
    fit_ref.check_against(ref, whole, fit_ref.bar32(ref[5], NCO), LS, SS)
    # four contiguous calls
    ctx.set_pulse_fit(LS, SS)
    parts = [np.full(len(ev), np.nan, np.float32), np.full(len(ev), np.nan, np.float32),
             np.full(len(ev), fit_ref.NO_LAG, np.int32), np.full(len(ev), np.nan, np.float32)]
    deferred = np.zeros(0, np.int64)
    for k in range(4):
        idx = np.concatenate([deferred, np.flatnonzero((ts >= 300 * k) & (ts < 300 * (k + 1)))])
        got = _one_call(ctx, d_phase[300 * k:300 * (k + 1)], 300, 300 * k, ev[idx])
        tail = ts[idx] - PRE + NCO + LS > 300 * (k + 1)
        early = ts[idx] - PRE - LS < 0
        assert np.array_equal(np.isnan(got[0]), tail | early)           # deferral: the call's last rows
        assert np.all(ts[idx][tail] >= 300 * (k + 1) - (NCO - PRE + LS))
        for dst, g in zip(parts, got):
            dst[idx[~tail]] = g[~tail]
        deferred = idx[tail]
    assert deferred.size > 5
    late = ts - PRE + NCO + LS > 1200                                   # never completed in the stream
    assert np.array_equal(np.flatnonzero(late), np.sort(deferred))
    assert _same([w[~late] for w in whole], [p[~late] for p in parts])
    # 1-row calls over the first 400 rows: a packet is passed with the row that completes its window
    ctx.set_pulse_fit(LS, SS)
    end = ts - PRE + NCO + LS - 1
    order = np.argsort(end, kind='stable')
    d_ev = _dev(ev[order])
    outs = _outputs(len(ev), fill=-7)
    lo = np.searchsorted(end[order], np.arange(401))
    for j in range(400):
        a, b = int(lo[j]), int(lo[j + 1])
        ctx.pulse_fit_device(d_phase[j:j + 1], 1, j, d_ev[a:] if b > a else None, b - a, *[o[a:] for o in outs])
    rowwise = _host(outs)
    done = order[:int(lo[400])]
    assert done.size > 300
    assert _same([w[done] for w in whole], [r[:done.size] for r in rowwise])
    assert np.all(rowwise[2][done.size:] == -7)
    # no carried rows: after a gap in j0, after mkid_set_pulse_fit, after mkid_set_pulse_filter
    mid = np.flatnonzero((ts >= 600) & (ts < 900))
    fresh = (ts[mid] - PRE - LS < 600) | (ts[mid] - PRE + NCO + LS > 900)
    assert (ts[mid] - PRE - LS < 600).sum() > 5
    _one_call(ctx, d_phase[:300], 300, 0, ev[:0])
    assert np.array_equal(np.isnan(_one_call(ctx, d_phase[600:900], 300, 600, ev[mid])[0]), fresh)
    for setter in (lambda: ctx.set_pulse_fit(LS, SS), lambda: ctx.set_pulse_filter(coeff, PRE)):
        _one_call(ctx, d_phase[300:600], 300, 300, ev[:0])
        carried = _one_call(ctx, d_phase[600:900], 300, 600, ev[mid])
        _one_call(ctx, d_phase[300:600], 300, 300, ev[:0])
        setter()
        cut = _one_call(ctx, d_phase[600:900], 300, 600, ev[mid])
        assert np.array_equal(np.isnan(carried[0]), ts[mid] - PRE + NCO + LS > 900)
        assert np.array_equal(np.isnan(cut[0]), fresh)
        assert _same([c[~fresh] for c in carried], [c[~fresh] for c in cut])


def test_fit_independence(ctx):
    """A packet's outputs do not depend on its place in the list, its neighbours, n or the grid, and
    a second run repeats the first bit for bit."""
    phase, coeff, ev, ts = _stream(seed=4)
    d_phase = _dev(phase)
    ctx.set_pulse_filter(coeff, PRE)
    ctx.set_pulse_fit(LS, SS)
    first = _one_call(ctx, d_phase, 1200, 0, ev)
    ctx.set_pulse_fit(LS, SS)
    assert _same(first, _one_call(ctx, d_phase, 1200, 0, ev))
    rng = np.random.default_rng(9)
    perm = rng.permutation(len(ev))
    ctx.set_pulse_fit(LS, SS)
    shuffled = _one_call(ctx, d_phase, 1200, 0, ev[perm])
    assert _same([f[perm] for f in first], shuffled)
    n = 10 * len(ev)
    big = np.array([fit_ref.pack(c, t) for c, t in zip(rng.integers(0, C + 8, n), rng.integers(0, 1300, n))], np.uint64)
    at = np.sort(rng.choice(n, len(ev), replace=False))
    big[at] = ev
    ctx.set_pulse_fit(LS, SS)
    embedded = _one_call(ctx, d_phase, 1200, 0, big)
    assert _same(first, [e[at] for e in embedded])


def test_fit_counted(ctx):
    """The counted form processes min(max(*d_count, 0), cap) packets and leaves the other outputs alone."""
    import torch
    phase, coeff, ev, ts = _stream(seed=5, n=600)
    d_phase, d_ev = _dev(phase), _dev(ev)
    ctx.set_pulse_filter(coeff, PRE)
    ctx.set_pulse_fit(LS, SS)
    whole = _one_call(ctx, d_phase, 1200, 0, ev)
    cap = 400
    for count in (-1, 0, 250, 400, 600):
        d_count = torch.tensor([count], dtype=torch.int64, device='cuda')
        outs = _outputs(len(ev), fill=-7)
        torch.cuda.synchronize()
        ctx.set_pulse_fit(LS, SS)
        ctx.pulse_fit_counted(d_phase, 1200, 0, d_ev, d_count, cap, *outs)
        got = _host(outs)
        m = min(max(count, 0), cap)
        assert _same([w[:m] for w in whole], [g[:m] for g in got])
        assert all(np.all(g[m:] == -7) for g in got)


def test_heights_unchanged_by_fit(gpu):
    """mkid_pulse_heights on a context that also runs the fit on the same rows of a two-call stream
    gives the bits, NaN pattern included, of a context that never heard of the fit."""
    from mkids_sdr_amd.channelizer import Channelizer
    phase, coeff, ev, ts = _stream(seed=6)
    d_phase = _dev(phase)
    res = {}
    for with_fit in (False, True):
        ch = Channelizer(C, max_chunk=2 ** 14)
        try:
            if with_fit:
                ch.set_pulse_fit(LS, SS)
            ch.set_pulse_filter(coeff, PRE)
            got = []
            for k in range(2):
                idx = np.flatnonzero((ts >= 600 * k - 50) & (ts < 600 * (k + 1)))
                d_e = _dev(ev[idx])
                d_h = _outputs(len(idx))[0]
                if with_fit:
                    ch.pulse_fit_device(d_phase[600 * k:600 * (k + 1)], 600, 600 * k, d_e, len(idx), *_outputs(len(idx)))
                ch.pulse_heights_device(d_phase[600 * k:600 * (k + 1)], 600, 600 * k, d_e, len(idx), d_h)
                got.append(_host([d_h])[0])
            res[with_fit] = got
        finally:
            ch.close()
    for a, b in zip(res[False], res[True]):
        assert np.isnan(a).sum() > 5 and np.isfinite(a).sum() > 500
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    early = ts[(ts >= 550) & (ts < 1200)] - PRE < 600          # windows reaching into the first call
    assert np.all(np.isfinite(res[True][1][early])) and early.sum() > 5


def test_filter_device_handoff(ctx):
    """set_pulse_filter_device(d_coeff) then pulse_heights equals set_pulse_filter(d_coeff.cpu())."""
    phase, coeff, ev, ts = _stream(seed=7)
    d_phase, d_ev, d_coeff = _dev(phase), _dev(ev), _dev(coeff)
    got = []
    for device in (True, False):
        if device:
            ctx.set_pulse_filter_device(d_coeff, PRE)
        else:
            ctx.set_pulse_filter(d_coeff.cpu().numpy(), PRE)
        d_h = _outputs(len(ev))[0]
        ctx.pulse_heights_device(d_phase, 1200, 0, d_ev, len(ev), d_h)
        got.append(_host([d_h])[0])
    assert np.isfinite(got[0]).sum() > 1000
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))


def test_filters_from_bank_device_load(ctx):
    """load=True hands the bank call's table to set_pulse_filter_device where it lies: on a bank
    with too few records every channel keeps the fallback, and the heights under the loaded table
    equal those under set_pulse_filter(fallback, pre=10)."""
    import torch
    from mkids_sdr_amd import template
    phase, coeff, ev, ts = _stream(seed=11)
    d_phase, d_ev = _dev(phase), _dev(ev)
    bank = (torch.zeros((C, 2, template.NPTS), dtype=torch.float32, device='cuda'),
            torch.zeros((C, 2), dtype=torch.int64, device='cuda'), torch.ones((C, 2), dtype=torch.int32, device='cuda'))
    torch.cuda.synchronize()
    got = []
    for load in (True, False):
        f = template.filters_from_bank_device(ctx, bank, ncoeff=NCO, min_records=20, fallback=coeff, load=load)
        assert not f['used'].any() and np.array_equal(f['coeff'], coeff)
        if not load:
            ctx.set_pulse_filter(f['coeff'], pre=10)
        d_h = _outputs(len(ev))[0]
        ctx.pulse_heights_device(d_phase, 1200, 0, d_ev, len(ev), d_h)
        got.append(_host([d_h])[0])
    assert np.isfinite(got[0]).sum() > 1000
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))


def _code(fn):
    with pytest.raises(_lib.MkidError) as e:
        fn()
    return e.value.code


def test_fit_state_and_argument_errors(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    phase, coeff, ev, ts = _stream(seed=8, rows=300, n=50)
    d_phase, d_ev, d_coeff = _dev(phase), _dev(ev), _dev(coeff)
    outs = _outputs(len(ev))
    d_count = _dev(np.array([10], np.int64))
    ch = Channelizer(C, max_chunk=2 ** 14)
    try:
        fit = lambda **kw: ch.pulse_fit_device(*[kw.get(k, v) for k, v in (
            ('phase', d_phase), ('rows', 300), ('j0', 0), ('events', d_ev), ('n', len(ev)), ('heights', outs[0]),
            ('dt', outs[1]), ('lag', outs[2]), ('h0', outs[3]))])
        assert _code(fit) == _lib.MKID_E_STATE                      # neither setter
        ch.set_pulse_fit(LS, SS)
        assert _code(fit) == _lib.MKID_E_STATE                      # no filter
        for bad in ((-1, 1), (32, 1), (3, 0), (3, 2), (3, -2)):
            assert _code(lambda: ch.set_pulse_fit(*bad)) == _lib.MKID_E_ARG
        L, h = ch._L, ch._h
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert L.mkid_set_pulse_fit(None, 3, 1) == _lib.MKID_E_ARG
        for args in ((None, C, NCO, PRE), (p(d_coeff), C - 1, NCO, PRE), (p(d_coeff), C, 0, PRE),
                     (p(d_coeff), C, 4097, PRE), (p(d_coeff), C, NCO, -1)):
            assert L.mkid_set_pulse_filter_device(h, *args) == _lib.MKID_E_ARG
        assert L.mkid_set_pulse_filter_device(None, p(d_coeff), C, NCO, PRE) == _lib.MKID_E_ARG
        ch.set_pulse_filter_device(d_coeff, PRE)
        fit()
        fit(rows=0, phase=None)
        fit(n=0, events=None, heights=None)
        for kw in (dict(phase=None), dict(events=None), dict(heights=None), dict(rows=-1), dict(j0=-1), dict(n=-1)):
            assert _code(lambda: fit(**kw)) == _lib.MKID_E_ARG, kw
        assert _code(lambda: ch.pulse_fit_counted(d_phase, 300, 0, d_ev, None, 10, *outs)) == _lib.MKID_E_ARG
        assert _code(lambda: ch.pulse_fit_counted(d_phase, 300, 0, d_ev, d_count, -1, *outs)) == _lib.MKID_E_ARG
        assert _code(lambda: ch.pulse_fit_counted(d_phase, 300, 0, None, d_count, 10, *outs)) == _lib.MKID_E_ARG
        ch.pulse_fit_counted(d_phase, 300, 0, d_ev, d_count, 10, *outs)
        # a context that has the filter but not the fit
        ch2 = Channelizer(C, max_chunk=2 ** 14)
        try:
            ch2.set_pulse_filter(coeff, PRE)
            assert _code(lambda: ch2.pulse_fit_device(d_phase, 300, 0, d_ev, len(ev), *outs)) == _lib.MKID_E_STATE
        finally:
            ch2.close()
        _host(outs)
    finally:
        ch.close()


def test_fit_nullable_outputs(ctx):
    phase, coeff, ev, ts = _stream(seed=10, n=400)
    d_phase, d_ev = _dev(phase), _dev(ev)
    ctx.set_pulse_filter(coeff, PRE)
    ctx.set_pulse_fit(LS, SS)
    whole = _one_call(ctx, d_phase, 1200, 0, ev)
    for drop in (1, 2, 3):
        outs = _outputs(len(ev), fill=-7)
        args = [None if i == drop else o for i, o in enumerate(outs)]
        ctx.set_pulse_fit(LS, SS)
        ctx.pulse_fit_device(d_phase, 1200, 0, d_ev, len(ev), *args)
        got = _host(outs)
        for i in range(4):
            if i == drop:
                assert np.all(got[i] == -7)
            else:
                assert np.array_equal(got[i].view(np.int32), whole[i].view(np.int32))
