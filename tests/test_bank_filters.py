"""mkid_bank_filters (k_template.hip, mkid_calib.hip): every channel's template and pulse filter
from a record bank in one device call.

mkid_make_template runs the same kernels on one channel whose records are all ready, so in IQ mode
a channel at any slot of a grouped bank must equal mkid_make_template + mkid_optimal_filter on the
same records run alone (R = P) bit for bit; that pins the indexing by (channel, pulse), the stop at
ready_c and the grouping, not the arithmetic. The independent reference for the arithmetic is the
oracle: its check of tests/test_gpu_template.py runs on the single call there and on every used
channel here. Phase mode forms I = cosf(sign phi), Q = sinf(sign phi) on the device, where the
loop path takes numpy's float32 cos / sin: the CPU test below shows that moving I, Q and the arctan2 by
+-2 ulp leaves every decision of the oracle on these sets alone and stays inside the bars that the
GPU test then uses, which is what makes exact counts and those bars a fair demand.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import template_pulses as tp
from oracle import template_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'mkidgpu.h')

F32_SENTINEL = 0x7FC12345          # NaN patterns: any write shows
F64_SENTINEL = 0x7FF80000DEADBEEF


# ---- CPU: the ABI ----------------------------------------------------------------------------------

def _header_struct(name):
    src = open(HEADER).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), src, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(',')]
    return fields


def test_bank_filters_abi_is_declared():
    """The entry point and its two structs in the header, in _lib.EXPORTS and _lib._SIGS, with
    ctypes mirrors of the same fields, order and size."""
    from mkids_sdr_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+mkid_bank_filters\s*\(', src)
    assert 'mkid_bank_filters' in _lib.EXPORTS and len(_lib._SIGS['mkid_bank_filters']) == 9
    ctypes_of = {'int32_t': ctypes.c_int32, 'float': ctypes.c_float, 'double': ctypes.c_double}
    for cname, mirror, size in (('mkid_bank_cfg', _lib.BankCfg, 36), ('mkid_bank_result', _lib.BankResult, 48)):
        want = [(n, ctypes_of[t]) for n, t in _header_struct(cname)]
        assert [(n, t) for n, t in mirror._fields_] == want
        assert ctypes.sizeof(mirror) == size
    assert [n for n, _ in _lib.BankCfg._fields_] == ['n_channels', 'max_per_ch', 'length', 'min_records', 'pre',
                                                     'ncoeff', 'ready_stride', 'group', 'sign']
    assert [n for n, _ in _lib.BankResult._fields_] == ['count', 'count1', 'pm', 'pdev', 'flag', 'pstart', 'status',
                                                        'ready']
    from mkids_sdr_amd import template
    assert template.RESULT_DTYPE.itemsize == 48 and list(template.RESULT_DTYPE.names) == [
        n for n, _ in _lib.BankResult._fields_]
    assert callable(template.bank_filters) and callable(template.filters_from_bank_device)


# ---- the phase-mode sets, their oracle results and their bars ------------------------------------

PHASE_SETS = ('+3.1', '-3.1', 'rest0.5')


@functools.lru_cache(maxsize=None)
def phase_set(name):
    """(phase records, oracle result on template.iq_from_phase(records))."""
    from mkids_sdr_amd import template
    if name == 'rest0.5':
        rec, ready = tp.filter_bank_records()
        rec = rec[1, :ready[1]].copy()
        ref = template_ref.make_template(*template.iq_from_phase(rec))
    else:
        where = float(name)
        rec = tp.phase_records(64, 5, where)
        ref = tp.case('phase', 64, where)[2]
    rec.setflags(write=False)
    return rec, ref


@functools.lru_cache(maxsize=None)
def iq_jitter_runs(name):
    """The oracle with I and Q moved by -2..+2 float32 ulp per sample and its arctan2 moved likewise
    (tp.ulp_jitter), three draws: what a device cosf / sinf / atan2f within 2 ulp may do."""
    from mkids_sdr_amd import template
    rec, _ = phase_set(name)
    I, Q = template.iq_from_phase(rec)
    runs = []
    for d in range(tp.JITTER_DRAWS):
        jI, jQ = tp.ulp_jitter(tp.JITTER_ULP, 2000 + d)(I), tp.ulp_jitter(tp.JITTER_ULP, 3000 + d)(Q)
        runs.append(template_ref.make_template(jI, jQ, phase_hook=tp.ulp_jitter(tp.JITTER_ULP, 1000 + d)))
    return tuple(runs)


def iq_jitter_deviation(name):
    ref = phase_set(name)[1]
    devs = [tp.deviations(ref, r) for r in iq_jitter_runs(name)]
    return {k: max(d[k] for d in devs) for k in tp.BARS}


def phase_bars(name):
    """tp.bars('phase', 64, +-3.1) for the sets at rest near +-pi; for the set at rest at 0.5 the
    larger of the project's bars and 4 x the jittered oracle's deviation."""
    if name == 'rest0.5':
        dev = iq_jitter_deviation(name)
        return {k: max(tp.BARS[k], 4.0 * dev[k]) for k in tp.BARS}
    return tp.bars('phase', 64, float(name))


@pytest.mark.parametrize('name', PHASE_SETS)
def test_phase_mode_bars_are_fair(name):
    """I, Q and arctan2 moved by +-2 ulp: the oracle keeps count1, count, flag and pstart and stays
    inside the bar of the GPU test; at rest 0.5 all four deviations are under tp.BARS."""
    ref = phase_set(name)[1]
    for r in iq_jitter_runs(name):
        assert (r['count1'], r['count'], r['flag'], r['pstart']) == (ref['count1'], ref['count'], ref['flag'],
                                                                     ref['pstart'])
    dev, bars = iq_jitter_deviation(name), phase_bars(name)
    print(name, ' '.join('%s %.2e (bar %.2e)' % (k, dev[k], bars[k]) for k in tp.BARS))
    assert ref['count'] > 0
    for k in tp.BARS:
        assert dev[k] <= bars[k]
        if name == 'rest0.5':
            assert dev[k] < tp.BARS[k]


# ---- GPU -------------------------------------------------------------------------------------------

on_gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def ch(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    c = Channelizer(64, max_chunk=1 << 14)
    yield c
    c.close()


def _flat_rows(P=24, seed=9):
    """The flat part of tp.one_good_among_flat: noisy rows without a pulse."""
    rng = np.random.default_rng(seed + 1)
    return ((2.0 - rng.normal(size=(P, 2000)) * .01).astype(np.float32),
            (rng.normal(size=(P, 2000)) * .01).astype(np.float32))


@functools.lru_cache(maxsize=None)
def iq_sets():
    """The channels of the IQ bank: (I, Q, ready, wanted status, tp.case key or None)."""
    sets = [tp.case('cat', P, 0)[:2] + (P, 0, ('cat', P, 0)) for P in (24, 99, 100, 101, 257)]
    sets.append(tp.case('cat', 24, 180)[:2] + (24, 0, ('cat', 24, 180)))
    sets.append(tp.case('cat', 257, 168)[:2] + (257, 0, ('cat', 257, 168)))
    sets.append(tp.one_good_among_flat(24) + (24, 3, None))
    sets.append(_flat_rows(24) + (24, 2, None))
    I24, Q24 = tp.case('cat', 24, 0)[:2]
    sets.append((I24, Q24, 5, 1, None))     # 24 rows held, 5 of them ready
    sets.append((I24[:0], Q24[:0], 0, 1, None))
    return tuple(sets)


def _bank(sets, R, order=None, Cb=None, at=0, filler=None):
    """Device I, Q [Cb][R][2000] with NaN at and beyond each channel's ready rows, info [Cb][2] int32
    {ready, a large `dropped`}: sets[order[k]] at channel at + k, `filler` sets in the others."""
    import torch
    order = list(range(len(sets))) if order is None else order
    Cb = Cb or len(order)
    I = torch.full((Cb, R, 2000), float('nan'), dtype=torch.float32, device='cuda')
    Q = torch.full((Cb, R, 2000), float('nan'), dtype=torch.float32, device='cuda')
    info = np.zeros((Cb, 2), np.int32)
    info[:, 1] = 0x7FFFFFF0 - np.arange(Cb)
    chan = {at + k: sets[i] for k, i in enumerate(order)}
    for c in range(Cb):
        sI, sQ, ready = (chan[c] if c in chan else filler[c % len(filler)])[:3]
        I[c, :ready] = torch.from_numpy(np.array(sI[:ready])).cuda()
        Q[c, :ready] = torch.from_numpy(np.array(sQ[:ready])).cuda()
        info[c, 0] = ready
    return I, Q, torch.from_numpy(info).cuda()


def _run(ch, I, Q, info, **kw):
    """template.bank_filters with templates kept, everything copied to the host."""
    from mkids_sdr_amd import template
    r = template.bank_filters(ch, I, Q, info, min_records=20, keep_templates=True, **kw)
    return dict(coeff=r['coeff'].cpu().numpy(), templates=r['templates'].cpu().numpy(),
                noise=r['noise'].cpu().numpy(), table=template.result_table(r['result']))


def _same_bits(a, b, rows_a=None, rows_b=None):
    for k in ('coeff', 'templates', 'noise'):
        x = a[k] if rows_a is None else a[k][rows_a]
        y = b[k] if rows_b is None else b[k][rows_b]
        assert np.array_equal(x.view('u%d' % x.dtype.itemsize), y.view('u%d' % y.dtype.itemsize)), k
    ta = a['table'] if rows_a is None else a['table'][rows_a]
    tb = b['table'] if rows_b is None else b['table'][rows_b]
    assert ta.tobytes() == tb.tobytes()


@pytest.fixture(scope='module')
def iq_bank(ch):
    I, Q, info = _bank(iq_sets(), 257)
    return I, Q, info, _run(ch, I, Q, info)


@pytest.fixture(scope='module')
def single(ch):
    """mkid_make_template + mkid_optimal_filter on each used set of the IQ bank, run alone (R = P)."""
    from mkids_sdr_amd import template
    out = {}
    for c, (I, Q, ready, status, _) in enumerate(iq_sets()):
        if status == 0:
            r = template.make_template(ch, I.copy(), Q.copy())
            r['coeff'] = template.optimal_filter(ch, r['d_template'], r['d_noise'], pre=100, ncoeff=100)
            out[c] = r
    return out


def _equals_single(got, c, want):
    t = got['table'][c]
    assert np.array_equal(got['templates'][c], want['template']) and np.array_equal(got['noise'][c], want['noise'])
    for k in ('count', 'count1', 'pm', 'pdev', 'flag', 'pstart'):
        assert t[k] == want[k], k
    assert np.array_equal(got['coeff'][c], want['coeff'].astype(np.float32))


@on_gpu
def test_iq_mode_equals_single_path_bit_for_bit(iq_bank, single):
    """Every used channel of an 11-channel bank (R = 257), at slots b = 0..6 of its group with 24 to
    257 of the 257 records ready, equals the same records run alone (mkid_make_template at R = P, then
    mkid_optimal_filter) bit for bit and passes the oracle check of tests/test_gpu_template.py; the
    channels with one pulse among flat rows, flat rows only, 5 records and none say status 3, 2, 1, 1."""
    from test_gpu_template import _check
    got = iq_bank[3]
    sets = iq_sets()
    assert got['table']['status'].tolist() == [s[3] for s in sets]
    assert got['table']['ready'].tolist() == [s[2] for s in sets]
    for c, (_, _, _, status, key) in enumerate(sets):
        t = got['table'][c]
        if status:
            assert (t['flag'], t['pstart'], t['count']) == (-1, -1, 0)
            continue
        _equals_single(got, c, single[c])
        ref = tp.case(*key)[2]
        _check(dict(template=got['templates'][c], noise=got['noise'][c], **{k: t[k] for k in t.dtype.names}), ref,
               tp.bars(*key))


@on_gpu
def test_iq_mode_first_pass_cap(ch):
    """1003 pulses per channel in a two-channel bank of R = 1003: pass 1 stops at 1000 pulses, pass 2
    re-references those 1000 a second time and the last three once. The channel at slot 1 and the one
    at slot 0 equal the same records run alone at R = P = 1003 bit for bit, and both pass the oracle
    check."""
    from mkids_sdr_amd import template
    from test_gpu_template import _check
    sets = [tp.case('cat', 1003, 0)[:2] + (1003,), tp.case('cat', 1003, 168)[:2] + (1003,)]
    I, Q, info = _bank(sets, 1003)
    got = _run(ch, I, Q, info)
    assert got['table']['status'].tolist() == [0, 0]
    for c, theta in enumerate((0, 168)):
        want = template.make_template(ch, sets[c][0].copy(), sets[c][1].copy())
        want['coeff'] = template.optimal_filter(ch, want['d_template'], want['d_noise'], pre=100, ncoeff=100)
        _equals_single(got, c, want)
        t = got['table'][c]
        _check(dict(template=got['templates'][c], noise=got['noise'][c], **{k: t[k] for k in t.dtype.names}),
               tp.case('cat', 1003, theta)[2], tp.bars('cat', 1003, theta))


def _raw_call(ch, I, Q, ready, cfg, tpl, noise, coeff, result):
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    import torch
    torch.cuda.synchronize()
    rc = ch._L.mkid_bank_filters(ch._h, p(I), p(Q), p(ready), ctypes.byref(cfg) if cfg is not None else None,
                                 p(tpl), p(noise), p(coeff), p(result))
    torch.cuda.synchronize()
    return rc


def _sentinel_outputs(Cb, ncoeff=100):
    import torch
    coeff = torch.full((Cb, ncoeff), F32_SENTINEL, dtype=torch.int32, device='cuda')
    tpl = torch.full((Cb, 2000), F64_SENTINEL, dtype=torch.int64, device='cuda')
    noise = torch.full((Cb, 800), F64_SENTINEL, dtype=torch.int64, device='cuda')
    result = torch.full((Cb, 12), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    return tpl, noise, coeff, result


@on_gpu
def test_unused_rows_untouched_and_inputs_unread(ch, iq_bank):
    """Outputs pre-filled with a NaN pattern: rows of channels with status != 0 keep its bits, used
    rows are finite and those of the plain run. The bank holds NaN at and beyond every channel's
    ready rows and its info a large `dropped` column (ready_stride = 2): neither is read, and the
    bank's bits are the same after the call."""
    import torch
    from mkids_sdr_amd import _lib, template
    I, Q, info, plain = iq_bank
    before = (I.view(dtype=torch.int32).clone(), Q.view(dtype=torch.int32).clone(), info.clone())
    Cb = I.shape[0]
    tpl, noise, coeff, result = _sentinel_outputs(Cb)
    cfg = _lib.BankCfg(Cb, 257, 2000, 20, 100, 100, 2, 0, -1.0)
    assert _raw_call(ch, I, Q, info, cfg, tpl, noise, coeff, result) == _lib.MKID_OK
    assert torch.equal(I.view(dtype=torch.int32), before[0]) and torch.equal(Q.view(dtype=torch.int32), before[1])
    assert torch.equal(info, before[2])
    table = template.result_table(result.view(dtype=torch.uint8))
    assert table.tobytes() == plain['table'].tobytes()
    coeff, tpl, noise = coeff.cpu().numpy(), tpl.cpu().numpy(), noise.cpu().numpy()
    for c in range(Cb):
        if table['status'][c]:
            assert (coeff[c] == F32_SENTINEL).all() and (tpl[c] == F64_SENTINEL).all() and (
                noise[c] == F64_SENTINEL).all()
        else:
            for got, want in ((coeff[c].view(np.float32), plain['coeff'][c]),
                              (tpl[c].view(np.float64), plain['templates'][c]),
                              (noise[c].view(np.float64), plain['noise'][c])):
                assert np.isfinite(got).all() and np.array_equal(got, want)


@on_gpu
def test_channels_do_not_depend_on_their_neighbours(ch, iq_bank):
    """The IQ bank again with group = 1, 2, 4, 0 (11 channels: a multiple of neither 2 nor 4), with
    its channels reversed, at channels 70.. of a 130-channel bank (three groups at the default budget)
    among other sets, and twice: the same bits for every channel."""
    I, Q, info, plain = iq_bank
    sets = iq_sets()
    n = len(sets)
    for group in (1, 2, 4, 0):
        _same_bits(_run(ch, I, Q, info, group=group), plain)
    _same_bits(_run(ch, I, Q, info), plain)
    order = list(range(n))[::-1]
    rI, rQ, rinfo = _bank(sets, 257, order=order)
    _same_bits(_run(ch, rI, rQ, rinfo), plain, rows_b=order)
    del rI, rQ
    filler = (tp.case('cat', 24, 180)[:2] + (24,), tp.case('cat', 24, 0)[:2] + (21,), sets[7][:3])
    bI, bQ, binfo = _bank(sets, 257, Cb=130, at=70, filler=filler)
    big = _run(ch, bI, bQ, binfo)
    _same_bits(big, plain, rows_a=slice(70, 70 + n))
    assert big['table']['status'][:70].tolist() == [(0, 0, 3)[c % 3] for c in range(70)]


@on_gpu
def test_phase_mode_against_the_oracle(ch):
    """Phase records (sign = -1) at rest at +3.1, -3.1 (64 records each) and the three channels of
    tp.filter_bank_records() in one bank of R = 64: the oracle's decisions on
    template.iq_from_phase(records) exactly, template, noise, pm and pdev within phase_bars, the
    filter equal to the oracle's filter of the device template and noise to a float32 rounding."""
    import torch
    from mkids_sdr_amd import template
    from test_gpu_template import _check
    rec3, ready3 = tp.filter_bank_records()
    bank = np.full((5, 64, 2000), np.nan, np.float32)
    bank[0], bank[1] = phase_set('+3.1')[0], phase_set('-3.1')[0]
    ready = np.array([64, 64] + ready3.tolist(), np.int32)
    for c in range(3):
        bank[2 + c, :ready3[c]] = rec3[c, :ready3[c]]
    r = template.bank_filters(ch, torch.from_numpy(bank).cuda(), None, torch.from_numpy(ready).cuda(),
                              min_records=20, keep_templates=True, sign=-1.0)
    table = template.result_table(r['result'])
    assert table['status'].tolist() == [0, 0, 3, 0, 1] and table['ready'].tolist() == ready.tolist()
    tpl, noise, coeff = r['templates'].cpu().numpy(), r['noise'].cpu().numpy(), r['coeff'].cpu().numpy()
    for c, name in ((0, '+3.1'), (1, '-3.1'), (3, 'rest0.5')):
        t = table[c]
        _check(dict(template=tpl[c], noise=noise[c], **{k: t[k] for k in t.dtype.names}), phase_set(name)[1],
               phase_bars(name))
        want = template_ref.optimal_filter(tpl[c], noise[c], ncoeff=100, pre=100).astype(np.float32)
        np.testing.assert_allclose(coeff[c], want, rtol=2.0 ** -23, atol=1e-12 * np.abs(want).max())
    assert not coeff[2].any() and not coeff[4].any()


@on_gpu
def test_filters_from_bank_device_agrees_with_the_loop(ch):
    """The hand-built bank of test_device_filters_from_bank_takes_the_fallback through both paths:
    used, flag, pstart, count and ready equal, fallback rows equal bit for bit, the used row within
    the bars of the phase-mode test."""
    import torch
    from mkids_sdr_amd import template
    from test_gpu_template import _check
    rec, ready = tp.filter_bank_records()
    bank = (torch.from_numpy(rec).cuda(), torch.zeros(rec.shape[:2], dtype=torch.int64, device='cuda'),
            torch.from_numpy(np.stack((ready, np.zeros_like(ready)), axis=1)).cuda())
    fallback = np.arange(100, dtype=np.float32)
    loop = template.filters_from_bank(ch, bank, ncoeff=100, pre=100, min_records=20, fallback=fallback)
    dev = template.filters_from_bank_device(ch, bank, ncoeff=100, pre=100, min_records=20, fallback=fallback,
                                            keep_templates=True)
    for k in ('used', 'flag', 'pstart', 'count', 'ready'):
        assert np.array_equal(dev[k], loop[k]), k
    assert dev['used'].tolist() == [False, True, False] and dev['status'].tolist() == [3, 0, 1]
    assert dev['coeff'].dtype == np.float32
    for c in (0, 2):
        assert np.array_equal(dev['coeff'][c].view(np.uint32), loop['coeff'][c].view(np.uint32))
        assert np.array_equal(dev['coeff'][c], fallback)
    assert sorted(dev['templates']) == [1]
    t, J = dev['templates'][1]
    ref = phase_set('rest0.5')[1]
    got = dict(template=t, noise=J, count=dev['count'][1], count1=ref['count1'], flag=dev['flag'][1],
               pstart=dev['pstart'][1], pm=ref['pm'], pdev=ref['pdev'])
    _check(got, ref, phase_bars('rest0.5'))
    want = template_ref.optimal_filter(t, J, ncoeff=100, pre=100).astype(np.float32)
    np.testing.assert_allclose(dev['coeff'][1], want, rtol=2.0 ** -23, atol=1e-12 * np.abs(want).max())


@on_gpu
def test_bad_requests_are_refused_before_any_launch(ch):
    """Every MKID_E_ARG case of the header: refused, and the outputs keep their bits."""
    import torch
    from mkids_sdr_amd import _lib
    I = torch.zeros((2, 3, 2000), dtype=torch.float32, device='cuda')
    ready = torch.tensor([3, 3], dtype=torch.int32, device='cuda')
    outs = _sentinel_outputs(2)
    keep = [o.clone() for o in outs]
    tpl, noise, coeff, result = outs

    def cfg(**kw):
        f = dict(n_channels=2, max_per_ch=3, length=2000, min_records=1, pre=100, ncoeff=100, ready_stride=1,
                 group=0, sign=-1.0)
        f.update(kw)
        return _lib.BankCfg(*(f[n] for n, _ in _lib.BankCfg._fields_))

    bad = [dict(length=1999), dict(length=4096), dict(n_channels=0), dict(max_per_ch=0), dict(pre=9),
           dict(pre=2001), dict(ncoeff=0), dict(ncoeff=801), dict(ready_stride=0), dict(group=-1)]
    for kw in bad:
        for Q in (I, None):
            assert _raw_call(ch, I, Q, ready, cfg(**kw), tpl, noise, coeff, result) == _lib.MKID_E_ARG, kw
    for sign in (0.0, float('nan'), float('inf')):
        assert _raw_call(ch, I, None, ready, cfg(sign=sign), tpl, noise, coeff, result) == _lib.MKID_E_ARG, sign
    good = cfg()
    for args in ((None, I, ready, good, tpl, noise, coeff, result), (I, I, None, good, tpl, noise, coeff, result),
                 (I, I, ready, None, tpl, noise, coeff, result), (I, I, ready, good, tpl, noise, None, result),
                 (I, I, ready, good, tpl, noise, coeff, None)):
        assert _raw_call(ch, *args) == _lib.MKID_E_ARG
    for o, k in zip(outs, keep):
        assert torch.equal(o, k)


# ---- mkid_make_template: the same launch on one channel --------------------------------------------

FIRST = b'make_template: no pulse passed the first pass'
SECOND = b'make_template: no pulse passed the second pass'


@on_gpu
@pytest.mark.parametrize('rows,P,message', [('flat', 24, FIRST), ('one_good', 24, SECOND), ('flat', 1, FIRST),
                                            ('one_good', 1, SECOND)])
def test_make_template_failure_leaves_outputs_alone(ch, rows, P, message):
    """Flat rows only (no pulse passes pass 1) and one good pulse among flat rows or alone (none
    passes pass 2), through the raw entry point with the template and noise pre-filled with the NaN
    pattern and info with a byte pattern: MKID_E_STATE with the pass's message, and every output
    byte as it was."""
    import torch
    from mkids_sdr_amd import _lib
    I, Q = _flat_rows(P) if rows == 'flat' else tp.one_good_among_flat(P)
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    tpl = torch.full((2000,), F64_SENTINEL, dtype=torch.int64, device='cuda')
    noise = torch.full((800,), F64_SENTINEL, dtype=torch.int64, device='cuda')
    info = _lib.TemplateInfo()
    ctypes.memset(ctypes.byref(info), 0x5A, ctypes.sizeof(info))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = ch._L.mkid_make_template(ch._h, p(dI), p(dQ), P, p(tpl), p(noise), ctypes.byref(info))
    torch.cuda.synchronize()
    assert rc == _lib.MKID_E_STATE and ch._L.mkid_last_error(ch._h) == message
    assert (tpl.cpu().numpy() == F64_SENTINEL).all() and (noise.cpu().numpy() == F64_SENTINEL).all()
    assert bytes(info) == b'\x5a' * ctypes.sizeof(info)


def _template_bits(r):
    return (r['template'].tobytes() + r['noise'].tobytes()
            + np.array([r[k] for k in ('count', 'count1', 'pm', 'pdev')], np.float64).tobytes()
            + np.array([r['flag'], r['pstart']], np.int32).tobytes())


@on_gpu
def test_make_template_and_bank_filters_share_one_workspace(gpu, iq_bank):
    """On a context of its own, so that the first call finds no workspace: make_template at P = 24
    (allocates), bank_filters on the 11-channel IQ bank (grows it), make_template at P = 257 and at
    24 again (the bank's larger workspace, reused), bank_filters again. The two P = 24 results are
    the same bits, and so are the two bank results, which are also those of the module's context."""
    from mkids_sdr_amd import template
    from mkids_sdr_amd.channelizer import Channelizer
    I, Q, info, plain = iq_bank
    c = Channelizer(64, max_chunk=1 << 14)
    try:
        one = lambda P: template.make_template(c, *(a.copy() for a in tp.case('cat', P, 0)[:2]))
        first24 = one(24)
        bank1 = _run(c, I, Q, info)
        big = one(257)
        again24 = one(24)
        bank2 = _run(c, I, Q, info)
    finally:
        c.close()
    assert _template_bits(first24) == _template_bits(again24) != _template_bits(big)
    _same_bits(bank1, bank2)
    _same_bits(bank1, plain)
