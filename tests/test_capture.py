"""Pulse capture (include/mkidgpu.h mkid_set_capture / mkid_capture_pulses, k_capture.hip) against
tests/capture_ref.py, the numpy statement of the contract.

CPU: the reference against a plain double loop (with 28-bit stamp unwrapping), its own chunk
invariance, the ABI declarations, and that the inputs of the GPU tests reach every category they
are meant to (recorded, skipped at the stream start, still pending, dropped, served from the
carried rows, windows over three calls). GPU: the device bank against the reference, exactly (the
capture is a copy): one call, chunked streams, dense packets, unwrapping, segment breaks, errors,
the chain on the device's own phase and packets, and bank -> template -> filter.
"""
import os
import re

import numpy as np
import pytest

import capture_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = 32   # Channelizer's default dead_time: sizes the device's pending list


def _events(pairs, j0):
    """(channel, global stamp) pairs -> packets, channel-major and time-ascending."""
    return np.array([cr.pack(c, jg) for c, jg in sorted(pairs)], np.uint64).reshape(-1)


def _deliver(pairs, cuts, j0=0, late=()):
    """Split a stream's packets over the calls that produce them: a packet goes with the call
    whose rows hold its stamp, the ones in `late` (stamped at a call's last row) with the next."""
    starts = j0 + np.concatenate([[0], np.cumsum(cuts)])
    per = [[] for _ in cuts]
    for c, jg in pairs:
        k = int(np.searchsorted(starts, jg, side='right')) - 1
        if (c, jg) in late:
            assert jg == starts[k + 1] - 1
            k += 1
        per[min(max(k, 0), len(cuts) - 1)].append((c, jg))
    return [_events(p, j0) for p in per], starts


def _calls(phase, pairs, cuts, j0=0, late=()):
    evs, starts = _deliver(pairs, cuts, j0, late)
    return [(phase[starts[k] - j0:starts[k + 1] - j0], int(starts[k]), evs[k]) for k in range(len(cuts))]


def _same(ref, got):
    records, stamps, info = got
    assert np.array_equal(info, ref.info)
    assert np.array_equal(stamps, ref.stamps)
    assert np.array_equal(records.view(np.uint32), ref.records.view(np.uint32))


# ---- the inputs of the GPU tests (built once, shared, never modified) ---------------------------

def _one_call(C=64, j0=0):
    """rows 300, L 20, pre 6, R 4: stamps 0 and 5 lie before the stream, 6 is the first eligible
    one, 286 the last that completes, 290 / 299 stay pending; channel 3 has 7 > R packets."""
    rows, L, pre, R = 300, 20, 6, 4
    rng = np.random.default_rng(70)
    phase = rng.normal(size=(rows, C)).astype(np.float32)
    pairs = []
    for c in range(0, C, 3):
        pairs += [(c, j0 + t) for t in (0, 5, 6, 50 + c, 150, 270, 286, 290, 299)]
    pairs = [p for p in pairs if p[0] != 3] + [(3, j0 + t) for t in (0, 50, 80, 110, 140, 170, 200, 230, 299)]
    pairs += [(C, j0 + 100), (4095, j0 + 120)]          # channel field >= C
    return dict(C=C, L=L, pre=pre, R=R, phase=phase, pairs=pairs, j0=j0)


CUTS = [64, 1, 700, 2000, 37, 2198]


def _chunked(C):
    """5000 rows, L 2000, pre 1000, cut as CUTS: call 4 covers rows [765, 2765), call 5 [2765, 2802).
    Stamps <= 999 are skipped, 1000..1765 complete in call 4, ..1802 in call 5, ..4000 in call 6 (a
    stamp in (1802, 2765) waits over three calls), later ones stay pending. 2764 and 2801 are the
    last rows of calls 4 and 5 and are delivered with the next call (2801: from the carried rows)."""
    L, pre, R = 2000, 1000, 8
    rng = np.random.default_rng(71 + C)
    phase = rng.normal(size=(5000, C)).astype(np.float32)
    pairs, late = [], set()
    for c in range(C):
        for t in (300, 999, 1000, 1400, 1765, 1766, 1802, 1803, 2300, 2764, 2801, 3300, 4000, 4001, 4700):
            if rng.random() < 0.5 or (c == 5):
                pairs.append((c, t + (int(rng.integers(0, 9)) if t in (300, 1400, 2300, 3300, 4700) else 0)))
                if t in (2764, 2801):
                    late.add(pairs[-1])
    return dict(C=C, L=L, pre=pre, R=R, phase=phase, pairs=pairs, late=late)


def _dense(C=64):
    """A packet every 32 rows in every channel, L 100: each row feeds about three records."""
    L, pre, R, rows = 100, 30, 64, 777
    rng = np.random.default_rng(72)
    phase = rng.normal(size=(2 * rows, C)).astype(np.float32)
    pairs = [(c, t) for c in range(C) for t in range(c % 32, 2 * rows, 32)]
    return dict(C=C, L=L, pre=pre, R=R, phase=phase, pairs=pairs, cuts=[rows, rows])


def _unwrap(j0, C=64):
    """Two calls of 150 rows from j0; one packet stamped j0 - 1 (before the stream) and one at the
    first call's last row, delivered with the second call."""
    d = _one_call(C, j0)
    d['pairs'] = [p for p in d['pairs'] if p[1] - j0 not in (149,)] + [(7, j0 - 1), (8, j0 + 149), (9, j0 + 149)]
    d['late'] = {(8, j0 + 149), (9, j0 + 149)}
    d['cuts'] = [150, 150]
    return d


def _ref_run(d, cuts=None, j0=0):
    cuts = cuts or d.get('cuts') or [d['phase'].shape[0]]
    calls = _calls(d['phase'], d['pairs'], cuts, d.get('j0', j0), d.get('late', ()))
    return cr.capture(calls, d['C'], d['L'], d['pre'], d['R'], cr.pend_cap(d['L'], d['pre'], DEAD)), calls


# ---- CPU -----------------------------------------------------------------------------------------

def _loop(phase, events, j0, C, L, pre, R):
    rec = np.zeros((C, R, L), np.float32)
    st = np.zeros((C, R), np.int64)
    info = np.zeros((C, 2), np.int32)
    rows = phase.shape[0]
    for w in events.tolist():
        c, ts = w >> 52, w & cr.TS_MASK
        base = max(j0 - (1 << 27), 0)
        jg = base + ((ts - (base & cr.TS_MASK)) & cr.TS_MASK)
        r0 = jg - pre - j0
        if c >= C or r0 < 0 or r0 + L > rows:
            continue
        if info[c, 0] == R:
            info[c, 1] += 1
            continue
        for i in range(L):
            rec[c, info[c, 0], i] = phase[r0 + i, c]
        st[c, info[c, 0]] = jg
        info[c, 0] += 1
    return rec, st, info


@pytest.mark.parametrize('j0', [0, 1000, (1 << 28) - 7, 3 << 28])
def test_capture_ref_matches_loop(j0):
    d = _one_call(8, j0)
    ev = _events(d['pairs'], j0)
    ref = cr.capture([(d['phase'], j0, ev)], 8, d['L'], d['pre'], d['R'])
    _same(ref, _loop(d['phase'], ev, j0, 8, d['L'], d['pre'], d['R']))
    s = ref.stats
    assert s['recorded'] == 12 and s['skipped'] == 5 and s['dropped'] == 5 and s['other_channel'] == 2
    assert ref.n_pending == 5


@pytest.mark.parametrize('seed', range(4))
def test_capture_ref_chunk_invariance(seed):
    rng = np.random.default_rng(seed)
    d = _chunked(8)
    d['late'] = set()
    whole, _ = _ref_run(d, [5000])
    for _ in range(3):
        cuts = np.diff(np.concatenate([[0], np.sort(rng.choice(np.arange(1, 5000), 7, replace=False)), [5000]]))
        part, _ = _ref_run(d, [int(x) for x in cuts])
        _same(whole, (part.records, part.stamps, part.info))
        assert part.n_pending == whole.n_pending
    one, _ = _ref_run(d, [1] * 5000)
    _same(whole, (one.records, one.stamps, one.info))


def test_capture_abi_declared():
    from mkids_sdr_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mkidgpu.h')).read(), flags=re.S)
    for name in ('mkid_set_capture', 'mkid_capture_pulses', 'mkid_capture_pulses_counted'):
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert name in _lib.EXPORTS and name in _lib._SIGS
    assert re.search(r'#define MKID_K_CAPTURE 7\b', src) and re.search(r'#define MKID_K_COUNT 8\b', src)
    assert (_lib.K_HEIGHTS, _lib.K_CAPTURE, _lib.K_COUNT) == (6, 7, 8)
    assert _lib.load().mkid_kernel_name(7) == b'k_capture'


def test_capture_inputs_hit_every_category():
    """The reference's own account of what the GPU tests' inputs exercise."""
    ref, _ = _ref_run(_one_call())
    s = ref.stats
    assert min(s['recorded'], s['skipped'], s['dropped'], s['other_channel'], ref.n_pending) > 0
    assert ref.info[:, 0].max() == 4 and ref.info[3, 1] == 3
    for C in (64, 256):
        d = _chunked(C)
        ref, _ = _ref_run(d, CUTS)
        s = ref.stats
        assert min(s['recorded'], s['skipped'], s['dropped'], s['carried'], s['prev_row'], s['spanned'],
                   s['waited3'], ref.n_pending) > 0, s
        whole, _ = _ref_run(dict(d, late=set()), [5000])
        _same(whole, (ref.records, ref.stamps, ref.info))
    ref, _ = _ref_run(_dense())
    assert ref.stats['recorded'] > 64 * 40 and ref.stats['dropped'] == 0 and ref.stats['spanned'] > 64
    assert ref.stats['skipped'] >= 32 and ref.n_pending >= 64
    for j0 in ((1 << 28) - 7, (3 << 28) + 5):
        ref, _ = _ref_run(_unwrap(j0))
        s = ref.stats
        assert s['prev_row'] == 2 and s['carried'] >= 2 and s['skipped'] > 0 and s['recorded'] > 20, s
        assert ref.stamps.max() > (j0 | cr.TS_MASK) or j0 > (1 << 29)   # stamps cross a 2^28 boundary


def test_iq_from_phase():
    from mkids_sdr_amd import template
    ph = np.linspace(-1, 1, 11, dtype=np.float32).reshape(1, -1)
    I, Q = template.iq_from_phase(ph)
    assert I.dtype == np.float32 and Q.dtype == np.float32
    assert np.allclose(np.arctan2(Q, I), -ph, atol=1e-6)


# ---- GPU -----------------------------------------------------------------------------------------

def _device_run(ch, calls, bank=None):
    bank = bank if bank is not None else ch.capture_bank()
    for phase, j0, ev in calls:
        ch.capture_pulses(phase, ev, j0, bank)
    return bank


def _host(bank):
    return tuple(t.cpu().numpy() for t in bank)


def _channelizer(d):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(d['C'], max_chunk=2 ** 14 * (d['C'] // 64))
    ch.set_capture(d['L'], d['pre'], d['R'])
    return ch


@pytest.mark.gpu
def test_capture_one_call(gpu):
    d = _one_call()
    ref, calls = _ref_run(d)
    assert ref.stats['recorded'] > 0 and ref.stats['dropped'] > 0 and ref.n_pending > 0
    ch = _channelizer(d)
    try:
        _same(ref, _host(_device_run(ch, calls)))
    finally:
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize('C', [64, 256])
def test_capture_chunk_invariance(gpu, C):
    d = _chunked(C)
    ref, calls = _ref_run(d, CUTS)
    assert min(ref.stats['carried'], ref.stats['waited3'], ref.stats['dropped'], ref.n_pending) > 0
    ch = _channelizer(d)
    try:
        got = _host(_device_run(ch, calls))
        _, whole = _ref_run(dict(d, late=set()), [5000])
        one = _host(_device_run(ch, whole))      # j0 = 0 again: a new segment
    finally:
        ch.close()
    _same(ref, got)
    _same(ref, one)


@pytest.mark.gpu
def test_capture_dense(gpu):
    d = _dense()
    ref, calls = _ref_run(d)
    assert ref.stats['recorded'] > 64 * 40 and ref.stats['spanned'] > 64
    ch = _channelizer(d)
    try:
        _same(ref, _host(_device_run(ch, calls)))
    finally:
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize('j0', [(1 << 28) - 7, (3 << 28) + 5])
def test_capture_unwrap(gpu, j0):
    d = _unwrap(j0)
    ref, calls = _ref_run(d)
    assert ref.stats['prev_row'] == 2 and ref.stats['carried'] >= 2
    ch = _channelizer(d)
    try:
        _same(ref, _host(_device_run(ch, calls)))
    finally:
        ch.close()


@pytest.mark.gpu
@pytest.mark.parametrize('count', [-1, 0])
def test_capture_counted_none(gpu, count):
    """A device-side count of 0, or below it, reads no packet: bank, stamps and info are those of
    the call with n = 0 on the same rows."""
    import torch
    d = _one_call()
    (phase, j0, ev), = _ref_run(d)[1]
    ch = _channelizer(d)
    try:
        d_ph = torch.from_numpy(phase).cuda()
        d_ev = torch.from_numpy(ev.view(np.int64)).cuda()
        d_count = torch.tensor([count], dtype=torch.int64, device='cuda')
        none, got = ch.capture_bank(), ch.capture_bank()
        torch.cuda.synchronize()
        ch.capture_pulses_device(d_ph, phase.shape[0], j0, d_ev, 0, *none)
        ch.capture_pulses_counted(d_ph, phase.shape[0], j0, d_ev, d_count, len(ev), *got)   # j0 again: a new segment
        torch.cuda.synchronize()
        none, got = _host(none), _host(got)
    finally:
        ch.close()
    assert len(ev) > 100 and not none[2].any()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(none, got))


@pytest.mark.gpu
def test_capture_segment_break_and_reset(gpu):
    """A call whose j0 skips ahead, and reset_stream, forget the carried rows and the pending
    packets and keep the bank; info handed in by the caller continues a bank."""
    C, L, pre, R = 64, 20, 6, 5
    rng = np.random.default_rng(73)
    ph = [rng.normal(size=(300, C)).astype(np.float32) for _ in range(4)]
    ev = [_events([(c, j0 + t) for c in range(0, C, 5) for t in ts], j0)
          for j0, ts in ((0, (100, 295)), (1000, (3, 120, 296)), (1300, (5, 130)), (1600, (-1, 3, 140)))]
    ref = cr.CaptureRef(C, L, pre, R, cr.pend_cap(L, pre, DEAD))
    ref.call(ph[0], 0, ev[0])
    assert ref.n_pending > 0                 # lost at the break
    ref.call(ph[1], 1000, ev[1])
    lost = ref.n_pending
    ref.reset()
    ref.call(ph[2], 1300, ev[2])             # contiguous in j0, but after a reset: stamp 1305 is skipped
    assert lost > 0 and ref.stats['skipped'] == 2 * 13
    ref.call(ph[3], 1600, ev[3])             # continues: stamps 1599 and 1603 come from the carried rows
    assert ref.stats['carried'] >= 2 * 13 and ref.stats['dropped'] > 0
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(C, max_chunk=2 ** 14)
    try:
        ch.set_capture(L, pre, R)
        bank = ch.capture_bank()
        ch.capture_pulses(ph[0], ev[0], 0, bank)
        ch.capture_pulses(ph[1], ev[1], 1000, bank)
        ch.reset()
        ch.capture_pulses(ph[2], ev[2], 1300, bank)
        mid = _host(bank)
        assert mid[2][:, 0].max() > 0
        bank2 = tuple(t.clone() for t in bank)   # the caller's copy of the bank carries on
        ch.capture_pulses(ph[3], ev[3], 1600, bank2)
        _same(ref, _host(bank2))
        assert all(np.array_equal(a, b) for a, b in zip(mid, _host(bank)))
    finally:
        ch.close()


@pytest.mark.gpu
def test_capture_errors(gpu):
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    import torch
    ch = Channelizer(64, max_chunk=2 ** 14)
    try:
        z = torch.zeros(64 * 4 * 8, dtype=torch.float32, device='cuda')
        with pytest.raises(_lib.MkidError) as e:    # not configured yet
            ch.capture_pulses_device(z, 4, 0, z, 1, z, z, z)
        assert e.value.code == _lib.MKID_E_STATE
        for bad in ((0, 0, 4), (4097, 0, 4), (20, -1, 4), (20, 20, 4), (20, 6, 0)):
            with pytest.raises(_lib.MkidError) as e:
                ch.set_capture(*bad)
            assert e.value.code == _lib.MKID_E_ARG
        ch.set_capture(4096, 4095, 1)
        ch.set_capture(8, 2, 4)
        with pytest.raises(_lib.MkidError):
            ch.capture_pulses_device(z, -1, 0, z, 1, z, z, z)
        with pytest.raises(_lib.MkidError):
            ch.capture_pulses_device(z, 4, 0, z, 1, None, z, z)
        bank = ch.capture_bank()
        ch.capture_pulses_device(None, 0, 0, None, 0, *bank)     # rows == 0 and n == 0 are valid
        assert ch._L.mkid_kernel_name(7) == b'k_capture'
        ch.set_timing(True, kernels=['k_capture'])
        ch.capture_pulses(np.zeros((4, 64), np.float32), np.zeros(0, np.uint64), 0, bank)
        assert ch.timing()['k_capture'][1] == 1
    finally:
        ch.close()


@pytest.mark.gpu
def test_capture_chain(gpu):
    """Two process_device calls, each followed by the counted capture on its own device phase,
    packets and count: the bank equals the reference on the downloaded phase and packets."""
    import torch
    import signals
    from mkids_sdr_amd.channelizer import Channelizer
    C, S, L, pre, R = 64, 2 ** 15, 120, 30, 8
    J = S // (2 * C)
    case = signals.make_case(C, 2 * S, seed=7, pulses_per_ch=6.0)
    quiet = signals.make_case(C, S, seed=7, pulses_per_ch=0)
    thr = signals.thresholds_from_quiet(quiet, signals.oracle_chain(quiet).process(quiet.iq)['raw'])
    ch = Channelizer(C, max_chunk=S)
    calls = []
    try:
        ch.set_pfb(case.pfb)
        ch.set_bins(case.bins)
        ch.set_dds(case.lut_i, case.lut_q)
        ch.set_lpf(case.lpf12)
        ch.set_fir(case.fir12)
        ch.set_centers(case.ic, case.qc)
        ch.set_thresholds(thr)
        ch.set_capture(L, pre, R)
        bank = ch.capture_bank()
        x = torch.from_numpy(case.iq.reshape(-1)).to('cuda')
        cap = J * C
        for k in range(2):
            d_ph = torch.empty((J, C), dtype=torch.float32, device='cuda')
            d_ev = torch.empty(cap, dtype=torch.int64, device='cuda')
            d_cnt = torch.zeros(2, dtype=torch.int64, device='cuda')
            torch.cuda.synchronize()
            ch.process_device(x[2 * k * S:2 * (k + 1) * S], S, d_ph, d_ev, cap, d_cnt)
            ch.capture_pulses_counted(d_ph, J, k * J, d_ev, d_cnt[1:], cap, *bank)
            torch.cuda.synchronize()
            n = int(d_cnt[1].item())
            calls.append((d_ph.cpu().numpy(), k * J, d_ev[:n].cpu().numpy().view(np.uint64)))
        got = _host(bank)
    finally:
        ch.close()
    ref = cr.capture(calls, C, L, pre, R, cr.pend_cap(L, pre, DEAD))
    assert ref.stats['recorded'] >= 20 and ref.stats['spanned'] > 0, ref.stats
    _same(ref, got)


def _filter_stream(C=64, npulse=260, gap=2200, chans=(5, 40)):
    """Two channels carry `npulse` pulses of the fake_pulses shape (tests/template_pulses.py) as a
    negative-going phase of 0.4 rad, `gap` rows apart, noise sigma 0.01; the others are zero.
    Packets sit at the pulse peaks, up to 5 rows off."""
    rng = np.random.default_rng(74)
    rows = 1000 + npulse * gap + 1200
    phase = np.zeros((rows, C), np.float32)
    t = np.arange(1000, dtype=np.float32)
    shape = ((1.0 - np.exp(-t / 0.1)) * np.exp(-t / 65.0)).astype(np.float32)
    pairs = []
    for c in chans:
        col = (rng.normal(size=rows) * 0.01).astype(np.float32)
        for p in range(npulse):
            start = 1000 + p * gap + int(rng.integers(0, 64))
            col[start:start + 1000] -= np.float32(0.4) * shape
            pairs.append((c, start + 1 + int(rng.integers(-5, 6))))
        phase[:, c] = col
    return phase, pairs


@pytest.mark.gpu
def test_capture_filters_from_bank(gpu):
    from oracle import template_ref
    from mkids_sdr_amd import template
    from mkids_sdr_amd.channelizer import Channelizer
    C, L, pre, R, chans = 64, 2000, 1000, 256, (5, 40)
    phase, pairs = _filter_stream(C, chans=chans)
    rows = phase.shape[0]
    cuts = [2 ** 16] * (rows // 2 ** 16) + ([rows % 2 ** 16] if rows % 2 ** 16 else [])
    calls = _calls(phase, pairs, cuts)
    ref = cr.capture(calls, C, L, pre, R, cr.pend_cap(L, pre, DEAD))
    assert ref.info[list(chans), 0].tolist() == [R, R] and ref.stats['dropped'] == 8 and ref.stats['spanned'] > 0
    fallback = np.arange(100, dtype=np.float32)
    ch = Channelizer(C, max_chunk=2 ** 14)
    try:
        ch.set_capture(L, pre, R)
        bank = _device_run(ch, calls)
        _same(ref, _host(bank))
        got = template.filters_from_bank(ch, bank, ncoeff=100, pre=100, min_records=20, fallback=fallback,
                                         keep_templates=True)
    finally:
        ch.close()
    for c in range(C):
        if c in chans:
            continue
        assert not got['used'][c] and np.array_equal(got['coeff'][c], fallback)
    for c in chans:
        I, Q = template.iq_from_phase(ref.records[c, :ref.info[c, 0]])
        r = template_ref.make_template(I, Q)
        assert r['count1'] > 200
        assert got['used'][c] and got['count'][c] == r['count']
        assert got['flag'][c] == r['flag'] and got['pstart'][c] == r['pstart']
        tpl, noise = got['templates'][c]
        np.testing.assert_allclose(tpl, r['template'], rtol=0, atol=2e-5)
        np.testing.assert_allclose(noise, r['noise'], rtol=2e-4, atol=1e-9 * r['noise'].max())
        g_ref = template_ref.optimal_filter(r['template'], r['noise'])
        np.testing.assert_allclose(got['coeff'][c], g_ref, rtol=0, atol=1e-3 * np.abs(g_ref).max())
