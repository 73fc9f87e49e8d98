"""Context hygiene of the C ABI: several contexts in one process (and from several host threads)
on the same GPU give the results one context gives alone; the device entry point rejects calls
larger than its workspace; packets of a call are channel-major over the whole call."""
import threading

import numpy as np
import pytest

import signals
from test_gpu_parity import configure, quiet_thresholds, sort_events

pytestmark = pytest.mark.gpu


def _run(case, thr, out, key, max_chunk, splits):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(case.C, max_chunk=max_chunk)
    try:
        configure(ch, case, thr)
        ph, ev = [], []
        for a, b in zip(splits[:-1], splits[1:]):
            p, e = ch.process(case.iq[a:b])
            ph.append(p)
            ev.append(e)
        out[key] = (np.concatenate(ph), np.concatenate(ev))
    finally:
        ch.close()


def test_two_contexts_two_threads_same_gpu(gpu):
    C, S = 256, 1 << 20
    cases = [signals.make_case(C, S, seed=s, pulses_per_ch=3.0, noise=100.0) for s in (31, 32)]
    thrs = [quiet_thresholds(C, S // 4, s) for s in (31, 32)]
    splits = [0, S // 2, S]
    alone = {}
    for i in range(2):
        _run(cases[i], thrs[i], alone, i, S, splits)
    both = {}
    ts = [threading.Thread(target=_run, args=(cases[i], thrs[i], both, i, S, splits)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(2):
        assert np.array_equal(alone[i][0], both[i][0])
        assert np.array_equal(alone[i][1], both[i][1])
        assert len(alone[i][1]) > 0
    # the two feedlines are different streams
    assert not np.array_equal(alone[0][0], alone[1][0])


def test_device_call_larger_than_workspace_is_rejected(gpu):
    import torch
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    C = 64
    ch = Channelizer(C, max_chunk=1 << 14)
    try:
        ch.set_iq_tap(3)
        n = 1 << 15
        x = torch.zeros(2 * n, dtype=torch.int16, device='cuda')
        ev = torch.empty(1024, dtype=torch.int64, device='cuda')
        cnt = torch.zeros(2, dtype=torch.int64, device='cuda')
        with pytest.raises(_lib.MkidError):
            ch.process_device(x, n, None, ev, 1024, cnt)
        ch.process_device(x, n // 2, None, ev, 1024, cnt)   # at the limit: fine
        torch.cuda.synchronize()
        assert ch.iq_tap().shape == (n // 2 // (2 * C), 2)
    finally:
        ch.close()


@pytest.mark.parametrize('front', ['auto', 'split'])
def test_packets_channel_major_over_whole_call(gpu, front):
    """Packets come out channel-major and time-ascending over the whole call, on either front end
    (one trigger plan and one compaction per call), at a call size the split front end once cut
    into four pieces."""
    from mkids_sdr_amd.channelizer import Channelizer
    C = 256
    S = 600 * 2 * C          # >= 512 N
    case = signals.make_case(C, S, seed=41, pulses_per_ch=4.0, noise=100.0)
    thr = quiet_thresholds(C, S // 4, 41)
    ch = Channelizer(C, max_chunk=S, front=front)
    try:
        configure(ch, case, thr)
        _, ev = ch.process(case.iq)
    finally:
        ch.close()
    assert len(ev) > 100
    assert np.array_equal(ev, sort_events(ev))


@pytest.mark.parametrize('front', ['auto', 'split'])
def test_raw_phase_is_the_whole_call(gpu, front):
    """mkid_last_raw_phase / mkid_read_raw_phase hold the Fix16_13 phase of the whole last call, from
    row 0: J = 512 rows at C = 64 is the smallest call the split front end once cut into pieces
    (it then reported the last piece only). Element for element the rows are the Fix16_13 of the
    float32 phase the same call returned; so are the 3 rows of a ragged second call."""
    from mkids_sdr_amd.channelizer import Channelizer
    C = 64
    N = 2 * C
    S = 512 * N
    case = signals.make_case(C, 2 * S, seed=47, pulses_per_ch=2.0)
    ch = Channelizer(C, max_chunk=S, front=front)
    try:
        configure(ch, case, np.full(C, -(1 << 30)))
        for a, b in ((0, S), (S, S + 3 * N)):
            ph, _ = ch.process(case.iq[a:b])
            raw = ch.raw_phase()
            assert ph.shape == ((b - a) // N, C) and raw.shape == ph.shape
            want = np.clip(np.rint(ph * np.float32(8192)), -25736, 25736).astype(np.int16)
            assert np.array_equal(raw, want)
            assert int(raw.max()) - int(raw.min()) > 8192   # live phases, not a cleared buffer
    finally:
        ch.close()


def test_split_follows_the_callers_stream(gpu):
    """All work of a split context runs on the stream handed to mkid_set_stream, in call order: two
    process_device calls back to back, then copies of their counts and packets enqueued on that
    same stream and ONE synchronisation of it (no device-wide one) give the packets the same two
    calls give through the synchronous host entry point."""
    import torch
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 64, 1 << 15
    J = S // (2 * C)
    case = signals.make_case(C, 2 * S, seed=48, pulses_per_ch=6.0)
    thr = quiet_thresholds(C, 2 * S, 48)
    ref = Channelizer(C, max_chunk=S, front='split')
    try:
        configure(ref, case, thr)
        want = [ref.process(case.iq[i * S:(i + 1) * S], want_phase=False)[1] for i in range(2)]
    finally:
        ref.close()
    assert min(len(w) for w in want) > 10
    cap = J * C
    st = torch.cuda.Stream()
    ch = Channelizer(C, max_chunk=S, front='split')
    try:
        configure(ch, case, thr)
        ch.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            x = [torch.from_numpy(case.iq[i * S:(i + 1) * S].reshape(-1)).to('cuda') for i in range(2)]
            ev = [torch.empty(cap, dtype=torch.int64, device='cuda') for _ in range(2)]
            cnt = [torch.empty(2, dtype=torch.int64, device='cuda') for _ in range(2)]
            h_ev = [torch.empty(cap, dtype=torch.int64, pin_memory=True) for _ in range(2)]
            h_cnt = [torch.empty(2, dtype=torch.int64, pin_memory=True) for _ in range(2)]
            for i in range(2):
                ch.process_device(x[i], S, None, ev[i], cap, cnt[i])
            for i in range(2):
                h_cnt[i].copy_(cnt[i], non_blocking=True)
                h_ev[i].copy_(ev[i], non_blocking=True)
        st.synchronize()
        for i in range(2):
            n = h_cnt[i].numpy()
            assert n[0] == n[1] == len(want[i])
            assert np.array_equal(h_ev[i].numpy()[:n[1]].view(np.uint64), want[i])
    finally:
        ch.close()


def test_host_call_longer_than_max_chunk_is_channel_major(gpu):
    """mkid_process cuts a call longer than cfg.max_chunk into max_chunk pieces; the pieces'
    lists are merged on the host, so the whole call is channel-major and time-ascending, and the
    packets equal one call through a context whose workspace holds the whole stream."""
    from mkids_sdr_amd.channelizer import Channelizer
    C = 256
    S = 600 * 2 * C
    case = signals.make_case(C, S, seed=43, pulses_per_ch=6.0, noise=100.0)
    thr = quiet_thresholds(C, S // 4, 43)
    out = {}
    for mc in (S, S // 4):
        ch = Channelizer(C, max_chunk=mc)
        try:
            configure(ch, case, thr)
            out[mc] = ch.process(case.iq)
        finally:
            ch.close()
    ev = out[S // 4][1]
    assert len(ev) > 100
    assert np.array_equal(ev, sort_events(ev))
    assert np.array_equal(ev, out[S][1])
    assert np.array_equal(out[S // 4][0], out[S][0])


def test_adc_and_phase_streams_do_not_mix(gpu):
    """A context carries one stream: mkid_trigger_phase on a context mid-ADC-stream (or the
    reverse) fails with MKID_E_STATE instead of shifting the live stream's stamps; after
    mkid_reset_stream either kind may start."""
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 64, 1 << 14
    case = signals.make_case(C, S, seed=44, pulses_per_ch=0.0)
    ch = Channelizer(C, max_chunk=S)
    try:
        configure(ch, case, np.full(C, -(1 << 30)))
        ch.process(case.iq)
        with pytest.raises(_lib.MkidError) as e:
            ch.trigger_phase(np.zeros((8, C), np.int16))
        assert e.value.code == _lib.MKID_E_STATE
        ch.reset()
        ch.trigger_phase(np.zeros((8, C), np.int16))
        with pytest.raises(_lib.MkidError) as e:
            ch.process(case.iq)
        assert e.value.code == _lib.MKID_E_STATE
        ch.reset()
        ch.process(case.iq)
    finally:
        ch.close()


def test_failed_call_after_planning_marks_the_stream(gpu, monkeypatch):
    """a process call that fails after its first launch was enqueued (here an injected
    failure, MKID_FAULT_LAUNCH=1) has advanced the context's stream, so the context is marked as
    carrying an ADC stream: a following mkid_trigger_phase fails with MKID_E_STATE. A call refused in
    planning (a bad size) leaves the stream kind unchanged."""
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 64, 1 << 14
    case = signals.make_case(C, S, seed=45, pulses_per_ch=0.0)
    monkeypatch.setenv('MKID_FAULT_LAUNCH', '1')
    ch = Channelizer(C, max_chunk=S)
    monkeypatch.delenv('MKID_FAULT_LAUNCH')
    try:
        configure(ch, case, np.full(C, -(1 << 30)))
        with pytest.raises(_lib.MkidError) as e:
            ch.process(case.iq[:100])              # not a multiple of N: refused before planning
        assert e.value.code == _lib.MKID_E_ARG
        ch.trigger_phase(np.zeros((8, C), np.int16))   # still a fresh context: allowed
        ch.reset()
        with pytest.raises(_lib.MkidError) as e:
            ch.process(case.iq)                    # the injected failure after the first launch
        assert e.value.code == _lib.MKID_E_HIP and 'injected' in str(e.value)
        with pytest.raises(_lib.MkidError) as e:
            ch.trigger_phase(np.zeros((8, C), np.int16))
        assert e.value.code == _lib.MKID_E_STATE
        ch.reset()
        ch.process(case.iq)                        # the hook fires once
    finally:
        ch.close()


def test_accumulator_rearm_and_failed_call(gpu, monkeypatch):
    """every mkid_set_accumulator(1) restarts the sums (the reference strobes avgIQ_ctrl
    before each startAccumulator 1), armed or not; a process call that fails while the accumulator
    is armed invalidates it (its sums may hold part of that call): mkid_avg_iq then fails with
    MKID_E_STATE until it is re-armed."""
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 64, 1 << 14
    case = signals.make_case(C, S, seed=46, pulses_per_ch=0.0)
    monkeypatch.setenv('MKID_FAULT_LAUNCH', '3')
    ch = Channelizer(C, max_chunk=S)
    monkeypatch.delenv('MKID_FAULT_LAUNCH')
    try:
        configure(ch, case, np.full(C, -(1 << 30)))
        ch.set_accumulator(True)
        ch.process(case.iq[:S // 2])               # launch 1: fine
        a1 = ch.avg_iq()
        ch.set_accumulator(True)                   # re-arm while armed: the sums restart
        with pytest.raises(_lib.MkidError) as e:
            ch.avg_iq()
        assert e.value.code == _lib.MKID_E_STATE   # no rows since the re-arm
        ch.process(case.iq[S // 2:])
        a2 = ch.avg_iq()
        assert not np.array_equal(a1[0], a2[0])    # the second half's own mean, not both halves'
        with pytest.raises(_lib.MkidError) as e:
            ch.process(case.iq[:S // 2])           # launch 3: the injected failure (hook = 3)
        assert e.value.code == _lib.MKID_E_HIP
        with pytest.raises(_lib.MkidError) as e:
            ch.avg_iq()
        assert e.value.code == _lib.MKID_E_STATE and 're-arm' in str(e.value)
        ch.reset()
        ch.set_accumulator(True)
        ch.process(case.iq)
        mi, mq = ch.avg_iq()
        assert np.isfinite(mi).all() and np.isfinite(mq).all()
    finally:
        ch.close()


def test_timing_mask_and_counts_written_per_call(gpu):
    """mkid_set_timing_mask with MKID_TIMING_ONLY bits times only the named kernels (bench.py's timed
    steps record events around the front end alone); d_counts is written by each call's
    compaction (no zeroing launch), so stale values in it do not leak into the next call."""
    import torch
    from mkids_sdr_amd import _lib
    from mkids_sdr_amd.channelizer import Channelizer
    C, S = 256, 1 << 20
    case = signals.make_case(C, S, seed=51, pulses_per_ch=3.0, noise=100.0)
    thr = quiet_thresholds(C, S // 4, 51)
    x = torch.from_numpy(case.iq.reshape(-1)).to('cuda')
    cap = 1 << 16
    res = []
    for junk in (0, 123456789):
        ch = Channelizer(C, max_chunk=S)
        try:
            configure(ch, case, thr)
            ev = torch.empty(cap, dtype=torch.int64, device='cuda')
            cnt = torch.full((2,), junk, dtype=torch.int64, device='cuda')
            ch.set_timing(True, kernels=['k_front'])
            ch.process_device(x, S, None, ev, cap, cnt)
            torch.cuda.synchronize()
            t = ch.timing()
            assert t['k_front'][1] == 1 and t['k_front'][0] > 0
            assert t['k_trigger'][1] == 0 and t['k_compact'][1] == 0
            ch.set_timing(True)
            c = cnt.cpu().numpy().copy()
            ch.process_device(x, S, None, ev, cap, cnt)
            torch.cuda.synchronize()
            t = ch.timing()
            assert t['k_front'][1] == 1 and t['k_trigger'][1] == 1 and t['k_compact'][1] == 1
            with pytest.raises(_lib.MkidError):   # a bit past the last kernel
                ch._chk(ch._L.mkid_set_timing_mask(ch._h, 1 << _lib.K_COUNT))
            # mkid_set_timing keeps its round-1..3 meaning, any non-zero value times
            # every kernel (the mask moved to its own entry point)
            ch._chk(ch._L.mkid_set_timing(ch._h, -1))
            ch._chk(ch._L.mkid_set_timing(ch._h, 2))
            ch.process_device(x, S, None, ev, cap, cnt)
            torch.cuda.synchronize()
            t = ch.timing()
            assert t['k_front'][1] == 1 and t['k_trigger'][1] == 1 and t['k_compact'][1] == 1
            ch.set_timing(False)
            with pytest.raises(ValueError):
                ch.set_timing(True, kernels=['no_such_kernel'])
            res.append((c, ev[:int(c[1])].cpu().numpy()))
        finally:
            ch.close()
    assert res[0][0][0] > 0 and np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])
