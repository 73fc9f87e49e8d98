#!/usr/bin/env python3
"""Time the threshold rule on one quiet Fix16_13 phase block three ways, in one process, at config
3's shape [8192][1024] and at [8192][2048]:

  device   mkid_phase_thresholds (init, range pass, count pass, finish) on a block that is already
           on the device: HIP-event time around the call on a stream shared with torch, median of
           --reps (20) calls after a warm-up call that grows the workspace
  host     codecs.thresholds_from_phase_block on the same block: wall time of the copy to the host
           plus the per-channel numpy loop, median of --loop-reps (3)
  copy     mkid_stream_copy of twice the block's bytes (HIP events, median of --reps): what two
           passes over the block cost when they stream from memory, the floor for range + count

The block: per-channel Gaussian noise, sigma 20..200 counts around offsets within +-2000 counts,
generated on the device. The thresholds of the two paths are compared. Prints one JSON line per shape.

    python tools/thresholds_rate.py [--reps 20] [--loop-reps 3] [--rows 8192] [--channels 1024 2048]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quiet_block(rows, C, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    sigma = 20.0 + 180.0 * torch.rand((1, C), generator=g, device='cuda')
    off = 4000.0 * torch.rand((1, C), generator=g, device='cuda') - 2000.0
    x = torch.randn((rows, C), generator=g, device='cuda') * sigma + off
    return torch.round(x).clamp(-25736, 25736).to(torch.int16).contiguous()


def events_ms(stream, fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--loop-reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--channels', type=int, nargs='+', default=[1024, 2048])
    ap.add_argument('--nsigma', type=float, default=2.5)
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd import codecs
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(64, max_chunk=1 << 14)
    s = torch.cuda.Stream()
    ch.set_stream(s.cuda_stream)
    for C in args.channels:
        rows = args.rows
        raw = quiet_block(rows, C)
        nbytes = raw.numel() * 2
        d_thr = torch.zeros(C, dtype=torch.int32, device='cuda')
        call = lambda: ch.phase_thresholds_device(raw, rows, C, C, args.nsigma, d_thr)
        call()                                  # warm-up: grows the workspace
        torch.cuda.synchronize()
        t_dev = events_ms(s, call, args.reps)
        src = torch.zeros(2 * nbytes, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        copy = lambda: ch.stream_copy(dst.data_ptr(), src.data_ptr(), 2 * nbytes)
        copy()
        t_copy = events_ms(s, copy, args.reps)
        t_host, ref = [], None
        for _ in range(args.loop_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = codecs.thresholds_from_phase_block(raw.cpu().numpy(), args.nsigma)
            t_host.append((time.perf_counter() - t0) * 1e3)
        dev = float(np.median(t_dev))
        cp = float(np.median(t_copy))
        out = dict(tool='thresholds_rate', rows=rows, channels=C, block_bytes=nbytes, nsigma=args.nsigma,
                   row_block=ch.phase_thresholds_block_rows(rows, C, C, raw.data_ptr() % 16 == 0),
                   device_ms=round(dev, 4), device_ms_min=round(min(t_dev), 4), device_ms_max=round(max(t_dev), 4),
                   device_calls=len(t_dev),
                   device_block_gb_per_s_two_passes=round(2 * nbytes / dev / 1e6, 1),
                   copy_ms=round(cp, 4), copy_ms_min=round(min(t_copy), 4), copy_ms_max=round(max(t_copy), 4),
                   copy_bytes_each_way=2 * nbytes, copy_gb_per_s_read_plus_write=round(4 * nbytes / cp / 1e6, 1),
                   device_over_copy=round(dev / cp, 2),
                   host_ms=round(float(np.median(t_host)), 1) if t_host else None,
                   host_ms_min=round(min(t_host), 1) if t_host else None, host_calls=len(t_host),
                   same_thresholds=bool(np.array_equal(ref, d_thr.cpu().numpy())) if ref is not None else None)
        print(json.dumps(out), flush=True)
    ch.set_stream(None)
    ch.close()


if __name__ == '__main__':
    main()
