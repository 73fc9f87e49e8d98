#!/usr/bin/env python3
"""Time the phase-noise spectra of one Fix16_13 phase block, in one process, at the reference's
longsnapshot shape on config 3's geometry: rows = 2^20, nch = ld = 1024, n_averages = 100, so
n = 10485 = 3 * 3 * 5 * 233.

  device      mkid_phase_noise_spectra on a block that is already on the device: HIP-event time
              around the call on a stream shared with torch, median of --reps (20) calls after a
              warm-up call that makes the tables for n
  device_pow2 the same block cut into 128 pieces of n = 8192 = 4^6 * 2: the same column loads
              with passes that cost 26 n per piece instead of 244 n, to tell the column load from
              the generic radix-233 pass; timed in a run of its own, because the context keeps the
              tables of one n and alternating the lengths would upload them on every call
  copy        mkid_stream_copy of the block's bytes (HIP events, median of --reps): what one pass
              over the block costs when it streams
  host        codecs.noise_spectrum on one column (wall clock, median of --loop-reps), times nch

Algorithmic bytes: 2 per sample read plus 8 per output bin. The block is per-channel Gaussian noise,
sigma 20..200 counts around offsets within +-2000 counts, generated on the device; one column of the
device result is compared with the host rule. Prints one JSON line and, with --out, writes it.

    python tools/noise_rate.py [--reps 20] [--loop-reps 3] [--rows 1048576] [--channels 1024]
                               [--averages 100] [--out profiles/noise/noise_rate_c3.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quiet_block(rows, C, seed=0, chunk=1 << 16):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    sigma = 20.0 + 180.0 * torch.rand((1, C), generator=g, device='cuda')
    off = 4000.0 * torch.rand((1, C), generator=g, device='cuda') - 2000.0
    out = torch.empty((rows, C), dtype=torch.int16, device='cuda')
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        x = torch.randn((r1 - r0, C), generator=g, device='cuda') * sigma + off
        out[r0:r1] = torch.round(x).clamp(-25736, 25736).to(torch.int16)
    return out


def event_ms(stream, fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(name, t):
    return {name + '_ms': round(float(np.median(t)), 4), name + '_ms_min': round(min(t), 4),
            name + '_ms_max': round(max(t), 4), name + '_calls': len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--loop-reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--channels', type=int, default=1024)
    ap.add_argument('--averages', type=int, default=100)
    ap.add_argument('--pow2-n', type=int, default=8192)
    ap.add_argument('--norm1', type=float, default=50.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd import codecs
    from mkids_sdr_amd.channelizer import Channelizer
    rows, C, na = args.rows, args.channels, args.averages
    n = rows // na
    na2 = max(rows // args.pow2_n, 1)
    n2 = rows // na2
    ch = Channelizer(64, max_chunk=1 << 14)
    s = torch.cuda.Stream()
    ch.set_stream(s.cuda_stream)
    raw = quiet_block(rows, C)
    nbytes = raw.numel() * 2
    d_spec = torch.zeros((C, n), dtype=torch.float64, device='cuda')
    d_spec2 = torch.zeros((C, n2), dtype=torch.float64, device='cuda')
    scale = codecs.SCALE_TO_ANGLE
    call = lambda: ch.noise_spectra_device(raw, rows, C, C, na, scale, args.norm1, d_spec)
    call2 = lambda: ch.noise_spectra_device(raw, rows, C, C, na2, scale, args.norm1, d_spec2)
    dst = torch.empty_like(raw)
    copy = lambda: ch.stream_copy(dst.data_ptr(), raw.data_ptr(), nbytes)
    # warm-up of every timed shape: code objects, clocks, and the tables of each n
    for fn in (call, call2, copy, copy):
        fn()
    torch.cuda.synchronize()
    # the context keeps the tables of the last n: each length is timed in a run of its own, behind
    # one more call that brings its tables back
    call()
    t_dev = [event_ms(s, call) for _ in range(args.reps)]
    t_copy = [event_ms(s, copy) for _ in range(args.reps)]
    call2()
    t_pow2 = [event_ms(s, call2) for _ in range(args.reps)]
    call()
    torch.cuda.synchronize()
    t_host = []
    col = raw[:, 0].cpu().numpy()
    for _ in range(args.loop_reps):
        t0 = time.perf_counter()
        _, ref = codecs.noise_spectrum(col * scale, na, args.norm1)
        t_host.append((time.perf_counter() - t0) * 1e3)
    got = d_spec[0].cpu().numpy()
    mag = np.abs(np.fft.fft((col[:n * na] * scale).reshape(na, n), axis=1))
    above = mag.min(axis=0) >= 1e-3 * np.sqrt(np.mean(mag[:, 1:] ** 2))   # the bins the tests compare
    dev, cp, p2 = float(np.median(t_dev)), float(np.median(t_copy)), float(np.median(t_pow2))
    alg = nbytes + 8 * C * n
    out = dict(tool='noise_rate', rows=rows, channels=C, n_averages=na, n=n, block_bytes=nbytes,
               algorithmic_bytes=alg, **stats('device', t_dev),
               device_algorithmic_gb_per_s=round(alg / dev / 1e6, 1),
               pow2_n=n2, pow2_n_averages=na2, **stats('device_pow2', t_pow2),
               **stats('copy', t_copy), copy_gb_per_s_read_plus_write=round(2 * nbytes / cp / 1e6, 1),
               device_over_copy=round(dev / cp, 2), device_pow2_over_copy=round(p2 / cp, 2),
               host_one_column_ms=round(float(np.median(t_host)), 2) if t_host else None,
               host_all_columns_ms=round(float(np.median(t_host)) * C, 1) if t_host else None,
               host_calls=len(t_host),
               largest_db_difference_column0=float(np.abs(got - ref)[above].max()) if t_host else None,
               bins_compared_column0=int(above.sum()))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    ch.set_stream(None)
    ch.close()


if __name__ == '__main__':
    main()
