#!/usr/bin/env python3
"""Time the resonator loop fits (mkid_fit_loops) at the array's size, 2048 channels x 10 starts x 200
sweep steps (a 100-point window), max_iter 200, ftol 1e-10:

  device   HIP-event time around the call on a stream shared with torch, the sweep already on the
           device: median of --reps (5) calls after one warm-up call
  host     wall time of mkid_fit_loops_host on the first --host-channels (64) of the same channels,
           median of --host-reps (3), for context

The loops are synthetic (roach.resdiff, Q 15e3 .. 80e3, noise 1 % of the radius). The device's and
the twin's results on the shared channels are compared loosely (same window; share of channels whose
chi^2 agree to 1e-6) as a sanity check; the tests hold the actual parity. Prints one JSON line.

    python tools/loopfit_time.py [--channels 2048] [--starts 10] [--steps 200] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def loops(nch, fsteps, seed=0, noise=0.01):
    from mkids_sdr_amd import roach
    rng = np.random.default_rng(seed)
    freq, I, Q = (np.zeros((nch, fsteps)) for _ in range(3))
    for c in range(nch):
        Qr, f0, R = rng.uniform(15e3, 80e3), rng.uniform(4e9, 6e9), rng.uniform(2e3, 2e4)
        span = rng.uniform(4.0, 8.0) * f0 / Qr
        cen = rng.uniform(2.0, 5.0, 2) * R * rng.choice([-1.0, 1.0], 2)
        x = f0 + rng.uniform(-0.1, 0.1) * span + np.linspace(-0.5 * span, 0.5 * span, fsteps)
        z = roach.resdiff(x, Qr, f0, rng.uniform(0.01, 0.3), rng.uniform(100.0, 2000.0), rng.uniform(-500.0, 500.0),
                          rng.uniform(-3.0, 3.0), 2.0 * R, 2.0 * R, cen[0], cen[1])
        freq[c] = x
        I[c] = z.real + noise * R * rng.standard_normal(fsteps)
        Q[c] = z.imag + noise * R * rng.standard_normal(fsteps)
    return freq, I, Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=2048)
    ap.add_argument('--starts', type=int, default=10)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--max-iter', type=int, default=200)
    ap.add_argument('--ftol', type=float, default=1e-10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-channels', type=int, default=64)
    ap.add_argument('--host-reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd import _lib, loopfit
    from mkids_sdr_amd.channelizer import Channelizer
    nch, S = args.channels, args.starts
    freq, I, Q = loops(nch, args.steps)
    dr = loopfit.draws(nch, S, 0)
    ch = Channelizer(64, max_chunk=1 << 14)
    s = torch.cuda.Stream()
    ch.set_stream(s.cuda_stream)
    t = [torch.from_numpy(a).cuda() for a in (freq, I, Q)]
    d_dr = torch.from_numpy(dr).cuda()
    d_fits = torch.zeros(nch * ctypes.sizeof(_lib.LoopFit), dtype=torch.uint8, device='cuda')
    call = lambda: ch.fit_loops_device(t[0], t[1], t[2], None, None, d_dr, None, nch, args.steps, S, args.max_iter,
                                       args.ftol, d_fits)
    torch.cuda.synchronize()
    call()
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(s)
        call()
        b.record(s)
        torch.cuda.synchronize()
        t_dev.append(a.elapsed_time(b))
    dev = d_fits.cpu().numpy().view(np.dtype(_lib.LOOP_FIT_DTYPE))
    nh = min(args.host_channels, nch)
    t_host, host = [], None
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        host = loopfit.fit_loops_host(freq[:nh], I[:nh], Q[:nh], dr[:nh], max_iter=args.max_iter, ftol=args.ftol)
        t_host.append((time.perf_counter() - t0) * 1e3)
    out = dict(tool='loopfit_time', channels=nch, starts=S, steps=args.steps, max_iter=args.max_iter, ftol=args.ftol,
               device_ms=round(float(np.median(t_dev)), 3), device_ms_min=round(min(t_dev), 3),
               device_ms_max=round(max(t_dev), 3), device_calls=len(t_dev),
               device_us_per_channel=round(1e3 * float(np.median(t_dev)) / nch, 2),
               device_evals_best_start_mean=round(float(dev['evals'].mean()), 1),
               device_status_counts={int(k): int(v) for k, v in zip(*np.unique(dev['status'], return_counts=True))})
    if host is not None:
        hm = float(np.median(t_host))
        with np.errstate(all='ignore'):
            close = np.abs(dev['chisq'][:nh] / host['chisq'] - 1.0) < 1e-6
        out.update(host_channels=nh, host_ms=round(hm, 1), host_ms_min=round(min(t_host), 1), host_calls=len(t_host),
                   host_ms_per_channel=round(hm / nh, 2),
                   host_ms_scaled_to_all_channels=round(hm / nh * nch, 0),
                   same_window=bool(np.array_equal(dev['cidx'][:nh], host['cidx'])),
                   chisq_within_1e6_share=round(float(np.mean(close)), 3))
    print(json.dumps(out), flush=True)
    ch.set_stream(None)
    ch.close()


if __name__ == '__main__':
    main()
