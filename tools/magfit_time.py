#!/usr/bin/env python3
"""Time the resonator magnitude fits (mkid_fit_mags), the loop fits they seed and the chain of the
two at the array's size, 2048 channels x 10 starts x 200 sweep steps, max_iter 200, ftol 1e-10, in one
run on the same loops (tools/loopfit_time.py's):

  mags    mkid_fit_mags writing d_qout
  loops   mkid_fit_loops with the ladder of Q starts (no d_qguess)
  chain   mkid_fit_mags, then mkid_fit_loops with d_qout as d_qguess, on the same stream

each a HIP-event time around the call(s) on a stream shared with torch, the sweep already on the
device: median of --reps (5) after one warm-up. The magnitude fit's results on the first
--host-channels (64) are compared with the host twin's bytes as a sanity check (the tests hold the
parity), and the twin's wall time is given for context. Prints one JSON line.

    python tools/magfit_time.py [--channels 2048] [--starts 10] [--steps 200] [--reps 5]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=2048)
    ap.add_argument('--starts', type=int, default=10)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--max-iter', type=int, default=200)
    ap.add_argument('--ftol', type=float, default=1e-10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-channels', type=int, default=64)
    args = ap.parse_args()
    import torch

    from loopfit_time import loops
    from mkids_sdr_amd import _lib, loopfit
    from mkids_sdr_amd.channelizer import Channelizer
    nch, S, fsteps = args.channels, args.starts, args.steps
    freq, I, Q = loops(nch, fsteps)
    md, ld = loopfit.mag_draws(nch, S, 0), loopfit.draws(nch, S, 0)
    ch = Channelizer(64, max_chunk=1 << 14)
    s = torch.cuda.Stream()
    ch.set_stream(s.cuda_stream)
    t = [torch.from_numpy(a).cuda() for a in (freq, I, Q)]
    d_md, d_ld = torch.from_numpy(md).cuda(), torch.from_numpy(ld).cuda()
    d_mags = torch.zeros(nch * ctypes.sizeof(_lib.MagFit), dtype=torch.uint8, device='cuda')
    d_qout = torch.zeros(nch, dtype=torch.float64, device='cuda')
    d_fits = torch.zeros(nch * ctypes.sizeof(_lib.LoopFit), dtype=torch.uint8, device='cuda')
    mags = lambda: ch.fit_mags_device(t[0], t[1], t[2], d_md, nch, fsteps, S, args.max_iter, args.ftol, d_mags, d_qout)
    lps = lambda qg: ch.fit_loops_device(t[0], t[1], t[2], None, None, d_ld, qg, nch, fsteps, S, args.max_iter,
                                         args.ftol, d_fits)
    calls = dict(mags=mags, loops=lambda: lps(None), chain=lambda: (mags(), lps(d_qout)))
    out = dict(tool='magfit_time', channels=nch, starts=S, steps=fsteps, max_iter=args.max_iter, ftol=args.ftol,
               calls=args.reps)
    for name, call in calls.items():
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(s)
            call()
            b.record(s)
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out.update({name + '_ms': round(float(np.median(ms)), 3), name + '_ms_min': round(min(ms), 3),
                    name + '_ms_max': round(max(ms), 3)})
        if name != 'mags':
            f = d_fits.cpu().numpy().view(np.dtype(_lib.LOOP_FIT_DTYPE))
            out.update({name + '_evals_best_start_mean': round(float(f['evals'].mean()), 1),
                        name + '_status_counts': {int(k): int(v) for k, v in zip(*np.unique(f['status'], return_counts=True))}})
    dev = d_mags.cpu().numpy().view(np.dtype(_lib.MAG_FIT_DTYPE))
    out.update(mags_us_per_channel=round(1e3 * out['mags_ms'] / nch, 2),
               mags_evals_best_start_mean=round(float(dev['evals'].mean()), 1),
               mags_status_counts={int(k): int(v) for k, v in zip(*np.unique(dev['status'], return_counts=True))})
    nh = min(args.host_channels, nch)
    if nh > 0:
        t0 = time.perf_counter()
        host = loopfit.fit_mags_host(freq[:nh], I[:nh], Q[:nh], md[:nh], max_iter=args.max_iter, ftol=args.ftol)
        hm = (time.perf_counter() - t0) * 1e3
        same = all(np.ascontiguousarray(dev[k][:nh]).tobytes() == np.ascontiguousarray(host[k]).tobytes()
                   for k in loopfit.MAG_FIELDS)
        out.update(host_channels=nh, host_ms=round(hm, 1), host_ms_scaled_to_all_channels=round(hm / nh * nch, 0),
                   mags_equal_host_twin=bool(same))
    print(json.dumps(out), flush=True)
    ch.set_stream(None)
    ch.close()


if __name__ == '__main__':
    main()
