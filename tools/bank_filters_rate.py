#!/usr/bin/env python3
"""Time the bank -> filter-table step both ways on one bank, in one process: the per-channel host
loop (template.filters_from_bank) and the single device call (template.filters_from_bank_device,
mkid_bank_filters). Config 3's channel count, C = 1024, with R = 128 phase records per channel:
negative-going pulses of 0.4 rad on a resting phase of 0.5 rad, noise sigma 0.02, rolled by -3..3
(the recipe of tests/template_pulses.phase_records), generated once on the device.

Wall clock around a synchronised call: the median of --loop-reps calls of the loop and of
--reps calls of the device path, in rounds that alternate which of the two goes first. For the device
path also the HIP-event time of the launches alone (outputs allocated beforehand), accepted pulses
per second and float64 FMA/s (1.56 M FMAs of convolution + 1.28 M of DFT per accepted pulse in
pass 2) against the chip's FP64 vector rate. Prints one JSON line.

    python tools/bank_filters_rate.py [--reps 20] [--loop-reps 5] [--channels 1024] [--records 128]
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

FMA_PER_PULSE = 1.56e6 + 1.28e6
FP64_VECTOR_FMA_PER_S = 78.6e12 / 2    # MI355X data sheet: 78.6 TFLOP/s FP64 vector


def make_bank(C, R, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.arange(1000, dtype=torch.float64, device='cuda')
    shape = torch.zeros(2000 + 8, dtype=torch.float64, device='cuda')
    shape[1004:2004] = -0.4 * (1.0 - torch.exp(-t / 0.1)) * torch.exp(-t / 65.0)
    rec = torch.empty((C, R, 2000), dtype=torch.float32, device='cuda')
    idx = torch.arange(2000, device='cuda')
    for c in range(C):   # a channel at a time keeps the float64 temporaries small
        roll = torch.randint(-3, 4, (R, 1), generator=g, device='cuda')
        ph = shape[(idx[None, :] + 4 - roll)] + torch.randn((R, 2000), generator=g, device='cuda',
                                                            dtype=torch.float64) * 0.02 + 0.5
        rec[c] = torch.remainder(ph + np.pi, 2 * np.pi) - np.pi
    info = torch.zeros((C, 2), dtype=torch.int32, device='cuda')
    info[:, 0] = R
    return rec, torch.zeros((C, R), dtype=torch.int64, device='cuda'), info


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--loop-reps', type=int, default=5)
    ap.add_argument('--channels', type=int, default=1024)
    ap.add_argument('--records', type=int, default=128)
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd import _lib, template
    from mkids_sdr_amd.channelizer import Channelizer
    C, R = args.channels, args.records
    bank = make_bank(C, R)
    ch = Channelizer(64, max_chunk=1 << 14)
    loop = lambda: template.filters_from_bank(ch, bank)
    device = lambda: template.filters_from_bank_device(ch, bank)
    _, dev_out = wall(device)            # warm-up: grows the workspace
    per_round = max(args.reps // max(args.loop_reps, 1), 1)
    t_loop, t_dev, order, loop_out = [], [], [], None
    for k in range(args.loop_reps):
        first = 'loop' if k % 2 == 0 else 'device'
        order.append(first)
        for which in ((first, 'device' if first == 'loop' else 'loop')):
            if which == 'loop':
                ms, loop_out = wall(loop)
                t_loop.append(ms)
            else:
                t_dev += [wall(device)[0] for _ in range(per_round)]
        print('round %d: loop %.0f ms, device %.1f ms' % (k, t_loop[-1], t_dev[-1]), file=sys.stderr, flush=True)
    while len(t_dev) < args.reps:
        t_dev.append(wall(device)[0])
    # the launches alone, by HIP events on a stream shared with torch
    s = torch.cuda.Stream()
    ch.set_stream(s.cuda_stream)
    coeff = torch.zeros((C, 100), dtype=torch.float32, device='cuda')
    result = torch.zeros((C, ctypes.sizeof(_lib.BankResult)), dtype=torch.uint8, device='cuda')
    cfg = _lib.BankCfg(C, R, 2000, 20, 100, 100, 2, 0, -1.0)
    t_ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(s)
        ch._chk(ch._L.mkid_bank_filters(ch._h, ctypes.c_void_p(bank[0].data_ptr()), None,
                                        ctypes.c_void_p(bank[2].data_ptr()), ctypes.byref(cfg), None, None,
                                        ctypes.c_void_p(coeff.data_ptr()), ctypes.c_void_p(result.data_ptr())))
        b.record(s)
        torch.cuda.synchronize()
        t_ev.append(a.elapsed_time(b))
    ch.set_stream(None)
    table = template.result_table(result)
    accepted = float(table['count'].sum())
    out = dict(tool='bank_filters_rate', channels=C, records_per_channel=R, used_channels=int(dev_out['used'].sum()),
               accepted_pulses=accepted, run_order_first=order,
               loop_ms=round(float(np.median(t_loop)), 2), loop_ms_min=round(min(t_loop), 2),
               loop_ms_max=round(max(t_loop), 2), loop_calls=len(t_loop),
               device_ms=round(float(np.median(t_dev)), 3), device_ms_min=round(min(t_dev), 3),
               device_ms_max=round(max(t_dev), 3), device_calls=len(t_dev),
               ratio=round(float(np.median(t_loop) / np.median(t_dev)), 1),
               launches_ms=round(float(np.median(t_ev)), 3), launches_ms_min=round(min(t_ev), 3),
               launches_ms_max=round(max(t_ev), 3))
    sec = np.median(t_ev) * 1e-3
    out.update(accepted_pulses_per_s=round(accepted / sec, 1), fp64_fma_per_s=float('%.4g' % (accepted * FMA_PER_PULSE / sec)),
               fraction_of_fp64_vector_rate=round(accepted * FMA_PER_PULSE / sec / FP64_VECTOR_FMA_PER_S, 4),
               bank_bytes=int(bank[0].numel() * 4),
               bank_read_gb_per_s=round(3 * bank[0].numel() * 4 / sec / 1e9, 1))
    if loop_out is not None:   # the two paths agree on what they used
        out['same_used_channels'] = bool(np.array_equal(loop_out['used'], dev_out['used']))
        out['same_counts'] = bool(np.array_equal(loop_out['count'], dev_out['count']))
        out['max_coeff_difference'] = float(np.abs(loop_out['coeff'] - dev_out['coeff']).max())
    print(json.dumps(out), flush=True)
    ch.close()


if __name__ == '__main__':
    main()
