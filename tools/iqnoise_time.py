#!/usr/bin/env python3
"""Time the IQ noise analysis (mkid_iq_noise) at the reference's shape, 2 000 000 int16 IQ pairs per
resonator at 262144 / 4096 / 8 / 521 / 5, for --channels (256: 2 GB of records) resonators:

  cold    host wall time of the first call of a context, to the end of a synchronise: it makes and
          uploads the tables of both lengths and allocates the workspace
  warm    HIP-event time around each of --reps (3) further calls on a stream shared with torch

The records are synthetic (sigma 30 counts about (3000, -2000), made on the device). The first
--check channels are compared with the host twin (largest |difference| over the tests' bar) as a
sanity check; the tests hold the actual parity. Prints one JSON line.

    python tools/iqnoise_time.py [--channels 256] [--reps 3] [--check 1]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--rows', type=int, default=2000000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--check', type=int, default=1)
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd import _lib, iqnoise
    from mkids_sdr_amd.channelizer import Channelizer
    nch, n = args.channels, args.rows
    cfg = iqnoise.make_cfg()
    gen = torch.Generator(device='cuda').manual_seed(1)
    d_i = torch.empty((nch, n), dtype=torch.int16, device='cuda')
    d_q = torch.empty((nch, n), dtype=torch.int16, device='cuda')
    for c in range(nch):
        d_i[c] = (3000.0 + 30.0 * torch.randn(n, device='cuda', generator=gen)).round().to(torch.int16)
        d_q[c] = (-2000.0 + 30.0 * torch.randn(n, device='cuda', generator=gen)).round().to(torch.int16)
    rng = np.random.default_rng(2)
    off = dict(i0=rng.uniform(-1e-3, 1e-3, nch), q0=rng.uniform(-1e-3, 1e-3, nch), icen=rng.uniform(5e-3, 9e-3, nch),
               qcen=rng.uniform(-5e-3, -2e-3, nch), qfit=rng.uniform(1.5e4, 4e4, nch))
    t = [torch.from_numpy(off[k]).cuda() for k in ('i0', 'q0', 'icen', 'qcen', 'qfit')]
    no = iqnoise.nout(cfg)
    d_pn = torch.zeros((nch, no), dtype=torch.float64, device='cuda')
    d_an = torch.zeros((nch, no), dtype=torch.float64, device='cuda')
    d_res = torch.zeros(nch * ctypes.sizeof(_lib.IqNoiseResult), dtype=torch.uint8, device='cuda')
    ch = Channelizer(64, max_chunk=1 << 14)
    s = torch.cuda.Stream()
    ch.set_stream(s.cuda_stream)
    call = lambda: ch.iq_noise_device(d_i, d_q, n, n, nch, *t, cfg, d_pn, d_an, d_res)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    cold = (time.perf_counter() - t0) * 1e3
    first = (d_pn.cpu().numpy(), d_res.cpu().numpy())
    warm = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(s)
        call()
        b.record(s)
        torch.cuda.synchronize()
        warm.append(a.elapsed_time(b))
    same = bool(np.array_equal(first[0], d_pn.cpu().numpy()) and np.array_equal(first[1], d_res.cpu().numpy()))
    res = d_res.cpu().numpy().view(np.dtype(_lib.IQ_NOISE_DTYPE))
    wm = float(np.median(warm))
    out = dict(tool='iqnoise_time', channels=nch, rows=n, nfft_low=cfg.nfft_low, nfft_high=cfg.nfft_high,
               record_gbytes=round(4.0 * nch * n / 1e9, 3), cold_ms=round(cold, 1), warm_ms=round(wm, 1),
               warm_ms_min=round(min(warm), 1), warm_ms_max=round(max(warm), 1), warm_calls=len(warm),
               warm_ms_per_channel=round(wm / nch, 3), repeat_same_bits=same,
               status_counts={int(k): int(v) for k, v in zip(*np.unique(res['status'], return_counts=True))})
    if args.check > 0:
        import iqnoise_cases as nc
        k = min(args.check, nch)
        I, Q = d_i[:k].cpu().numpy(), d_q[:k].cpu().numpy()
        sub = {key: v[:k] for key, v in off.items()}
        t0 = time.perf_counter()
        host = iqnoise.analyze_noise_host(I, Q, nc.fits_of(sub), i0=sub['i0'], q0=sub['q0'])
        out.update(host_twin_ms_per_channel=round((time.perf_counter() - t0) * 1e3 / k, 1))
        ref = nc.iq_ref(I, Q, sub, dict(iqnoise.DEFAULTS))
        ref['qfit'] = sub['qfit']
        got = dict(pn=first[0][:k], an=d_an[:k].cpu().numpy(), freq=host['freq'],
                   **{f: res[f][:k] for f in iqnoise.RESULT_FIELDS})
        with contextlib.redirect_stdout(io.StringIO()):      # compare_noise prints every figure
            worst = nc.compare_noise(got, nc.with_sums(host, ref), dict(iqnoise.DEFAULTS), 'time')
        out.update(checked_channels=k, largest_ratio_to_bar=round(worst, 5))
    print(json.dumps(out), flush=True)
    ch.set_stream(None)
    ch.close()


if __name__ == '__main__':
    main()
