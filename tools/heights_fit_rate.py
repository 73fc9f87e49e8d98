#!/usr/bin/env python3
"""Time mkid_pulse_fit (k_heights_fit.hip) against mkid_pulse_heights, in one process, at config 5's
shape: phase [2^18][2048] (one 2^30-sample step at N = 4096), ncoeff = 100, pre = 20, and the packet
volume tools/heights_rate.py takes for a bench step (690 000 packets spread over the channels,
stamps ascending).

  plain     mkid_pulse_heights on the packets: the one-alignment estimate
  fit_L     mkid_pulse_fit with search half-width L = 0, 3, 8
  naive_L   2 L + 1 mkid_pulse_heights calls on the packets stamped ts + d, d = -L .. L: the lag
            values of fit_L without the kernel (the selection would still have to follow)

Every path is one HIP-event interval on a stream shared with torch; the paths alternate inside each
of --reps rounds after two warm-up rounds, and the median, minimum and maximum over the rounds are
reported. The fit's outputs are checked against the naive calls' values on the way: both are fp32
sums, in different orders, so h0 is compared with the plain height within 1e-5 sum |c| max |x|, and
the chosen lag must maximise the naive values within twice that. Prints one JSON line and, with
--out, writes it.

    python tools/heights_fit_rate.py [--reps 20] [--packets 690000] [--out profiles/heightsfit/heights_fit_rate_c5.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEARCHES = (0, 3, 8)


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
            name + '_ms_max': round(max(t), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--packets', type=int, default=690000)
    ap.add_argument('--channels', type=int, default=2048)
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--ncoeff', type=int, default=100)
    ap.add_argument('--pre', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd.channelizer import Channelizer
    C, J, nco, pre, n = args.channels, args.rows, args.ncoeff, args.pre, args.packets
    Lmax = max(SEARCHES)
    rng = np.random.default_rng(0)
    coeff = rng.normal(size=(C, nco)).astype(np.float32)
    s = torch.cuda.Stream()
    plain = Channelizer(C, max_chunk=1 << 20)
    plain.set_stream(s.cuda_stream)
    plain.set_pulse_filter(coeff, pre)
    fits = {}
    for L in SEARCHES:                       # a context each: the search is a property of the context
        fits[L] = Channelizer(C, max_chunk=1 << 20)
        fits[L].set_stream(s.cuda_stream)
        fits[L].set_pulse_filter(coeff, pre)
        fits[L].set_pulse_fit(L, -1)
    d_ph = torch.randn(J, C, device='cuda')
    chs = rng.integers(0, C, n).astype(np.uint64)
    ts = np.sort(rng.integers(pre + Lmax, J - nco - Lmax, n)).astype(np.int64)
    d_ev = {d: torch.from_numpy(((chs << np.uint64(52)) | (ts + d).astype(np.uint64)).view(np.int64)).cuda()
            for d in range(-Lmax, Lmax + 1)}
    d_h = torch.empty(n, dtype=torch.float32, device='cuda')
    d_lags = torch.empty((2 * Lmax + 1, n), dtype=torch.float32, device='cuda')
    out4 = {L: (torch.empty(n, dtype=torch.float32, device='cuda'), torch.empty(n, dtype=torch.float32, device='cuda'),
                torch.empty(n, dtype=torch.int32, device='cuda'), torch.empty(n, dtype=torch.float32, device='cuda'))
            for L in SEARCHES}
    torch.cuda.synchronize()

    def run_plain():
        plain.pulse_heights_device(d_ph, J, 0, d_ev[0], n, d_h)

    def run_fit(L):
        return lambda: fits[L].pulse_fit_device(d_ph, J, 0, d_ev[0], n, *out4[L])

    def run_naive(L):
        def f():
            for d in range(-L, L + 1):
                plain.pulse_heights_device(d_ph, J, 0, d_ev[d], n, d_lags[d + Lmax])
        return f

    paths = [('plain', run_plain)] + [('fit_%d' % L, run_fit(L)) for L in SEARCHES] + \
            [('naive_%d' % L, run_naive(L)) for L in SEARCHES if L > 0]
    times = {name: [] for name, _ in paths}
    for rep in range(args.reps + 2):         # two warm-up rounds: code objects, clocks, caches
        for name, fn in paths:
            t = event_ms(s, fn)
            if rep >= 2:
                times[name].append(t)
    # the fit against the naive calls' values (the last naive round left all 2 Lmax + 1 lags)
    run_naive(Lmax)()
    torch.cuda.synchronize()
    lags = d_lags.cpu().numpy().astype(np.float64)
    scale = 1e-5 * np.abs(coeff).sum(axis=1)[chs.astype(np.int64)] * float(d_ph.abs().max()) + 1e-6
    check = {}
    for L in SEARCHES:
        h, dt, lag, h0 = (o.cpu().numpy() for o in out4[L])
        y = -lags[Lmax - L:Lmax + L + 1]
        k = lag.astype(np.int64) + L
        check['fit_%d' % L] = dict(
            h0_within_bar=bool(np.all(np.abs(h0 - lags[Lmax]) <= scale)),
            lag_near_maximal=bool(np.all(y[k, np.arange(n)] >= y.max(axis=0) - 2 * scale)),
            dt_within_half_row=bool(np.all(np.abs(dt - lag) <= 0.5)),
            interior_fraction=round(float(np.mean(np.abs(lag) < L)), 4) if L else 0.0)
    med = {name: float(np.median(t)) for name, t in times.items()}
    out = dict(tool='heights_fit_rate', channels=C, rows=J, ncoeff=nco, pre=pre, packets=n, reps=args.reps,
               window_bytes_per_packet={('fit_%d' % L): 4 * (nco + 2 * L) for L in SEARCHES})
    for name, t in times.items():
        out.update(stats(name, t))
        out[name + '_mpackets_per_s'] = round(n / med[name] / 1e3, 1)
    for L in SEARCHES:
        out['fit_%d_over_plain' % L] = round(med['fit_%d' % L] / med['plain'], 3)
        if L:
            out['fit_%d_over_naive_%d' % (L, L)] = round(med['fit_%d' % L] / med['naive_%d' % L], 3)
    out['checks'] = check
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    for c in [plain] + list(fits.values()):
        c.set_stream(None)
        c.close()


if __name__ == '__main__':
    main()
