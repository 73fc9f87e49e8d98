#!/usr/bin/env python3
"""Time mkid_capture_pulses (k_capture.hip) at config 3's geometry: phase [2^19][1024] (2 GB, one
2^30-sample step, well past the 256 MB Infinity Cache), about 500 packets per channel at least 40
rows apart, records of 2000 rows (pre 1000), 512 per channel. MKID_K_CAPTURE HIP-event time per
launch, median over --reps launches after warm-up, against mkid_stream_copy of the same phase
buffer in the same process. Prints one JSON line per library.

    python tools/capture_rate.py [--reps 20] [--lib build/variants/NAME.so ...]

--lib adds build variants (tools/build_variant.sh) timed in the same process on the same buffers.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(ch, name, launch, reps, warm=3):
    import torch
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    ch.set_timing(True, kernels=[name])
    out, prev = [], 0.0
    for _ in range(reps):
        launch()
        torch.cuda.synchronize()
        tot = ch.timing()[name][0]
        out.append(tot - prev)
        prev = tot
    ch.set_timing(False)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--per-ch', type=int, default=500)
    ap.add_argument('--lib', action='append', default=[])
    args = ap.parse_args()
    import torch
    from mkids_sdr_amd.channelizer import Channelizer
    C, J, L, pre, R = 1024, 1 << 19, 2000, 1000, 512
    rng = np.random.default_rng(0)
    step = (J - 2 * L) // args.per_ch
    assert step >= 72 and args.per_ch <= R
    ts = pre + np.arange(args.per_ch)[None, :] * step + rng.integers(0, step - 40, (C, args.per_ch))
    ev = ((np.arange(C, dtype=np.uint64)[:, None] << np.uint64(52)) | ts.astype(np.uint64)).reshape(-1)
    d_ev = torch.from_numpy(ev.view(np.int64)).cuda()
    d_ph = torch.randn(J, C, device='cuda')
    d_dst = torch.empty_like(d_ph)
    bank = None
    for lib in [None] + args.lib:
        ch = Channelizer(C, max_chunk=1 << 20, lib_path=lib)
        ch.set_capture(L, pre, R)
        if bank is None:
            bank = ch.capture_bank()
        nbytes = d_ph.numel() * 4

        def capture():
            bank[2].zero_()
            torch.cuda.synchronize()     # the zeroing runs on torch's stream
            ch.capture_pulses_device(d_ph, J, 0, d_ev, ev.size, *bank)   # j0 = 0 again: a new segment

        ms, lo, hi = _median_ms(ch, 'k_capture', capture, args.reps)
        info = bank[2].cpu().numpy()
        records = int(info[:, 0].sum())
        assert records == C * args.per_ch and int(info[:, 1].sum()) == 0
        c, k = C // 3, args.per_ch // 2
        s = int(ts[c, k]) - pre
        assert torch.equal(bank[0][c, k], d_ph[s:s + L, c]) and int(bank[1][c, k]) == int(ts[c, k])
        cms, _, _ = _median_ms(ch, 'k_stream_copy', lambda: ch.stream_copy(d_dst, d_ph, nbytes), args.reps)
        written = records * L * 4
        print(json.dumps(dict(kernel='k_capture', lib=lib or 'libmkidgpu.so', channels=C, rows=J, length=L,
                              records=records, ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                              launches=args.reps, bytes_read=nbytes, bytes_written=written,
                              gb_per_s=round((nbytes + written) / ms / 1e6, 1),
                              stream_copy_ms=round(cms, 4), stream_copy_gb_per_s=round(2 * nbytes / cms / 1e6, 1),
                              fraction_of_copy=round((nbytes + written) / ms / (2 * nbytes / cms), 3))),
              flush=True)
        ch.close()


if __name__ == '__main__':
    main()
