#!/usr/bin/env python3
"""Writes tests/golden/iqnoise_mlab.npz: IQsweep.AnalyzeNoise's arithmetic (lib/iqsweep.py:775-822) on two
synthetic int16 noise records, with matplotlib.mlab.psd and np.polyfit called directly, at a small
shape: n = 20580, NFFT 8192 and 128 with half overlap, 2 high-resolution bins replaced (so 190
stitched bins), the line through stitched bins 140..144 read at 25 kHz. The file holds data only: the
records, the offsets, centres and Q, and what the reference's lines give for them.

    python tools/make_iqnoise_golden.py        (needs matplotlib; the tests only read the file)
"""
import os

import matplotlib.mlab
import numpy as np

N, NFFT_LOW, NFFT_HIGH, K_JOIN, FIT_FIRST, FIT_COUNT = 20580, 8192, 128, 2, 140, 5
SAMPRATE, F_EVAL, GAIN, FULL_SCALE = 200000.0, 25000.0, 0.2, 32767.0
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'iqnoise_mlab.npz')


def analyze(xi, xq, i0, q0, icen, qcen, qres):
    """One record through the reference's steps, in its order of operations (the line numbers are
    lib/iqsweep.py's)."""
    ia = xi * GAIN / FULL_SCALE - i0 - icen                          # :775-776 scale, zero point, centre
    qa = xq * GAIN / FULL_SCALE - q0 - qcen
    ang = np.arctan2(np.mean(qa), np.mean(ia))                       # :779
    rot_i = ia * np.cos(ang) + qa * np.sin(ang)                      # :781-782 rotate onto the I axis
    rot_q = -ia * np.sin(ang) + qa * np.cos(ang)
    rad = np.mean(rot_i)                                             # :784-786 normalise
    rot_i, rot_q = rot_i / rad, rot_q / rad
    phase, amp = np.arctan2(rot_q, rot_i), np.sqrt(rot_i ** 2 + rot_q ** 2)   # :788-789
    psd = lambda x, nfft: matplotlib.mlab.psd(x, NFFT=nfft, Fs=SAMPRATE, noverlap=nfft // 2)   # :792-801
    (p_lo, f_lo), (a_lo, _) = psd(phase, NFFT_LOW), psd(amp, NFFT_LOW)
    (p_hi, f_hi), (a_hi, _) = psd(phase, NFFT_HIGH), psd(amp, NFFT_HIGH)
    jn, top = NFFT_LOW // NFFT_HIGH * K_JOIN, NFFT_HIGH // 2         # :803-817 stitch, Nyquist left out
    pn, an = np.concatenate([p_lo[:jn], p_hi[K_JOIN:top]]), np.concatenate([a_lo[:jn], a_hi[K_JOIN:top]])
    idx = np.concatenate([f_lo[:jn], f_hi[K_JOIN:top]])
    fit = slice(FIT_FIRST, FIT_FIRST + FIT_COUNT)                    # :820-822 the line and fn1k
    line = np.poly1d(np.polyfit(idx[fit], pn[fit], 1))
    return dict(pn=pn, an=an, pnidx=idx, fn1k=line(F_EVAL) / (16.0 * qres ** 2), resang=ang, rad=rad,
                S_low=p_lo.sum() + a_lo.sum(), S_high=p_hi.sum() + a_hi.sum())


def main():
    rng = np.random.default_rng(20221)
    I = np.rint(np.array([[3000.0], [2890.0]]) + 30.0 * rng.standard_normal((2, N))).astype(np.int16)
    Q = np.rint(np.array([[-2000.0], [-2105.0]]) + 30.0 * rng.standard_normal((2, N))).astype(np.int16)
    off = dict(i0=np.array([4e-4, -7e-4]), q0=np.array([-2e-4, 9e-4]), icen=np.array([6.1e-3, 8.4e-3]),
               qcen=np.array([-3.3e-3, -4.6e-3]), qfit=np.array([21500.0, 36250.0]))
    res = [analyze(I[c], Q[c], off['i0'][c], off['q0'][c], off['icen'][c], off['qcen'][c], off['qfit'][c])
           for c in range(2)]
    out = {k: np.array([r[k] for r in res]) for k in res[0]}
    cfg = dict(nfft_low=NFFT_LOW, nfft_high=NFFT_HIGH, k_join=K_JOIN, fit_first=FIT_FIRST, fit_count=FIT_COUNT,
               samprate=SAMPRATE, f_eval=F_EVAL, gain=GAIN, full_scale=FULL_SCALE)
    np.savez_compressed(OUT, I=I, Q=Q, **off, **out, **{'cfg_' + k: np.array(v) for k, v in cfg.items()})
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
