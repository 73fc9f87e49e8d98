"""Welch noise spectra and the 1 kHz frequency noise of every resonator (include/mkidgpu.h
mkid_welch_psd, mkid_iq_noise): IQsweep.AnalyzeNoise (lib/iqsweep.py:770-822) for all channels in one
device call. A long int16 IQ record per channel is moved to the fitted loop centre, rotated and
normalised; matplotlib.mlab.psd-style Welch spectra of its phase and amplitude at two resolutions are
stitched into one spectrum, and fn1k is read off a line through a few bins around 1 kHz, over 16 Q^2.
"""
import ctypes

import numpy as np

from . import _lib

# the reference's values (LoadNoise :750, AnalyzeNoise :775-822)
DEFAULTS = dict(nfft_low=262144, nfft_high=4096, k_join=8, fit_first=521, fit_count=5, group=0, samprate=200000.0,
                f_eval=1000.0, gain=0.2, full_scale=32767.0)
RESULT_FIELDS = ('mean_i', 'mean_q', 'resang', 'rad', 'fn1k', 'sum_i', 'sum_q', 'nseg_low', 'nseg_high', 'status')
NOISE_HEADER, NOISE_BLOCK, NOISE_BLOCKS = 12, 200000, 10     # LoadNoise's file layout


def make_cfg(**kw):
    """mkid_iqnoise_cfg from DEFAULTS and the overrides."""
    bad = set(kw) - set(DEFAULTS)
    if bad:
        raise TypeError('unknown noise settings: %s' % sorted(bad))
    v = dict(DEFAULTS, **kw)
    c = _lib.IqNoiseCfg()
    for k, x in v.items():
        setattr(c, k, float(x) if k in ('samprate', 'f_eval', 'gain', 'full_scale') else int(x))
    return c


def nout(cfg):
    """Stitched bins: r k_join + nfft_high / 2 - k_join (2552 for the reference's values)."""
    return (cfg.nfft_low // cfg.nfft_high) * cfg.k_join + cfg.nfft_high // 2 - cfg.k_join


def freqs(cfg=None, **kw):
    """The stitched frequency axis (mkid_iq_noise_freqs): each bin at its own resolution."""
    cfg = cfg if cfg is not None else make_cfg(**kw)
    out = np.zeros(max(nout(cfg), 1), np.float64)
    _lib.check(_lib.load().mkid_iq_noise_freqs(ctypes.byref(cfg), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def _series(a, b):
    a = np.ascontiguousarray(np.atleast_2d(a), np.float64)
    if b is not None:
        b = np.ascontiguousarray(np.atleast_2d(b), np.float64)
        if b.shape != a.shape:
            raise ValueError('a and b must have one shape [nch][n]')
    return a, b


def welch(chan, a, b, nfft, fs, group=0):
    """matplotlib.mlab.psd's defaults (Hanning, no detrending, one-sided density, half overlap) for the
    rows of a and b (float64 [nch][n]; b may be None) on the GPU of `chan` -> (pa, pb) [nch][nfft/2+1]
    (pb None without b)."""
    import torch
    dev = chan.torch_device()
    a, b = _series(a, b)
    nch, n = a.shape
    d_a = torch.from_numpy(a).to(dev)
    d_b = None if b is None else torch.from_numpy(b).to(dev)
    nb = max(int(nfft) // 2 + 1, 1)
    d_pa = torch.zeros((nch, nb), dtype=torch.float64, device=dev)
    d_pb = None if b is None else torch.zeros((nch, nb), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)      # the uploads run on torch's stream, the kernels on the context's
    chan.welch_psd_device(d_a, d_b, n, n, nch, nfft, fs, group, d_pa, d_pb)
    torch.cuda.synchronize(dev)
    return d_pa.cpu().numpy(), None if d_pb is None else d_pb.cpu().numpy()


def welch_host(a, b, nfft, fs, group=0):
    """The same call through the host twin (mkid_welch_psd_host); needs no GPU."""
    a, b = _series(a, b)
    nch, n = a.shape
    nb = max(int(nfft) // 2 + 1, 1)
    pa = np.zeros((nch, nb), np.float64)
    pb = None if b is None else np.zeros((nch, nb), np.float64)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.load().mkid_welch_psd_host(p(a), p(b), n, n, nch, int(nfft), float(fs), int(group), p(pa), p(pb)))
    return pa, pb


def _records(I, Q, fits, i0, q0):
    I = np.ascontiguousarray(np.atleast_2d(I), np.int16)
    Q = np.ascontiguousarray(np.atleast_2d(Q), np.int16)
    if I.shape != Q.shape:
        raise ValueError('I and Q must be int16 [nch][n] of one shape')
    nch = I.shape[0]
    p = np.asarray(fits['p'], np.float64)
    if p.shape != (nch, 10):
        raise ValueError("fits['p'] must be [nch][10] (loopfit.fit_loops)")
    col = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (nch,)))
    return I, Q, col(i0), col(q0), col(p[:, 8]), col(p[:, 9]), col(p[:, 0])


def _by_field(cfg, pn, an, res):
    out = {k: res[k].copy() for k in RESULT_FIELDS}
    out.update(pn=pn, an=an, freq=freqs(cfg))
    return out


def analyze_noise(chan, I, Q, fits, i0=0, q0=0, **cfg):
    """AnalyzeNoise for every row of the int16 records I, Q [nch][n] on the GPU of `chan`. fits is the
    dict loopfit.fit_loops returns (p[:, 8], p[:, 9]: the loop centre; p[:, 0]: Q); i0, q0 the zero
    point (scalar or [nch]); cfg overrides DEFAULTS. One device call, one synchronisation -> dict(pn,
    an [nch][nout], freq [nout], fn1k, resang, rad, status, mean_i, mean_q, sum_i, sum_q, nseg_low,
    nseg_high)."""
    import torch
    dev = chan.torch_device()
    c = make_cfg(**cfg)
    I, Q, z_i, z_q, icen, qcen, qfit = _records(I, Q, fits, i0, q0)
    nch, n = I.shape
    t = [torch.from_numpy(a).to(dev) for a in (I, Q, z_i, z_q, icen, qcen, qfit)]
    no = max(nout(c), 1)
    d_pn = torch.zeros((nch, no), dtype=torch.float64, device=dev)
    d_an = torch.zeros((nch, no), dtype=torch.float64, device=dev)
    d_res = torch.zeros(nch * ctypes.sizeof(_lib.IqNoiseResult), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    chan.iq_noise_device(t[0], t[1], n, n, nch, t[2], t[3], t[4], t[5], t[6], c, d_pn, d_an, d_res)
    torch.cuda.synchronize(dev)
    res = d_res.cpu().numpy().view(np.dtype(_lib.IQ_NOISE_DTYPE))
    return _by_field(c, d_pn.cpu().numpy(), d_an.cpu().numpy(), res)


def analyze_noise_host(I, Q, fits, i0=0, q0=0, **cfg):
    """The same call through the host twin (mkid_iq_noise_host); needs no GPU."""
    c = make_cfg(**cfg)
    I, Q, z_i, z_q, icen, qcen, qfit = _records(I, Q, fits, i0, q0)
    nch, n = I.shape
    no = max(nout(c), 1)
    pn, an = np.zeros((nch, no), np.float64), np.zeros((nch, no), np.float64)
    res = np.zeros(nch, np.dtype(_lib.IQ_NOISE_DTYPE))
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.load().mkid_iq_noise_host(p(I), p(Q), n, n, nch, p(z_i), p(z_q), p(icen), p(qcen), p(qfit),
                                              ctypes.byref(c), p(pn), p(an), p(res)))
    return _by_field(c, pn, an, res)


def load_noise(path, resnum):
    """IQsweep.LoadNoise's file layout (lib/iqsweep.py:738-768): a header of 12 float64, then ten
    blocks of 200000 int16 I, 200000 int16 Q of resonator 0 followed by the same of resonator 1
    -> (header, I, Q) with I, Q int16 [2000000] of resonator `resnum` (0, or anything else for 1)."""
    hdr = np.fromfile(path, np.float64, NOISE_HEADER)
    body = np.fromfile(path, np.int16, offset=8 * NOISE_HEADER)
    if len(hdr) < NOISE_HEADER or len(body) < 4 * NOISE_BLOCK * NOISE_BLOCKS:
        raise ValueError('%s is no noise file: %d header values, %d samples' % (path, len(hdr), len(body)))
    blocks = body[:4 * NOISE_BLOCK * NOISE_BLOCKS].reshape(NOISE_BLOCKS, 4, NOISE_BLOCK)
    k = 0 if resnum == 0 else 2
    return hdr, blocks[:, k].reshape(-1).copy(), blocks[:, k + 1].reshape(-1).copy()
