"""Resonator loop fits (include/mkidgpu.h mkid_fit_loops): every channel's swept IQ loop fitted with
the reference's ten-parameter model (IQsweep.FitLoopMP, lib/iqsweep.py:141-291) in one device call,
giving Q, f0, the loop centre, Qc, Qi and the dip depth per channel. The model, window, guesses,
bounds, start recipe and derived quantities are the reference's; the solver is the library's own.
"""
import ctypes

import numpy as np

from . import _lib, roach

PARAMS = ('Q', 'f0', 'aleak', 'ph1', 'da', 'ang1', 'Igain', 'Qgain', 'Ioff', 'Qoff')
FIELDS = ('p', 'chisq', 'qc', 'qi', 'dipdb', 'cidx', 'low', 'high', 'n', 'best_start', 'evals', 'status')


def draws(nch, S, seed):
    """The random numbers of lib/iqsweep.py:236-244 for nch channels and S starts -> float64
    [nch][S][5]: g standard normal, u2, u3, u4 uniform in [0, 1), u5 uniform in [-1, 1)."""
    rng = np.random.default_rng(seed)
    d = np.empty((int(nch), int(S), 5), np.float64)
    d[..., 0] = rng.standard_normal((nch, S))
    d[..., 1:4] = rng.random((nch, S, 3))
    d[..., 4] = rng.uniform(-1.0, 1.0, (nch, S))
    return d


def model(p, x):
    """The loop model at frequencies x for parameters p (PARAMS order) -> complex I + iQ, over
    roach.resdiff."""
    return roach.resdiff(x, *[float(v) for v in p])


def _by_field(fits, chisq_all):
    out = {k: fits[k].copy() for k in FIELDS}
    out['chisq_all'] = chisq_all
    return out


def _inputs(freq, I, Q, isd, qsd, dr, qguess):
    f = np.ascontiguousarray(freq, np.float64)
    i = np.ascontiguousarray(I, np.float64)
    q = np.ascontiguousarray(Q, np.float64)
    if not (f.ndim == 2 and f.shape == i.shape == q.shape):
        raise ValueError('freq, I, Q must be [nch][fsteps] of one shape')
    nch, fsteps = f.shape
    d = np.ascontiguousarray(dr, np.float64)
    if d.ndim != 3 or d.shape[0] != nch or d.shape[2] != 5:
        raise ValueError('draws must be [nch][S][5]')
    if (isd is None) != (qsd is None):
        raise ValueError('isd and qsd go together')
    sd = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (isd, qsd)]
    if sd[0] is not None and not (sd[0].shape == sd[1].shape == f.shape):
        raise ValueError('isd, qsd must have the shape of I')
    g = None if qguess is None else np.ascontiguousarray(np.broadcast_to(np.asarray(qguess, np.float64), (nch,)))
    return f, i, q, sd[0], sd[1], d, g, nch, fsteps, d.shape[1]


def fit_loops(chan, freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10):
    """Fit every row of a sweep on the GPU of `chan`: freq (Hz), I, Q float64 [nch][fsteps] (zero point
    subtracted), draws [nch][S][5] (draws()), optional isd, qsd (weights 1 / sd) and qguess [nch].
    One device call on the context's stream, one synchronisation, one copy of the results (144 bytes
    a channel) -> dict of arrays by field (FIELDS), 'p' [nch][10] in PARAMS order, and 'chisq_all'
    [nch][S]."""
    import torch
    dev = chan.torch_device()
    f, i, q, sI, sQ, d, g, nch, fsteps, S = _inputs(freq, I, Q, isd, qsd, draws, qguess)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    t = [up(a) for a in (f, i, q, sI, sQ, d, g)]
    d_fits = torch.zeros(nch * ctypes.sizeof(_lib.LoopFit), dtype=torch.uint8, device=dev)
    d_all = torch.zeros((nch, S), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)      # the uploads run on torch's stream, the kernel on the context's
    chan.fit_loops_device(*t, nch, fsteps, S, max_iter, ftol, d_fits, d_all)
    torch.cuda.synchronize(dev)
    fits = d_fits.cpu().numpy().view(np.dtype(_lib.LOOP_FIT_DTYPE))
    return _by_field(fits, d_all.cpu().numpy())


def fit_loops_host(freq, I, Q, draws, isd=None, qsd=None, qguess=None, max_iter=200, ftol=1e-10):
    """The same call through the host twin (mkid_fit_loops_host); needs no GPU."""
    L = _lib.load()
    f, i, q, sI, sQ, d, g, nch, fsteps, S = _inputs(freq, I, Q, isd, qsd, draws, qguess)
    fits = np.zeros(nch, np.dtype(_lib.LOOP_FIT_DTYPE))
    call = np.zeros((nch, S), np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.mkid_fit_loops_host(p(f), p(i), p(q), p(sI), p(sQ), p(d), p(g), nch, fsteps, S, int(max_iter),
                                     float(ftol), p(fits), p(call)))
    return _by_field(fits, call)
