"""Energy calibration from laser spectra (include/mkidgpu.h mkid_spectrum_lines): every channel's
laser lines found and fitted in its pulse-height spectrum in one device call, giving the channel's
height -> energy polynomial and resolving power, and the float32 table that the energy cube
(mkid_energy_cube, observe.Observation(energy=...)) reads. The laser box itself is driven by the
reference's dashboard (ArconsDashboard.py toggle_laser / do_cal); the reference holds no solution.
"""
import ctypes

import numpy as np

from . import _lib

NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]   # the NaN an energy is stored as


class EnergyCal:
    """The result of spectrum_lines for nch channels and P lines.

    lines    structured array [nch][P] of _lib.LINE_FIT_DTYPE (bin, nfit, peak_s, counts, mu, sigma, amp)
    cal      structured array [nch] of _lib.ENERGY_CAL_DTYPE (c[3], r[3], n_found, status)
    cal_f    float32 [nch][4]: c0, c1, c2 and 1.0 (usable) or 0.0
    d_cal_f  the same table on the device (a torch tensor), or None for a host-made calibration
    energies the P line energies in eV, in ascending bin order
    """

    def __init__(self, lines, cal, cal_f, energies, d_cal_f=None):
        self.lines, self.cal, self.cal_f = lines, cal, np.ascontiguousarray(cal_f, np.float32)
        self.energies = np.asarray(energies, np.float64)
        self.d_cal_f = d_cal_f

    @property
    def status(self):
        return self.cal['status']

    def usable(self):
        """bool [nch]: all lines found and fitted, and a slope of one sign."""
        return self.cal_f[:, 3] != 0

    def energy(self, ch, h):
        """The fp32 rule of mkid_energy_cube in numpy: e = c0 + h (c1 + h c2), one float32 rounding
        per operation, NaN (0x7FC00000) where channel ch is not usable, h is not finite or the
        arithmetic gives no number. ch and h broadcast."""
        ch = np.asarray(ch, np.int64)
        h = np.asarray(h, np.float32)
        ch, h = np.broadcast_arrays(ch, h)
        cf = self.cal_f[ch]
        with np.errstate(all='ignore'):
            e = (cf[..., 0] + (h * (cf[..., 1] + (h * cf[..., 2]).astype(np.float32)).astype(np.float32))
                 .astype(np.float32)).astype(np.float32)
        bad = (cf[..., 3] == 0) | ~np.isfinite(h) | np.isnan(e)
        return np.where(bad, NAN32, e).astype(np.float32)

    def resolving_power(self):
        """float64 [nch][P]: R = E / (FWHM of the line in energy) at each line, NaN where the channel has
        no calibration."""
        return self.cal['r'][:, :len(self.energies)].copy()

    def device_table(self, chan):
        """The float32 table on the GPU of `chan`, uploaded once when the calibration was made on the host."""
        if self.d_cal_f is None:
            import torch
            self.d_cal_f = torch.from_numpy(self.cal_f).to(chan.torch_device())
            torch.cuda.synchronize(chan.torch_device())
        return self.d_cal_f


def spectrum_lines(chan, d_spectra, lo, step, nbins, energies, smooth=2, min_sep=32, min_peak=10, fit_half=12):
    """The laser lines of every row of d_spectra (a device int32 tensor [nch][nbins + 3], the table
    of mkid_height_spectra; bin b of channel c starts at lo[c] + b step[c], scalars or [nch]) ->
    EnergyCal. One device call on the context's stream, one synchronisation, and the copy of the
    results (48 P + 72 bytes a channel); the float32 table stays on the device for the cube."""
    import torch
    dev = chan.torch_device()
    nch = int(d_spectra.shape[0])
    e = np.ascontiguousarray(energies, np.float64).ravel()
    P = e.size
    lo32 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (nch,)))
    st32 = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (nch,)))
    d_lo, d_step = torch.from_numpy(lo32).to(dev), torch.from_numpy(st32).to(dev)
    d_lines = torch.zeros(nch * max(P, 1) * ctypes.sizeof(_lib.LineFit), dtype=torch.uint8, device=dev)
    d_cal = torch.zeros(nch * ctypes.sizeof(_lib.EnergyCal), dtype=torch.uint8, device=dev)
    d_cal_f = torch.zeros((nch, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)      # the uploads run on torch's stream, the kernel on the context's
    chan.spectrum_lines_device(d_spectra, d_lo, d_step, nch, nbins, e, smooth, min_sep, min_peak, fit_half, d_lines,
                               d_cal, d_cal_f)
    torch.cuda.synchronize(dev)
    lines = d_lines.cpu().numpy().view(np.dtype(_lib.LINE_FIT_DTYPE)).reshape(nch, P)
    cal = d_cal.cpu().numpy().view(np.dtype(_lib.ENERGY_CAL_DTYPE))
    return EnergyCal(lines, cal, d_cal_f.cpu().numpy(), e, d_cal_f)


def spectrum_lines_host(spectra, lo, step, nbins, energies, smooth=2, min_sep=32, min_peak=10, fit_half=12):
    """The same call through the host twin (mkid_spectrum_lines_host): spectra int32 [nch][nbins + 3]
    in host memory -> EnergyCal without a device table; needs no GPU."""
    L = _lib.load()
    sp = np.ascontiguousarray(spectra, np.int32)
    nch = sp.shape[0]
    e = np.ascontiguousarray(energies, np.float64).ravel()
    P = e.size
    lo32 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (nch,)))
    st32 = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (nch,)))
    lines = np.zeros((nch, max(P, 1)), np.dtype(_lib.LINE_FIT_DTYPE))
    cal = np.zeros(nch, np.dtype(_lib.ENERGY_CAL_DTYPE))
    cal_f = np.zeros((nch, 4), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.mkid_spectrum_lines_host(p(sp), p(lo32), p(st32), nch, int(nbins), P, p(e), int(smooth), int(min_sep),
                                          int(min_peak), int(fit_half), p(lines), p(cal), p(cal_f)))
    return EnergyCal(lines[:, :P], cal, cal_f, e)
