"""Python front-end of one MI355X channeliser context (one feedline on one GPU).

This is the host-side mirror of the firmware configuration the reference performs over katcp
(ROACH_Setup.py / ROACH_Pulses.py) — every setter maps to one register group (see
include/mkidgpu.h) — and of its data path: ``process`` runs the HIP kernels (PFB+FFT+DDC, IQ
low-pass + phase, matched-filter trigger) and returns the phase stream and photon packets.
"""
import ctypes

import numpy as np

from . import _lib, codecs
from .pfb import pfb_prototype


def _ptr(a):
    """Host numpy array / torch tensor / int -> void*."""
    if a is None:
        return None
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    if hasattr(a, 'data_ptr'):
        return ctypes.c_void_p(a.data_ptr())
    return a.ctypes.data_as(ctypes.c_void_p)


class Channelizer:
    def __init__(self, n_channels, device=0, max_chunk=1 << 22, dead_time=32, sample_rate=512e6,
                 max_events_per_ch=0, lib_path=None, front='auto'):
        self._L = _lib.load(lib_path)
        cfg = _lib.Cfg()
        _lib.check(self._L.mkid_default_cfg(ctypes.byref(cfg), int(n_channels)))
        cfg.max_chunk = int(max_chunk)
        cfg.dead_time = int(dead_time)
        cfg.sample_rate = float(sample_rate)
        cfg.max_events_per_ch = int(max_events_per_ch)
        if front not in ('auto', 'split'):
            raise ValueError("front must be 'auto' (fused K1-K6 where supported) or 'split'")
        cfg.front = _lib.FRONT_AUTO if front == 'auto' else _lib.FRONT_SPLIT
        h = ctypes.c_void_p()
        _lib.check(self._L.mkid_create(ctypes.byref(cfg), int(device), ctypes.byref(h)))
        self._h = h
        self.cfg = cfg
        self.device = int(device)
        self.C = cfg.n_channels
        self.N = cfg.fft_len
        self.P = cfg.dds_entries
        self.pulse_filter = None       # (ncoeff, pre) once a pulse filter is set
        self.pulse_fit_search = None   # search half-width once set_pulse_fit ran
        self.set_pfb(pfb_prototype(self.N, cfg.pfb_taps))

    # ---- lifecycle -------------------------------------------------------------------------
    def torch_device(self):
        """The torch device of this context's GPU (allocations for it go there, not to the
        current device)."""
        import torch
        return torch.device('cuda', self.device)

    def close(self):
        if getattr(self, '_h', None):
            self._L.mkid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != _lib.MKID_OK:
            msg = (self._L.mkid_last_error(self._h) or b'').decode(errors='replace')
            raise _lib.MkidError(rc, msg)
        return rc

    # ---- configuration (one register group each) ---------------------------------------------
    def set_stream(self, stream_ptr):
        """Run on an external hipStream_t (e.g. a torch.cuda.Stream's cuda_stream); 0/None
        restores the context's own non-blocking stream. torch's default stream has handle 0, so
        to share a stream with torch work use a torch.cuda.Stream, not the default one."""
        self._chk(self._L.mkid_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def set_pfb(self, coeffs):
        c = np.ascontiguousarray(coeffs, np.float32)
        self._chk(self._L.mkid_set_pfb(self._h, _ptr(c), c.size))

    def set_bins(self, bins):
        b = np.ascontiguousarray(bins, np.int32)
        self._chk(self._L.mkid_set_bins(self._h, _ptr(b), b.size))

    def set_dds(self, lut_i, lut_q):
        li = np.ascontiguousarray(lut_i, np.int16).reshape(self.C, -1)
        lq = np.ascontiguousarray(lut_q, np.int16).reshape(self.C, -1)
        self._chk(self._L.mkid_set_dds(self._h, _ptr(li), _ptr(lq), li.shape[1]))

    def set_lpf(self, taps12):
        t = np.ascontiguousarray(taps12, np.int16)
        self._chk(self._L.mkid_set_lpf(self._h, _ptr(t), t.size))

    def set_fir(self, taps12):
        t = np.ascontiguousarray(taps12, np.int16).reshape(self.C, -1)
        self._chk(self._L.mkid_set_fir(self._h, _ptr(t), t.shape[0], t.shape[1]))

    def set_centers(self, ic, qc):
        i = np.ascontiguousarray(ic, np.float32)
        q = np.ascontiguousarray(qc, np.float32)
        self._chk(self._L.mkid_set_centers(self._h, _ptr(i), _ptr(q), i.size))

    def set_thresholds(self, thr):
        t = np.ascontiguousarray(thr, np.int32)
        self._chk(self._L.mkid_set_thresholds(self._h, _ptr(t), t.size))

    def set_baseline(self, mode=_lib.BASE_EMA, alpha=41, kf=82, kq=93623, base_thr=8192):
        self._chk(self._L.mkid_set_baseline(self._h, int(mode), int(alpha), int(kf), int(kq),
                                            int(base_thr)))

    def set_rearm(self, frac_q8):
        """Trigger re-arm hysteresis (mkid_set_rearm): re-arm at thr - floor(thr * frac_q8 / 256)."""
        self._chk(self._L.mkid_set_rearm(self._h, int(frac_q8)))

    def reset(self):
        self._chk(self._L.mkid_reset_stream(self._h))

    # ---- data path ---------------------------------------------------------------------------
    def process(self, iq, want_phase=True, cap=None):
        """iq: int16 [S][2] host array. Returns (phase [S/N][C] float32 or None, events uint64)."""
        x = np.ascontiguousarray(iq, np.int16).reshape(-1, 2)
        S = x.shape[0]
        J = S // self.N
        phase = np.empty((J, self.C), np.float32) if want_phase else None
        cap = J * self.C if cap is None else int(cap)
        ev = np.empty(max(cap, 1), np.uint64)
        n = ctypes.c_int64()
        rc = self._L.mkid_process(self._h, _ptr(x), S, _ptr(phase), _ptr(ev), cap, ctypes.byref(n))
        self._chk(rc)
        return phase, ev[:n.value].copy()

    def process_device(self, d_iq, nsamples, d_phase, d_events, cap, d_counts):
        """Device pointers (ints or torch tensors); asynchronous on the context stream."""
        self._chk(self._L.mkid_process_device(self._h, _ptr(d_iq), int(nsamples), _ptr(d_phase),
                                              _ptr(d_events), int(cap), _ptr(d_counts)))

    def trigger_phase_device(self, d_raw, rows, d_events, cap, d_counts):
        """K7 + K8 on device Fix16_13 phase rows [rows][C] (mkid_trigger_phase)."""
        self._chk(self._L.mkid_trigger_phase(self._h, _ptr(d_raw), int(rows), _ptr(d_events), int(cap),
                                             _ptr(d_counts)))

    def trigger_phase(self, raw):
        """Host convenience: raw int16 [rows][C] -> packets (uint64, channel-major)."""
        import torch
        dev = self.torch_device()
        r = np.ascontiguousarray(raw, np.int16).reshape(-1, self.C)
        d_raw = torch.from_numpy(r).to(dev)
        cap = r.shape[0] * self.C // 2 + 64
        d_ev = torch.empty(cap, dtype=torch.int64, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self.trigger_phase_device(d_raw, r.shape[0], d_ev, cap, d_cnt)
        torch.cuda.synchronize(dev)
        n = d_cnt.cpu().numpy()
        if n[0] > n[1]:
            raise _lib.MkidError(_lib.MKID_E_OVERFLOW, 'trigger_phase: packets dropped')
        return d_ev[:int(n[1])].cpu().numpy().view(np.uint64).copy()

    def raw_phase_ptr(self):
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        self._chk(self._L.mkid_last_raw_phase(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def raw_phase(self):
        """Host copy of the last call's Fix16_13 phase rows, int16 [rows][C]."""
        p, rows = self.raw_phase_ptr()
        out = np.empty((rows, self.C), np.int16)
        n = ctypes.c_int64()
        self._chk(self._L.mkid_read_raw_phase(self._h, _ptr(out), rows, ctypes.byref(n)))
        return out

    # ---- thresholds from a quiet phase block (loadThresholds, ROACH_Pulses.py:211-299) ---------
    def phase_thresholds_device(self, d_raw, rows, ld, nch, nsigma, d_thr, d_stats=None):
        """The reference's threshold rule on device Fix16_13 rows d_raw[rows][ld], channels
        0..nch-1, into d_thr int32 [nch] (and d_stats, _lib.ThrStats [nch]); device pointers or
        torch tensors, asynchronous on the context stream (mkid_phase_thresholds)."""
        self._chk(self._L.mkid_phase_thresholds(self._h, _ptr(d_raw), int(rows), int(ld), int(nch),
                                                float(nsigma), _ptr(d_thr), _ptr(d_stats)))

    def phase_thresholds_block_rows(self, rows, ld, nch, aligned16=True):
        """Rows per workgroup row block of phase_thresholds_device for a block of that shape;
        aligned16: whether the block starts on a 16-byte boundary."""
        b = ctypes.c_int64()
        self._chk(self._L.mkid_phase_thresholds_block_rows(self._h, int(rows), int(ld), int(nch),
                                                           1 if aligned16 else 0, ctypes.byref(b)))
        return b.value

    def phase_thresholds_of(self, d_raw, rows, ld, nch, nsigma=2.5):
        """(thr int32 [nch], med float64 [nch]) on the host for channels 0..nch-1 of device rows
        d_raw[rows][ld] (pointer or tensor on this context's GPU): one phase_thresholds_device
        call, one synchronisation and the copy of the 28 nch result bytes."""
        import torch
        dev = self.torch_device()
        d_thr = torch.empty(nch, dtype=torch.int32, device=dev)
        d_st = torch.empty(nch * ctypes.sizeof(_lib.ThrStats), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)      # d_raw may have been written on another stream
        self.phase_thresholds_device(d_raw, rows, ld, nch, nsigma, d_thr, d_st)
        torch.cuda.synchronize(dev)      # the call ran on the context's stream
        st = d_st.cpu().numpy().view(np.dtype([('med', '<f8'), ('p05', '<f8'), ('lo', '<i4'), ('hi', '<i4')]))
        return d_thr.cpu().numpy(), st['med'].copy()

    def phase_thresholds(self, raw=None, nsigma=2.5):
        """(thr int32 [nch], med float64 [nch]) of every channel of a phase block, computed on the
        device: raw int16 [rows][nch] host array (uploaded), or None for the last process call's
        raw phase where it lies (raw_phase_ptr). Bit-identical to
        codecs.thresholds_from_phase_block / threshold_from_phase on the same rows."""
        if raw is None:
            d_raw, rows = self.raw_phase_ptr()
            if rows < 1:
                raise _lib.MkidError(_lib.MKID_E_STATE, 'phase_thresholds: no processed call to take rows from')
            return self.phase_thresholds_of(d_raw, rows, self.C, self.C, nsigma)
        import torch
        r = np.ascontiguousarray(raw, np.int16)
        if r.ndim != 2:
            raise ValueError('raw must be [rows][channels]')
        d_raw = torch.from_numpy(r).to(self.torch_device())
        return self.phase_thresholds_of(d_raw, r.shape[0], r.shape[1], r.shape[1], nsigma)

    def load_thresholds(self, nsigma=2.5):
        """loadThresholds for every channel at once: the thresholds of the last process call's raw
        phase (a quiet stretch of the stream), loaded with set_thresholds. The thresholds cross the
        host once (4 C bytes); the re-arm levels follow them as for any set_thresholds.
        Returns (thr, med)."""
        thr, med = self.phase_thresholds(None, nsigma)
        self.set_thresholds(thr)
        return thr, med

    # ---- phase-noise spectra of a phase block (longsnapshot's noise FFT, ROACH_Pulses.py:521-543) --
    def noise_spectra_device(self, d_raw, rows, ld, nch, n_averages, scale, norm1, d_spec):
        """The reference's phase-noise spectrum of channels 0..nch-1 of device Fix16_13 rows
        d_raw[rows][ld] into d_spec float64 [nch][rows // n_averages]; device pointers or torch
        tensors, asynchronous on the context stream (mkid_phase_noise_spectra)."""
        self._chk(self._L.mkid_phase_noise_spectra(self._h, _ptr(d_raw), int(rows), int(ld), int(nch),
                                                   int(n_averages), float(scale), float(norm1), _ptr(d_spec)))

    def noise_spectra_of(self, d_raw, rows, ld, nch, n_averages=100, norm1=50.0):
        """(np.fft.fftfreq(n), spec float64 [nch][n]) on the host, n = rows // n_averages, for
        channels 0..nch-1 of device rows d_raw[rows][ld] (pointer or tensor on this context's GPU),
        in degrees (scale = codecs.SCALE_TO_ANGLE): one noise_spectra_device call, one
        synchronisation and the copy of the result."""
        import torch
        dev = self.torch_device()
        n = int(rows) // int(n_averages) if n_averages >= 1 else 0
        d_spec = torch.empty((int(nch), max(n, 0)), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)      # d_raw may have been written on another stream
        self.noise_spectra_device(d_raw, rows, ld, nch, n_averages, codecs.SCALE_TO_ANGLE, norm1, d_spec)
        torch.cuda.synchronize(dev)      # the call ran on the context's stream
        return np.fft.fftfreq(n), d_spec.cpu().numpy()

    def noise_spectra(self, raw=None, n_averages=100, norm1=50.0):
        """(np.fft.fftfreq(n), spec float64 [nch][n]) of every channel of a phase block, computed on
        the device: raw int16 [rows][nch] host array (uploaded), or None for the last process call's
        raw phase where it lies (raw_phase_ptr). codecs.noise_spectrum(raw[:, c] * SCALE_TO_ANGLE,
        n_averages, norm1) channel by channel, in float32 arithmetic."""
        if raw is None:
            d_raw, rows = self.raw_phase_ptr()
            if rows < 1:
                raise _lib.MkidError(_lib.MKID_E_STATE, 'noise_spectra: no processed call to take rows from')
            return self.noise_spectra_of(d_raw, rows, self.C, self.C, n_averages, norm1)
        import torch
        r = np.ascontiguousarray(raw, np.int16)
        if r.ndim != 2:
            raise ValueError('raw must be [rows][channels]')
        d_raw = torch.from_numpy(r).to(self.torch_device())
        return self.noise_spectra_of(d_raw, r.shape[0], r.shape[1], r.shape[1], n_averages, norm1)

    def set_iq_tap(self, channel):
        """Record channel's low-pass output (IQ snapshot source); channel < 0 turns it off."""
        self._chk(self._L.mkid_set_iq_tap(self._h, int(channel)))

    def iq_tap(self):
        """int16 [rows][2] I/Q of the tapped channel for the rows of the last process call."""
        n = ctypes.c_int64()
        self._chk(self._L.mkid_read_iq_tap(self._h, None, 0, ctypes.byref(n)))
        out = np.empty((n.value, 2), np.int16)
        self._chk(self._L.mkid_read_iq_tap(self._h, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def trigger_reruns(self):
        n = ctypes.c_int64()
        self._chk(self._L.mkid_trigger_reruns(self._h, ctypes.byref(n)))
        return n.value

    def set_accumulator(self, on):
        """startAccumulator (ROACH_Setup.py:654-659): True arms the avgIQ accumulator (the sums
        restart; every following process call adds its rows), False stops it (sums kept)."""
        self._chk(self._L.mkid_set_accumulator(self._h, 1 if on else 0))

    def avg_iq(self):
        """Per-channel mean low-pass I/Q over the rows accumulated since set_accumulator(True)."""
        mi = np.empty(self.C, np.float32)
        mq = np.empty(self.C, np.float32)
        self._chk(self._L.mkid_avg_iq(self._h, _ptr(mi), _ptr(mq)))
        return mi, mq

    # ---- host-replay triggers --------------------------------------------
    def replay_trigger(self, d_raw, n, ld, nch, mode, length, start, need, skip, threshold_deg,
                       wrap_negative=False, d_hits=None, cap=64, d_counts=None):
        """Run the reference's rolling-/block-mean replay trigger on device Fix16_13 phase
        d_raw[n][ld] (int16 device tensor or pointer), channels 0..nch-1. Returns the device
        (hits [nch, cap] int32, counts [nch] int32) tensors (allocated when not given)."""
        import torch
        if d_hits is None:
            d_hits = torch.full((nch, cap), -1, dtype=torch.int32, device=self.torch_device())
        if d_counts is None:
            d_counts = torch.zeros(nch, dtype=torch.int32, device=self.torch_device())
        rc = _lib.ReplayCfg(int(mode), int(length), int(start), int(need), int(skip),
                            1 if wrap_negative else 0, float(threshold_deg))
        self._chk(self._L.mkid_replay_trigger(self._h, _ptr(d_raw), int(n), int(ld), int(nch),
                                              ctypes.byref(rc), _ptr(d_hits), int(cap), _ptr(d_counts)))
        return d_hits, d_counts

    # ---- per-packet optimal-filter pulse height (BASELINE config 5) -----------------------------
    def set_pulse_filter(self, coeff, pre):
        """coeff: float [C][ncoeff] (one filter per channel, e.g. template.optimal_filter's weights
        tiled); the height of a packet stamped ts is sum_i coeff[ch][i] phase[ts - pre + i][ch]."""
        cf = np.ascontiguousarray(coeff, np.float32).reshape(self.C, -1)
        self._chk(self._L.mkid_set_pulse_filter(self._h, _ptr(cf), cf.shape[0], cf.shape[1], int(pre)))
        self.pulse_filter = (int(cf.shape[1]), int(pre))   # (ncoeff, pre), for observe.Observation

    def pulse_heights_device(self, d_phase, rows, j0, d_events, n, d_heights):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h)."""
        self._chk(self._L.mkid_pulse_heights(self._h, _ptr(d_phase), int(rows), int(j0), _ptr(d_events),
                                             int(n), _ptr(d_heights)))

    def pulse_heights_counted(self, d_phase, rows, j0, d_events, d_count, cap, d_heights):
        """As pulse_heights_device with the packet count read on the device (d_count: an int64
        device pointer/tensor, e.g. the d_counts[1:] of the process call)."""
        self._chk(self._L.mkid_pulse_heights_counted(self._h, _ptr(d_phase), int(rows), int(j0), _ptr(d_events),
                                                     _ptr(d_count), int(cap), _ptr(d_heights)))

    def pulse_heights(self, phase, events, j0=0):
        """Host convenience: phase float32 [rows][C] (rad) of global rows j0.., events uint64 [n]
        -> float32 heights [n] (NaN where the window leaves the rows)."""
        import torch
        dev = self.torch_device()
        ph = torch.from_numpy(np.ascontiguousarray(phase, np.float32)).to(dev)
        ev = torch.from_numpy(np.ascontiguousarray(events, np.uint64).view(np.int64)).to(dev)
        out = torch.empty(ev.numel(), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)  # the uploads run on torch's stream, the kernel on the context's
        self.pulse_heights_device(ph, ph.shape[0], j0, ev, ev.numel(), out)
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()

    # ---- pulse height with a lag search and a sub-sample arrival time (mkid_pulse_fit) -------------
    def set_pulse_filter_device(self, d_coeff, pre, ncoeff=None):
        """set_pulse_filter from a device table float32 [C][ncoeff], e.g. the coeff tensor of
        template.bank_filters: a device-to-device copy, nothing passes through the host. ncoeff
        defaults to the tensor's row length (give it with a raw pointer)."""
        if hasattr(d_coeff, 'data_ptr'):
            import torch
            if d_coeff.dtype != torch.float32 or not d_coeff.is_contiguous() or d_coeff.numel() % self.C:
                raise ValueError('d_coeff must be contiguous float32 [C][ncoeff]')
            if ncoeff is None:
                ncoeff = d_coeff.numel() // self.C
            torch.cuda.synchronize(self.torch_device())   # the table may have been written on another stream
        if ncoeff is None:
            raise ValueError('ncoeff is needed with a raw pointer')
        self._chk(self._L.mkid_set_pulse_filter_device(self._h, _ptr(d_coeff), self.C, int(ncoeff), int(pre)))
        self.pulse_filter = (int(ncoeff), int(pre))

    def set_pulse_fit(self, search=3, polarity=-1):
        """Search half-width L (0..31 rows around the stamp) and polarity of pulse_fit. The lag that
        maximises polarity * H is chosen. The default -1 follows template.matched_fir_taps' sign
        convention: phase pulses are negative-going at the trigger and the filters of
        template.optimal_filter / bank_filters respond positively to the (sign-flipped, positive)
        template, so a photon gives a negative H and the fit looks for its minimum. Either order
        with set_pulse_filter; forgets the fit's carried rows."""
        self._chk(self._L.mkid_set_pulse_fit(self._h, int(search), int(polarity)))
        self.pulse_fit_search = int(search)

    def pulse_fit_device(self, d_phase, rows, j0, d_events, n, d_heights, d_dt=None, d_lag=None, d_h0=None):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h mkid_pulse_fit).
        d_dt, d_lag and d_h0 may be None."""
        self._chk(self._L.mkid_pulse_fit(self._h, _ptr(d_phase), int(rows), int(j0), _ptr(d_events), int(n),
                                         _ptr(d_heights), _ptr(d_dt), _ptr(d_lag), _ptr(d_h0)))

    def pulse_fit_counted(self, d_phase, rows, j0, d_events, d_count, cap, d_heights, d_dt=None, d_lag=None,
                          d_h0=None):
        """As pulse_fit_device with the packet count read on the device (d_count: an int64 device
        pointer/tensor, e.g. the d_counts[1:] of the process call)."""
        self._chk(self._L.mkid_pulse_fit_counted(self._h, _ptr(d_phase), int(rows), int(j0), _ptr(d_events),
                                                 _ptr(d_count), int(cap), _ptr(d_heights), _ptr(d_dt), _ptr(d_lag),
                                                 _ptr(d_h0)))

    def pulse_fit(self, phase, events, j0=0):
        """Host convenience: phase float32 [rows][C] (rad) of global rows j0.., events uint64 [n] ->
        (heights float32 [n], dt float32 [n], lag int32 [n], h0 float32 [n]); NaN / INT32_MIN where
        the search window leaves the rows. The arrival of a packet is its unwrapped stamp + dt."""
        import torch
        dev = self.torch_device()
        ph = torch.from_numpy(np.ascontiguousarray(phase, np.float32).reshape(-1, self.C)).to(dev)
        ev = torch.from_numpy(np.ascontiguousarray(events, np.uint64).view(np.int64)).to(dev)
        n = ev.numel()
        h, dt, h0 = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        lag = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # the uploads run on torch's stream, the kernel on the context's
        self.pulse_fit_device(ph, ph.shape[0], j0, ev, n, h, dt, lag, h0)
        torch.cuda.synchronize(dev)
        return h.cpu().numpy(), dt.cpu().numpy(), lag.cpu().numpy(), h0.cpu().numpy()

    # ---- count image and pulse-height spectra (mkid_count_photons, mkid_height_spectra) -----------
    def count_photons_device(self, d_events, n, j0, n_seconds, d_image, d_outside):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h mkid_count_photons):
        d_image int32 [n_seconds][C] and d_outside int64 [2] are added to."""
        self._chk(self._L.mkid_count_photons(self._h, _ptr(d_events), int(n), int(j0), int(n_seconds),
                                             _ptr(d_image), _ptr(d_outside)))

    def count_photons_counted(self, d_events, d_count, cap, j0, n_seconds, d_image, d_outside):
        """As count_photons_device with the packet count read on the device."""
        self._chk(self._L.mkid_count_photons_counted(self._h, _ptr(d_events), _ptr(d_count), int(cap), int(j0),
                                                     int(n_seconds), _ptr(d_image), _ptr(d_outside)))

    def list_photons_device(self, d_events, n, j0, n_seconds, K, layout, d_image, d_outside, d_words, d_stamps,
                            d_dropped):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h mkid_list_photons):
        d_image and d_outside are added to as by count_photons_device, and the packets go to their
        cells' rows of d_words uint64 / d_stamps int64 [n_seconds][C][K]; d_dropped int64 [1] counts
        the packets past slot K - 1."""
        self._chk(self._L.mkid_list_photons(self._h, _ptr(d_events), int(n), int(j0), int(n_seconds), int(K),
                                            int(layout), _ptr(d_image), _ptr(d_outside), _ptr(d_words),
                                            _ptr(d_stamps), _ptr(d_dropped)))

    def list_photons_counted(self, d_events, d_count, cap, j0, n_seconds, K, layout, d_image, d_outside, d_words,
                             d_stamps, d_dropped):
        """As list_photons_device with the packet count read on the device."""
        self._chk(self._L.mkid_list_photons_counted(self._h, _ptr(d_events), _ptr(d_count), int(cap), int(j0),
                                                    int(n_seconds), int(K), int(layout), _ptr(d_image),
                                                    _ptr(d_outside), _ptr(d_words), _ptr(d_stamps), _ptr(d_dropped)))

    def fill_photon_heights_device(self, d_events, d_heights, d_dt, n, j0, j_defer, n_seconds, K, d_image, d_stamps,
                                   d_row_height, d_row_dt, d_fill):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h
        mkid_fill_photon_heights): the heights (and d_dt, nullable) of the packets that are not
        deferred go to their slots of d_row_height (d_row_dt, nullable) float32 [n_seconds][C][K];
        d_fill int64 [2] counts those found and those not."""
        self._chk(self._L.mkid_fill_photon_heights(self._h, _ptr(d_events), _ptr(d_heights), _ptr(d_dt), int(n),
                                                   int(j0), int(j_defer), int(n_seconds), int(K), _ptr(d_image),
                                                   _ptr(d_stamps), _ptr(d_row_height), _ptr(d_row_dt), _ptr(d_fill)))

    def fill_photon_heights_counted(self, d_events, d_heights, d_dt, d_count, cap, j0, j_defer, n_seconds, K, d_image,
                                    d_stamps, d_row_height, d_row_dt, d_fill):
        """As fill_photon_heights_device with the packet count read on the device."""
        self._chk(self._L.mkid_fill_photon_heights_counted(self._h, _ptr(d_events), _ptr(d_heights), _ptr(d_dt),
                                                           _ptr(d_count), int(cap), int(j0), int(j_defer),
                                                           int(n_seconds), int(K), _ptr(d_image), _ptr(d_stamps),
                                                           _ptr(d_row_height), _ptr(d_row_dt), _ptr(d_fill)))

    # ---- the ring of second slots (mkid_list_photons_ring .. mkid_clear_second) ------------------
    def list_photons_ring_device(self, d_events, n, j0, sec0, n_slots, sec_end, K, layout, d_image, d_outside, d_words,
                                 d_stamps, d_dropped):
        """As list_photons_device into tables [n_slots][C][K]: second sec goes to slot sec mod n_slots
        while sec0 <= sec < min(sec0 + n_slots, sec_end); d_outside is int64 [4] (include/mkidgpu.h
        mkid_list_photons_ring)."""
        self._chk(self._L.mkid_list_photons_ring(self._h, _ptr(d_events), int(n), int(j0), int(sec0), int(n_slots),
                                                 int(sec_end), int(K), int(layout), _ptr(d_image), _ptr(d_outside),
                                                 _ptr(d_words), _ptr(d_stamps), _ptr(d_dropped)))

    def list_photons_ring_counted(self, d_events, d_count, cap, j0, sec0, n_slots, sec_end, K, layout, d_image,
                                  d_outside, d_words, d_stamps, d_dropped):
        """As list_photons_ring_device with the packet count read on the device."""
        self._chk(self._L.mkid_list_photons_ring_counted(self._h, _ptr(d_events), _ptr(d_count), int(cap), int(j0),
                                                         int(sec0), int(n_slots), int(sec_end), int(K), int(layout),
                                                         _ptr(d_image), _ptr(d_outside), _ptr(d_words), _ptr(d_stamps),
                                                         _ptr(d_dropped)))

    def fill_photon_heights_ring_device(self, d_events, d_heights, d_dt, n, j0, j_defer, sec0, n_slots, sec_end, K,
                                        d_image, d_stamps, d_row_height, d_row_dt, d_fill):
        """As fill_photon_heights_device into the ring's tables (include/mkidgpu.h
        mkid_fill_photon_heights_ring)."""
        self._chk(self._L.mkid_fill_photon_heights_ring(self._h, _ptr(d_events), _ptr(d_heights), _ptr(d_dt), int(n),
                                                        int(j0), int(j_defer), int(sec0), int(n_slots), int(sec_end),
                                                        int(K), _ptr(d_image), _ptr(d_stamps), _ptr(d_row_height),
                                                        _ptr(d_row_dt), _ptr(d_fill)))

    def fill_photon_heights_ring_counted(self, d_events, d_heights, d_dt, d_count, cap, j0, j_defer, sec0, n_slots,
                                         sec_end, K, d_image, d_stamps, d_row_height, d_row_dt, d_fill):
        """As fill_photon_heights_ring_device with the packet count read on the device."""
        self._chk(self._L.mkid_fill_photon_heights_ring_counted(self._h, _ptr(d_events), _ptr(d_heights), _ptr(d_dt),
                                                                _ptr(d_count), int(cap), int(j0), int(j_defer),
                                                                int(sec0), int(n_slots), int(sec_end), int(K),
                                                                _ptr(d_image), _ptr(d_stamps), _ptr(d_row_height),
                                                                _ptr(d_row_dt), _ptr(d_fill)))

    def pack_second(self, sec, n_slots, K, d_image, d_words, d_stamps, d_row_height, d_row_dt, cap_out, d_counts,
                    d_offsets, d_out_words, d_out_stamps, d_out_height, d_out_dt, d_total):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h mkid_pack_second):
        slot sec mod n_slots of the tables as d_counts int32 [C], d_offsets int64 [C + 1], the rows'
        photons end to end in the four outputs (cut at cap_out) and d_total int64 [2]."""
        self._chk(self._L.mkid_pack_second(self._h, int(sec), int(n_slots), int(K), _ptr(d_image), _ptr(d_words),
                                           _ptr(d_stamps), _ptr(d_row_height), _ptr(d_row_dt), int(cap_out),
                                           _ptr(d_counts), _ptr(d_offsets), _ptr(d_out_words), _ptr(d_out_stamps),
                                           _ptr(d_out_height), _ptr(d_out_dt), _ptr(d_total)))

    def clear_second(self, sec, n_slots, K, d_image, d_row_height, d_row_dt):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h mkid_clear_second):
        the filled heights (and dt) of slot sec mod n_slots back to NaN and its image row to 0."""
        self._chk(self._L.mkid_clear_second(self._h, int(sec), int(n_slots), int(K), _ptr(d_image),
                                            _ptr(d_row_height), _ptr(d_row_dt)))

    def height_spectra_device(self, d_events, d_heights, n, j0, j_defer, d_lo, d_inv, nbins, d_spectra,
                              d_deferred=None, cap_def=0, d_ndef=None):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h mkid_height_spectra):
        d_spectra int32 [C][nbins + 3] is added to; with d_deferred, the packets that still wait for
        their height are appended there and counted in d_ndef int64 [2]."""
        self._chk(self._L.mkid_height_spectra(self._h, _ptr(d_events), _ptr(d_heights), int(n), int(j0), int(j_defer),
                                              _ptr(d_lo), _ptr(d_inv), int(nbins), _ptr(d_spectra), _ptr(d_deferred),
                                              int(cap_def), _ptr(d_ndef)))

    def height_spectra_counted(self, d_events, d_heights, d_count, cap, j0, j_defer, d_lo, d_inv, nbins, d_spectra,
                               d_deferred=None, cap_def=0, d_ndef=None):
        """As height_spectra_device with the packet count read on the device."""
        self._chk(self._L.mkid_height_spectra_counted(self._h, _ptr(d_events), _ptr(d_heights), _ptr(d_count), int(cap),
                                                      int(j0), int(j_defer), _ptr(d_lo), _ptr(d_inv), int(nbins),
                                                      _ptr(d_spectra), _ptr(d_deferred), int(cap_def), _ptr(d_ndef)))

    # ---- laser lines, the energy calibration and the energy cube (include/mkidgpu.h) ---------------
    def spectrum_lines_device(self, d_spectra, d_lo, d_step, nch, nbins, energies, smooth, min_sep, min_peak,
                              fit_half, d_lines, d_cal, d_cal_f):
        """Device pointers; asynchronous on the context stream (mkid_spectrum_lines): the laser lines
        of channels 0..nch-1 of d_spectra int32 [nch][nbins + 3] into d_lines (_lib.LineFit [nch][P]),
        d_cal (_lib.EnergyCal [nch]) and d_cal_f float32 [nch][4]; energies: P host values in eV."""
        e = np.ascontiguousarray(energies, np.float64).ravel()
        self._chk(self._L.mkid_spectrum_lines(self._h, _ptr(d_spectra), _ptr(d_lo), _ptr(d_step), int(nch), int(nbins),
                                              int(e.size), _ptr(e), int(smooth), int(min_sep), int(min_peak),
                                              int(fit_half), _ptr(d_lines), _ptr(d_cal), _ptr(d_cal_f)))

    def energy_cube_device(self, d_events, d_heights, n, j0, j_defer, d_cal_f, mode, hc, vlo, vinv, nb, d_cube,
                           d_energy=None):
        """Device pointers; asynchronous on the context stream (mkid_energy_cube): d_cube int32
        [C][nb + 3] is added to, d_energy float32 [n] (optional) takes every pixel packet's energy."""
        self._chk(self._L.mkid_energy_cube(self._h, _ptr(d_events), _ptr(d_heights), int(n), int(j0), int(j_defer),
                                           _ptr(d_cal_f), int(mode), float(hc), float(vlo), float(vinv), int(nb),
                                           _ptr(d_cube), _ptr(d_energy)))

    def energy_cube_counted(self, d_events, d_heights, d_count, cap, j0, j_defer, d_cal_f, mode, hc, vlo, vinv, nb,
                            d_cube, d_energy=None):
        """As energy_cube_device with the packet count read on the device."""
        self._chk(self._L.mkid_energy_cube_counted(self._h, _ptr(d_events), _ptr(d_heights), _ptr(d_count), int(cap),
                                                   int(j0), int(j_defer), _ptr(d_cal_f), int(mode), float(hc),
                                                   float(vlo), float(vinv), int(nb), _ptr(d_cube), _ptr(d_energy)))

    # ---- resonator loop fits (include/mkidgpu.h mkid_fit_loops) --------------------------------------
    def fit_loops_device(self, d_freq, d_i, d_q, d_isd, d_qsd, d_draws, d_qguess, nch, fsteps, n_starts, max_iter,
                         ftol, d_fits, d_chisq_all=None):
        """Device pointers; asynchronous on the context stream (mkid_fit_loops): float64 d_freq, d_i,
        d_q [nch][fsteps], d_isd, d_qsd (both or None), d_draws [nch][S][5], d_qguess [nch] or None,
        into d_fits (_lib.LoopFit [nch]) and d_chisq_all float64 [nch][S] (optional)."""
        self._chk(self._L.mkid_fit_loops(self._h, _ptr(d_freq), _ptr(d_i), _ptr(d_q), _ptr(d_isd), _ptr(d_qsd),
                                         _ptr(d_draws), _ptr(d_qguess), int(nch), int(fsteps), int(n_starts),
                                         int(max_iter), float(ftol), _ptr(d_fits), _ptr(d_chisq_all)))

    def fit_loops(self, freq, I, Q, draws, **kw):
        """Host convenience: loopfit.fit_loops on this context -> dict of arrays by field."""
        from . import loopfit
        return loopfit.fit_loops(self, freq, I, Q, draws, **kw)

    # ---- resonator magnitude fits (include/mkidgpu.h mkid_fit_mags) -----------------------------------
    def fit_mags_device(self, d_freq, d_i, d_q, d_draws, nch, fsteps, n_starts, max_iter, ftol, d_fits, d_qout=None,
                        d_chisq_all=None):
        """Device pointers; asynchronous on the context stream (mkid_fit_mags): float64 d_freq, d_i,
        d_q [nch][fsteps], d_draws [nch][S], into d_fits (_lib.MagFit [nch]), d_qout float64 [nch]
        (optional; a valid d_qguess of fit_loops_device) and d_chisq_all float64 [nch][S] (optional)."""
        self._chk(self._L.mkid_fit_mags(self._h, _ptr(d_freq), _ptr(d_i), _ptr(d_q), _ptr(d_draws), int(nch),
                                        int(fsteps), int(n_starts), int(max_iter), float(ftol), _ptr(d_fits),
                                        _ptr(d_qout), _ptr(d_chisq_all)))

    def fit_mags(self, freq, I, Q, draws, **kw):
        """Host convenience: loopfit.fit_mags on this context -> dict of arrays by field."""
        from . import loopfit
        return loopfit.fit_mags(self, freq, I, Q, draws, **kw)

    # ---- Welch spectra and the IQ noise analysis (include/mkidgpu.h mkid_welch_psd, mkid_iq_noise) ------
    def welch_psd_device(self, d_a, d_b, n, ld, nch, nfft, fs, group, d_pa, d_pb=None):
        """Device pointers; asynchronous on the context stream (mkid_welch_psd): float64 d_a, d_b
        (nullable) [nch][ld] -> d_pa, d_pb (nullable) [nch][nfft/2+1]."""
        self._chk(self._L.mkid_welch_psd(self._h, _ptr(d_a), _ptr(d_b), int(n), int(ld), int(nch), int(nfft),
                                         float(fs), int(group), _ptr(d_pa), _ptr(d_pb)))

    def iq_noise_device(self, d_i, d_q, n, ld, nch, d_i0, d_q0, d_icen, d_qcen, d_qfit, cfg, d_pn, d_an, d_result):
        """Device pointers; asynchronous on the context stream (mkid_iq_noise): int16 d_i, d_q
        [nch][ld], float64 offsets, centres and Q [nch], cfg an _lib.IqNoiseCfg -> d_pn, d_an
        [nch][nout], d_result [nch] mkid_iqnoise_result."""
        self._chk(self._L.mkid_iq_noise(self._h, _ptr(d_i), _ptr(d_q), int(n), int(ld), int(nch), _ptr(d_i0),
                                        _ptr(d_q0), _ptr(d_icen), _ptr(d_qcen), _ptr(d_qfit),
                                        None if cfg is None else ctypes.byref(cfg), _ptr(d_pn), _ptr(d_an),
                                        _ptr(d_result)))

    def analyze_noise(self, I, Q, fits, **kw):
        """Host convenience: iqnoise.analyze_noise on this context -> dict of arrays by field."""
        from . import iqnoise
        return iqnoise.analyze_noise(self, I, Q, fits, **kw)

    def concat_packets(self, d_a, d_na, cap_a, d_b, d_nb, cap_b, d_out, cap_out, d_nout):
        """d_out = the first min(*d_na, cap_a) packets of d_a, then the first min(*d_nb, cap_b) of d_b,
        cut at cap_out; d_nout int64 [2] = {produced, written}. Both counts are read on the device."""
        self._chk(self._L.mkid_concat_packets(self._h, _ptr(d_a), _ptr(d_na), int(cap_a), _ptr(d_b), _ptr(d_nb),
                                              int(cap_b), _ptr(d_out), int(cap_out), _ptr(d_nout)))

    def count_photons(self, events, j0, n_seconds):
        """Host convenience: events uint64 [n] of the call whose first global row is j0 ->
        (image int32 [n_seconds][C], outside int64 [2])."""
        import torch
        dev = self.torch_device()
        ev = torch.from_numpy(np.ascontiguousarray(events, np.uint64).view(np.int64)).to(dev)
        image = torch.zeros((int(n_seconds), self.C), dtype=torch.int32, device=dev)
        outside = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)  # the uploads run on torch's stream, the kernel on the context's
        self.count_photons_device(ev if ev.numel() else None, ev.numel(), j0, n_seconds, image, outside)
        torch.cuda.synchronize(dev)
        return image.cpu().numpy(), outside.cpu().numpy()

    def height_spectra(self, events, heights, lo, step, nbins, j0=0, j_defer=None, cap_def=0):
        """Host convenience: events uint64 [n] and their heights float32 [n]; lo and step scalars or
        [C] (bin b of channel c is [lo[c] + b step[c], lo[c] + (b + 1) step[c]) up to fp32 rounding;
        the rule is include/mkidgpu.h's, with inv = float32(1) / float32(step)) -> spectra int32
        [C][nbins + 3]. With j_defer also (deferred uint64 [written], ndef int64 [2])."""
        import torch
        dev = self.torch_device()
        ev = torch.from_numpy(np.ascontiguousarray(events, np.uint64).view(np.int64)).to(dev)
        h = torch.from_numpy(np.ascontiguousarray(heights, np.float32)).to(dev)
        lo32 = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (self.C,)))
        with np.errstate(divide='ignore', invalid='ignore'):
            inv32 = np.ascontiguousarray(np.broadcast_to(np.float32(1) / np.asarray(step, np.float32), (self.C,)))
        d_lo, d_inv = torch.from_numpy(lo32).to(dev), torch.from_numpy(inv32).to(dev)
        spectra = torch.zeros((self.C, int(nbins) + 3), dtype=torch.int32, device=dev)
        defer = j_defer is not None
        d_def = torch.zeros(max(int(cap_def), 1), dtype=torch.int64, device=dev) if defer else None
        d_ndef = torch.zeros(2, dtype=torch.int64, device=dev) if defer else None
        torch.cuda.synchronize(dev)  # the uploads run on torch's stream, the kernels on the context's
        n = ev.numel()
        self.height_spectra_device(ev if n else None, h if n else None, n, j0, j_defer if defer else 0, d_lo, d_inv,
                                   nbins, spectra, d_def, cap_def, d_ndef)
        torch.cuda.synchronize(dev)
        if not defer:
            return spectra.cpu().numpy()
        ndef = d_ndef.cpu().numpy()
        return spectra.cpu().numpy(), d_def[:int(ndef[1])].cpu().numpy().view(np.uint64), ndef

    # ---- pulse capture: phase windows around the packets, into a per-channel record bank -----------
    def set_capture(self, length=2000, pre=1000, max_per_ch=256):
        """Records of `length` phase rows starting `pre` rows before each packet's stamp, at most
        `max_per_ch` per channel (mkid_set_capture; the defaults are the reference's
        [bob-500, bob+1500) RawPulse length, centred). Starts a new stream segment."""
        self._chk(self._L.mkid_set_capture(self._h, int(length), int(pre), int(max_per_ch)))
        self._capture = (int(length), int(pre), int(max_per_ch))

    def capture_bank(self):
        """A fresh bank on this context's GPU: (records [C][R][L] float32, stamps [C][R] int64,
        info [C][2] int32 {ready, dropped}, zeroed)."""
        import torch
        if getattr(self, '_capture', None) is None:
            raise _lib.MkidError(_lib.MKID_E_STATE, 'capture_bank: set_capture first')
        L, _, R = self._capture
        dev = self.torch_device()
        return (torch.zeros((self.C, R, L), dtype=torch.float32, device=dev),
                torch.zeros((self.C, R), dtype=torch.int64, device=dev),
                torch.zeros((self.C, 2), dtype=torch.int32, device=dev))

    def capture_pulses_device(self, d_phase, rows, j0, d_events, n, d_records, d_stamps, d_info):
        """Device pointers; asynchronous on the context stream (include/mkidgpu.h)."""
        self._chk(self._L.mkid_capture_pulses(self._h, _ptr(d_phase), int(rows), int(j0), _ptr(d_events), int(n),
                                              _ptr(d_records), _ptr(d_stamps), _ptr(d_info)))

    def capture_pulses_counted(self, d_phase, rows, j0, d_events, d_count, cap, d_records, d_stamps, d_info):
        """As capture_pulses_device with the packet count read on the device (d_count: an int64
        device pointer/tensor, e.g. the d_counts[1:] of the process call)."""
        self._chk(self._L.mkid_capture_pulses_counted(self._h, _ptr(d_phase), int(rows), int(j0), _ptr(d_events),
                                                      _ptr(d_count), int(cap), _ptr(d_records), _ptr(d_stamps),
                                                      _ptr(d_info)))

    def capture_pulses(self, phase, events, j0=0, bank=None):
        """Host convenience: phase float32 [rows][C] (rad) of global rows j0.., events uint64 [n]
        (channel-major, time-ascending) -> the bank (device tensors; a new one when not given)."""
        import torch
        dev = self.torch_device()
        ph = torch.from_numpy(np.ascontiguousarray(phase, np.float32).reshape(-1, self.C)).to(dev)
        ev = torch.from_numpy(np.ascontiguousarray(events, np.uint64).view(np.int64)).to(dev)
        if bank is None:
            bank = self.capture_bank()
        torch.cuda.synchronize(dev)  # the uploads run on torch's stream, the kernels on the context's
        self.capture_pulses_device(ph, ph.shape[0], j0, ev, ev.numel(), *bank)
        torch.cuda.synchronize(dev)
        return bank

    # ---- timing ------------------------------------------------------------------------------
    def set_timing(self, on, kernels=None):
        """on: time every kernel (HIP events); kernels: names (e.g. ['k_front']) to time only
        those (mkid_set_timing with MKID_TIMING_ONLY masks; each timed launch costs two event
        records on the stream)."""
        if on and kernels:
            names = [self._L.mkid_kernel_name(k).decode() for k in range(_lib.K_COUNT)]
            mask = 0
            for n in kernels:
                if n not in names:
                    raise ValueError('unknown kernel %r (one of %s)' % (n, names))
                mask |= 1 << names.index(n)
            self._chk(self._L.mkid_set_timing_mask(self._h, mask))
        else:
            self._chk(self._L.mkid_set_timing(self._h, 1 if on else 0))

    def timing(self):
        out = {}
        for k in range(_lib.K_COUNT):
            ms = ctypes.c_double()
            n = ctypes.c_int64()
            self._chk(self._L.mkid_get_timing(self._h, k, ctypes.byref(ms), ctypes.byref(n)))
            out[self._L.mkid_kernel_name(k).decode()] = (ms.value, n.value)
        return out

    def stream_copy(self, d_dst, d_src, nbytes):
        """Diagnostic HBM copy (mkid_stream_copy), asynchronous on the context stream."""
        self._chk(self._L.mkid_stream_copy(self._h, _ptr(d_dst), _ptr(d_src), int(nbytes)))

    # ---- synthetic source (tests / bench only) -------------------------------------------------
    def synth_adc(self, d_out, nsamples, n0, d_base, d_tones, d_pulses, npulses, tau_rise,
                  tau_fall, window, sigma, seed):
        self._chk(self._L.mkid_synth_adc(self._h, _ptr(d_out), int(nsamples), int(n0),
                                         _ptr(d_base), _ptr(d_tones), _ptr(d_pulses),
                                         int(npulses), float(tau_rise), float(tau_fall),
                                         int(window), float(sigma), int(seed) & 0xffffffff))


def pack_reference(wide):
    """Wide device packets -> reference 64-bit packets (mkid_pack_reference, C <= 254)."""
    L = _lib.load()
    w = np.ascontiguousarray(wide, np.uint64)
    out = np.empty_like(w)
    _lib.check(L.mkid_pack_reference(_ptr(w), w.size, _ptr(out)))
    return out
