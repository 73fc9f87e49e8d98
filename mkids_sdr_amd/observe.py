"""The observing products of a streamed run, kept on the device: the per-second count image
(PacketMaster's photon_counts[sec][pixel], PacketMaster.c:371-381) and the per-channel pulse-height
spectra, for every channel at once and across calls, with the heights' deferral protocol
(include/mkidgpu.h mkid_pulse_heights: the packets of a call's last rows get their height with the
next call) run on the device too. A step enqueues five calls on the context's stream and makes no
device-to-host copy and no synchronisation. With photon_rows=K it also keeps the product itself:
PacketMaster's per-pixel, per-second photon rows (/r#/p#/t<obs>, PacketMaster.c:978-1050), K slots a
row, each photon with its height (and arrival offset) once the deferral protocol has settled it
(include/mkidgpu.h mkid_list_photons, mkid_fill_photon_heights): six calls a step, still no
synchronisation.
"""
import numpy as np

from . import _lib, packets


def j_defer(j0, rows, ncoeff, pre, search=0):
    """The first stamp whose search window passes the last row of the call that covers global rows
    j0 .. j0 + rows - 1: a window is inside while (jg - j0 - pre) + search + ncoeff <= rows
    (csrc/fit_common.h inside; search = 0 for the plain heights)."""
    return int(j0) + int(rows) + int(pre) - int(ncoeff) - int(search) + 1


class Observation:
    """Count image, spectra and deferred lists of one observation on the GPU of `chan` (a
    Channelizer with its pulse filter set, and set_pulse_fit when fit=True).

    n_seconds   seconds of the image (PacketMaster's exptime)
    nbins       bins per spectrum; lo, step: scalars or [C], bin b of channel c starts at
                lo[c] + b step[c] (the rule, with inv = float32(1) / float32(step), is
                include/mkidgpu.h mkid_height_spectra); columns 0, nbins + 1, nbins + 2 are under, over
                and "no height"
    cap         capacity of the packet list given to step()
    cap_deferred  capacity of the deferred lists: at least the packets of a call's last
                ncoeff - pre + search rows
    debug       keep a host copy of every step's joined list and heights (synchronises each step)
    photon_rows  None: no photon rows, and the calls of a step are exactly those above. K: rows of K
                slots per pixel and second (PacketMaster keeps 2499), [n_seconds][C][K] words, stamps,
                heights and arrival offsets on the device, the last two NaN until filled (the
                offsets stay NaN without fit)
    row_layout  _lib.ROW_WIDE (any C) or _lib.ROW_REFERENCE (packets.encode_wire's word, C <= 254)
    """

    def __init__(self, chan, n_seconds, nbins, lo, step, cap, cap_deferred, fit=False, debug=False,
                 photon_rows=None, row_layout=_lib.ROW_WIDE):
        import torch
        if chan.pulse_filter is None:
            raise ValueError('Observation: set the pulse filter first')
        if fit and chan.pulse_fit_search is None:
            raise ValueError('Observation(fit=True): set_pulse_fit first')
        self.chan, self.fit, self.debug = chan, bool(fit), bool(debug)
        self.n_seconds, self.nbins = int(n_seconds), int(nbins)
        self.cap, self.cap_def = int(cap), int(cap_deferred)
        C, dev = chan.C, chan.torch_device()
        self.lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float32), (C,)))
        self.step_width = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (C,)))
        with np.errstate(divide='ignore', invalid='ignore'):
            self.inv = np.float32(1) / self.step_width
        self.d_lo, self.d_inv = torch.from_numpy(self.lo).to(dev), torch.from_numpy(self.inv).to(dev)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.d_image = z((self.n_seconds, C), torch.int32)
        self.d_spectra = z((C, self.nbins + 3), torch.int32)
        self.d_outside = z(2, torch.int64)
        self.d_def = [z(max(self.cap_def, 1), torch.int64) for _ in range(2)]
        self.d_ndef = [z(2, torch.int64) for _ in range(2)]
        self.d_zero = z(2, torch.int64)
        self.cap_join = self.cap + self.cap_def
        self.d_join = z(max(self.cap_join, 1), torch.int64)
        self.d_njoin = z(2, torch.int64)
        self.d_heights = z(max(self.cap_join, 1), torch.float32)
        self.K, self.row_layout = (None if photon_rows is None else int(photon_rows)), int(row_layout)
        if self.K is not None:
            if not 1 <= self.K <= 65536:
                raise ValueError('Observation: photon_rows must be 1 .. 65536')
            shape = (self.n_seconds, C, self.K)
            self.d_words, self.d_stamps = z(shape, torch.int64), z(shape, torch.int64)
            self.d_row_height = torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
            self.d_row_dt = torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
            self.d_dt = z(max(self.cap_join, 1), torch.float32) if self.fit else None
            self.d_dropped, self.d_fill = z(1, torch.int64), z(2, torch.int64)
        self.cur = 0          # d_def[cur], d_ndef[cur]: the packets deferred by the last step
        self.steps = []       # debug: (joined uint64, heights float32, j0, j_defer) of every step
        torch.cuda.synchronize(dev)   # torch's stream made the buffers, the context's stream uses them

    def step(self, d_phase, rows, j0, d_events, d_counts):
        """After the process call that wrote d_phase ([rows][C] from global row j0), d_events and
        d_counts (int64 [2]: [1] = packets stored): count its packets, join them behind the packets
        deferred by the last step, take the heights of the joined list, and bin them; the packets
        whose windows pass this call's last row wait in the other deferred list."""
        ch, cur = self.chan, self.cur
        d_n = d_counts[1:]
        ncoeff, pre = ch.pulse_filter
        L = ch.pulse_fit_search if self.fit else 0
        jd = j_defer(j0, rows, ncoeff, pre, L)
        if self.K is None:
            ch.count_photons_counted(d_events, d_n, self.cap, j0, self.n_seconds, self.d_image, self.d_outside)
        else:
            ch.list_photons_counted(d_events, d_n, self.cap, j0, self.n_seconds, self.K, self.row_layout, self.d_image,
                                    self.d_outside, self.d_words, self.d_stamps, self.d_dropped)
        ch.concat_packets(self.d_def[cur], self.d_ndef[cur][1:], self.cap_def, d_events, d_n, self.cap,
                          self.d_join, self.cap_join, self.d_njoin)
        d_nj = self.d_njoin[1:]
        d_dt = self.d_dt if self.K is not None else None
        if self.fit and d_dt is not None:
            ch.pulse_fit_counted(d_phase, rows, j0, self.d_join, d_nj, self.cap_join, self.d_heights, d_dt)
        else:
            heights = ch.pulse_fit_counted if self.fit else ch.pulse_heights_counted
            heights(d_phase, rows, j0, self.d_join, d_nj, self.cap_join, self.d_heights)
        ch.stream_copy(self.d_ndef[cur ^ 1], self.d_zero, 16)   # on the context's stream: no torch memset
        ch.height_spectra_counted(self.d_join, self.d_heights, d_nj, self.cap_join, j0, jd, self.d_lo, self.d_inv,
                                  self.nbins, self.d_spectra, self.d_def[cur ^ 1], self.cap_def, self.d_ndef[cur ^ 1])
        if self.K is not None:
            ch.fill_photon_heights_counted(self.d_join, self.d_heights, d_dt, d_nj, self.cap_join, j0, jd,
                                           self.n_seconds, self.K, self.d_image, self.d_stamps, self.d_row_height,
                                           self.d_row_dt, self.d_fill)
        self.cur = cur ^ 1
        if self.debug:
            import torch
            torch.cuda.synchronize(ch.torch_device())
            n = int(self.d_njoin[1].item())
            self.steps.append((self.d_join[:n].cpu().numpy().view(np.uint64).copy(),
                               self.d_heights[:n].cpu().numpy().copy(), int(j0), jd))

    def _sync(self):
        import torch
        torch.cuda.synchronize(self.chan.torch_device())

    def image(self):
        """int32 [n_seconds][C]: packets per second and channel."""
        self._sync()
        return self.d_image.cpu().numpy()

    def photon_counts(self, max_events=2500):
        """The image as PacketMaster holds it: a pixel-second keeps at most max_events - 1 events
        (PacketMaster.c:371-381 stops counting there)."""
        return np.minimum(self.image(), int(max_events) - 1)

    def spectra(self):
        """int32 [C][nbins + 3]: under, the nbins bins, over, no height."""
        self._sync()
        return self.d_spectra.cpu().numpy()

    def edges(self, c):
        """The nbins + 1 nominal bin edges of channel c (float64 from the fp32 lo and step; the
        column a height lands in is the fp32 rule's)."""
        return float(self.lo[c]) + np.arange(self.nbins + 1) * float(self.step_width[c])

    def outside(self):
        """int64 [2]: packets of channels >= C, packets of seconds >= n_seconds."""
        self._sync()
        return self.d_outside.cpu().numpy()

    def deferred_counts(self):
        """int64 [2] of the last step: packets deferred, packets kept (less: cap_deferred is too small)."""
        self._sync()
        return self.d_ndef[self.cur].cpu().numpy()

    def pending(self):
        """uint64: the packets still deferred after the last step, in list order."""
        n = int(self.deferred_counts()[1])
        return self.d_def[self.cur][:n].cpu().numpy().view(np.uint64).copy()

    # ---- photon rows (photon_rows=K) ------------------------------------------------------------
    def _rows_on(self):
        if self.K is None:
            raise ValueError('Observation: made without photon_rows')

    def photons(self, sec, ch):
        """The photons stored for pixel ch in second sec, the first min(image, K) of that cell in
        ascending stamp: dict(word uint64, stamp int64 (the unwrapped phase row), us int64
        (microsecond since PPS), height float32, dt float32 (rows; NaN without fit)); a height is
        NaN until the photon's window has completed."""
        self._rows_on()
        self._sync()
        m = min(int(self.d_image[sec, ch].item()), self.K)
        host = lambda t: t[sec, ch, :m].cpu().numpy()
        stamp = host(self.d_stamps)
        return dict(word=host(self.d_words).view(np.uint64), stamp=stamp,
                    us=packets.Timebase(self.chan.cfg.sample_rate, self.chan.N).microsecond(stamp),
                    height=host(self.d_row_height), dt=host(self.d_row_dt))

    def rows(self, sec):
        """Second sec as PacketMaster holds it (its rows[(r, p)][sec] for every pixel p): a list
        of C uint64 arrays, pixel p's the first min(image, K) words of its row."""
        self._rows_on()
        self._sync()
        m = np.minimum(self.d_image[sec].cpu().numpy(), self.K)
        w = self.d_words[sec].cpu().numpy().view(np.uint64)
        return [w[p, :m[p]].copy() for p in range(self.chan.C)]

    def dropped(self):
        """Packets that found their row full (PacketMaster stores none past its 2499th)."""
        self._rows_on()
        self._sync()
        return int(self.d_dropped.item())

    def fill_counts(self):
        """int64 [2]: heights stored in a row; heights whose photon has no slot (its row was full,
        or its second is past n_seconds)."""
        self._rows_on()
        self._sync()
        return self.d_fill.cpu().numpy()
