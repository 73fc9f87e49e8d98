"""The observing products of a streamed run, kept on the device: the per-second count image
(PacketMaster's photon_counts[sec][pixel], PacketMaster.c:371-381) and the per-channel pulse-height
spectra, for every channel at once and across calls, with the heights' deferral protocol
(include/mkidgpu.h mkid_pulse_heights: the packets of a call's last rows get their height with the
next call) run on the device too. A step enqueues five calls on the context's stream and makes no
device-to-host copy and no synchronisation. With photon_rows=K it also keeps the product itself:
PacketMaster's per-pixel, per-second photon rows (/r#/p#/t<obs>, PacketMaster.c:978-1050), K slots a
row, each photon with its height (and arrival offset) once the deferral protocol has settled it
(include/mkidgpu.h mkid_list_photons, mkid_fill_photon_heights): six calls a step, still no
synchronisation. With ring=R the rows are a ring of R second slots of bounded memory: ready() says
which seconds are settled, and drain() packs each into PacketMaster's variable-length form on the
device (mkid_pack_second), copies only the photons to the host as a Second, and clears the slot for
reuse (mkid_clear_second), as PacketMaster hands a finished second to its writer
(PacketMaster.c:329-368). calibrate() reads the laser lines out of the spectra (wavecal.py), and with
energy=cal a step also bins every settled photon's energy into the energy or wavelength cube that the
reference's quick-look consumes (include/mkidgpu.h mkid_energy_cube; quicklook.py): one more call a
step, between the heights and the spectra.
"""
import numpy as np

from . import _lib, packets, quicklook, wavecal


def j_defer(j0, rows, ncoeff, pre, search=0):
    """The first stamp whose search window passes the last row of the call that covers global rows
    j0 .. j0 + rows - 1: a window is inside while (jg - j0 - pre) + search + ncoeff <= rows
    (csrc/fit_common.h inside; search = 0 for the plain heights)."""
    return int(j0) + int(rows) + int(pre) - int(ncoeff) - int(search) + 1


def settled_bound(j0, rows, jd):
    """After a step over rows j0 .. j0 + rows - 1 with deferral point jd, every packet stamped below
    min(jd, j0 + rows - 1) is final: a later call stamps no packet below its own j0 - 1 (the trigger
    stamps the packet it emits at row j with j - 1, csrc/k_trigger.hip make_packet), so every such
    packet has been listed; and a packet stamped below jd is not deferred by this step, so it has
    been filled or counted in fill[1]."""
    return min(int(jd), int(j0) + int(rows) - 1)


def ready_seconds(tb, sec0, n_slots, sec_end, settled, last=-1):
    """The seconds of the window [sec0, min(sec0 + n_slots, sec_end)) that are ready, in order: second
    s when every stamp of it lies below the settled bound, tb.first_row(s + 1) <= settled, or when
    s <= last (a final drain)."""
    out, s = [], int(sec0)
    while s < min(int(sec_end), int(sec0) + int(n_slots)) and (tb.first_row(s + 1) <= settled or s <= last):
        out.append(s)
        s += 1
    return out


class Second:
    """One second of photon rows in PacketMaster's variable-length form (include/mkidgpu.h
    mkid_pack_second): counts int32 [C] (the raw counts, the image row), offsets int64 [C + 1]
    (pixel p's photons are entries offsets[p] .. offsets[p + 1]), and per photon word uint64, stamp
    int64, us int64, height and dt float32 (NaN where the height never settled)."""

    def __init__(self, sec, counts, offsets, word, stamp, us, height, dt):
        self.sec, self.counts, self.offsets = int(sec), counts, offsets
        self.word, self.stamp, self.us, self.height, self.dt = word, stamp, us, height, dt

    def row(self, p):
        """Pixel p's photons as Observation.photons(sec, p) gives them."""
        a, b = int(self.offsets[p]), int(self.offsets[p + 1])
        return dict(word=self.word[a:b], stamp=self.stamp[a:b], us=self.us[a:b], height=self.height[a:b],
                    dt=self.dt[a:b])

    def rows(self):
        """The second as Observation.rows(sec) gives it: a list of C uint64 arrays."""
        return [self.word[int(a):int(b)].copy() for a, b in zip(self.offsets[:-1], self.offsets[1:])]


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
    ring        None: the tables above. R (with photon_rows): the tables are [R][C][K], second sec in slot
                sec mod R while it is one of the R seconds from the first undrained one on, and
                n_seconds, the exposure, may be any positive value; drain() takes the settled
                seconds out as Second objects and frees their slots. image(), rows() and photons()
                then raise: the data leave through Second. outside() is int64 [4] there.
    energy      None: no cube, and the calls of a step are exactly those above. A wavecal.EnergyCal
                for the C channels: every step adds one energy_cube_counted call over the joined
                list, after the heights and before the spectra, into the cube int32 [C][nb + 3]
    energy_bins (mode, lo, hi, nb): _lib.CUBE_ENERGY (eV) or _lib.CUBE_WAVELENGTH (hc / e), nb bins
                from lo to hi, bin width float32((hi - lo) / nb) and vinv its float32 reciprocal;
                default: the quick-look's ten wavelength slices (quicklook.slice_bins)
    hc          float32 h c in the units of e times those of the wavelength (default quicklook.H * quicklook.C)
    """

    def __init__(self, chan, n_seconds, nbins, lo, step, cap, cap_deferred, fit=False, debug=False,
                 photon_rows=None, row_layout=_lib.ROW_WIDE, ring=None, energy=None, energy_bins=None, hc=None):
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
        self.R = None if ring is None else int(ring)
        if self.R is not None and (photon_rows is None or not 1 <= self.R <= 1 << 20 or self.n_seconds < 1):
            raise ValueError('Observation(ring=R): needs photon_rows, 1 <= R <= 2^20 and n_seconds >= 1')
        self.sec0 = 0                      # ring: the first second not yet drained
        self.settled, self.j_end = 0, 0    # every packet stamped below `settled` is final; rows processed
        self.d_image = z((self.n_seconds if self.R is None else self.R, C), torch.int32)
        self.d_spectra = z((C, self.nbins + 3), torch.int32)
        self.d_outside = z(2 if self.R is None else 4, torch.int64)
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
            shape = (self.n_seconds if self.R is None else self.R, C, self.K)
            self.d_words, self.d_stamps = z(shape, torch.int64), z(shape, torch.int64)
            self.d_row_height = torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
            self.d_row_dt = torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
            self.d_dt = z(max(self.cap_join, 1), torch.float32) if self.fit else None
            self.d_dropped, self.d_fill = z(1, torch.int64), z(2, torch.int64)
            self.d_pack = None             # the packed second's buffers: a ring's now, else with the first packed()
            if self.R is not None:
                self._pack_buffers()
        self.energy = energy
        if energy is not None:
            if energy.cal_f.shape != (C, 4):
                raise ValueError('Observation(energy=cal): the calibration must cover the C channels')
            self.hc = np.float32(quicklook.H * quicklook.C if hc is None else hc)
            mode, vlo, vhi, nb = energy_bins if energy_bins is not None else quicklook.slice_bins()
            self.cube_mode, self.nb = int(mode), int(nb)
            if self.cube_mode not in (_lib.CUBE_ENERGY, _lib.CUBE_WAVELENGTH) or not 1 <= self.nb <= 16384:
                raise ValueError('Observation(energy_bins=...): a known mode and 1 <= nb <= 16384')
            self.vlo = np.float32(vlo)
            with np.errstate(divide='ignore', invalid='ignore'):
                self.vinv = np.float32(1) / np.float32((np.float32(vhi) - self.vlo) / np.float32(self.nb))
            self.d_cal_f = energy.device_table(chan)
            self.d_cube = z((C, self.nb + 3), torch.int32)
            self.d_energy = z(max(self.cap_join, 1), torch.float32)
        self.step_energies = []   # debug with energy: float32 energies of every step's joined list
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
        elif self.R is not None:
            ch.list_photons_ring_counted(d_events, d_n, self.cap, j0, self.sec0, self.R, self.n_seconds, self.K,
                                         self.row_layout, self.d_image, self.d_outside, self.d_words, self.d_stamps,
                                         self.d_dropped)
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
        if self.energy is not None:
            ch.energy_cube_counted(self.d_join, self.d_heights, d_nj, self.cap_join, j0, jd, self.d_cal_f,
                                   self.cube_mode, self.hc, self.vlo, self.vinv, self.nb, self.d_cube, self.d_energy)
        ch.stream_copy(self.d_ndef[cur ^ 1], self.d_zero, 16)   # on the context's stream: no torch memset
        ch.height_spectra_counted(self.d_join, self.d_heights, d_nj, self.cap_join, j0, jd, self.d_lo, self.d_inv,
                                  self.nbins, self.d_spectra, self.d_def[cur ^ 1], self.cap_def, self.d_ndef[cur ^ 1])
        if self.R is not None:
            ch.fill_photon_heights_ring_counted(self.d_join, self.d_heights, d_dt, d_nj, self.cap_join, j0, jd,
                                                self.sec0, self.R, self.n_seconds, self.K, self.d_image,
                                                self.d_stamps, self.d_row_height, self.d_row_dt, self.d_fill)
        elif self.K is not None:
            ch.fill_photon_heights_counted(self.d_join, self.d_heights, d_dt, d_nj, self.cap_join, j0, jd,
                                           self.n_seconds, self.K, self.d_image, self.d_stamps, self.d_row_height,
                                           self.d_row_dt, self.d_fill)
        self.cur = cur ^ 1
        self.j_end = int(j0) + int(rows)
        self.settled = max(self.settled, settled_bound(j0, rows, jd))
        if self.debug:
            import torch
            torch.cuda.synchronize(ch.torch_device())
            n = int(self.d_njoin[1].item())
            self.steps.append((self.d_join[:n].cpu().numpy().view(np.uint64).copy(),
                               self.d_heights[:n].cpu().numpy().copy(), int(j0), jd))
            if self.energy is not None:
                self.step_energies.append(self.d_energy[:n].cpu().numpy().copy())

    def _sync(self):
        import torch
        torch.cuda.synchronize(self.chan.torch_device())

    def _not_ring(self, what):
        if self.R is not None:
            raise ValueError('Observation(ring=R).%s: a ring keeps no whole table; take the seconds as Second '
                             'objects from drain()' % what)

    def image(self):
        """int32 [n_seconds][C]: packets per second and channel."""
        self._not_ring('image')
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

    def calibrate(self, energies, smooth=2, min_sep=32, min_peak=10, fit_half=12):
        """The laser lines of the observation's own spectra, found and fitted on the device
        (wavecal.spectrum_lines) -> wavecal.EnergyCal, whose table a later Observation takes as
        energy=cal. energies: the line energies in eV in ascending bin order."""
        return wavecal.spectrum_lines(self.chan, self.d_spectra, self.lo, self.step_width, self.nbins, energies, smooth,
                                      min_sep, min_peak, fit_half)

    def cube(self):
        """int32 [C][nb + 3]: under, the nb energy or wavelength bins, over, no energy."""
        if self.energy is None:
            raise ValueError('Observation: made without energy')
        self._sync()
        return self.d_cube.cpu().numpy()

    def edges(self, c):
        """The nbins + 1 nominal bin edges of channel c (float64 from the fp32 lo and step; the
        column a height lands in is the fp32 rule's)."""
        return float(self.lo[c]) + np.arange(self.nbins + 1) * float(self.step_width[c])

    def outside(self):
        """int64 [2]: packets of channels >= C, packets of seconds >= n_seconds; with ring=R int64 [4]:
        then those of seconds already drained, and those the ring had no slot for."""
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
        self._not_ring('photons')
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
        self._not_ring('rows')
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

    # ---- a second in packed form; the ring (ring=R) ----------------------------------------------
    def _pack_buffers(self):
        """Room for any second in packed form: C K entries, one more slot's worth of memory."""
        import torch
        C, dev = self.chan.C, self.chan.torch_device()
        cap = C * self.K
        e = lambda dt: torch.empty(cap, dtype=dt, device=dev)
        self.d_pack = dict(cap=cap, counts=torch.empty(C, dtype=torch.int32, device=dev),
                           offsets=torch.empty(C + 1, dtype=torch.int64, device=dev), word=e(torch.int64),
                           stamp=e(torch.int64), height=e(torch.float32), dt=e(torch.float32),
                           total=torch.empty(2, dtype=torch.int64, device=dev))

    def _packed(self, sec, n_slots, clear):
        """Pack second sec on the device, clear its slot when asked, synchronise once, and copy
        counts, offsets and the second's photons (nothing of the padding) to the host."""
        ch, C = self.chan, self.chan.C
        if self.d_pack is None:
            self._pack_buffers()
            self._sync()                   # torch's stream made the buffers, the context's stream uses them
        b = self.d_pack
        ch.pack_second(sec, n_slots, self.K, self.d_image, self.d_words, self.d_stamps, self.d_row_height,
                       self.d_row_dt, b['cap'], b['counts'], b['offsets'], b['word'], b['stamp'], b['height'], b['dt'],
                       b['total'])
        if clear:
            ch.clear_second(sec, n_slots, self.K, self.d_image, self.d_row_height, self.d_row_dt)
        self._sync()
        offsets = b['offsets'].cpu().numpy()
        m = int(offsets[C])                # cap = C K holds any second
        host = lambda k: b[k][:m].cpu().numpy()
        stamp = host('stamp')
        return Second(sec, b['counts'].cpu().numpy(), offsets, host('word').view(np.uint64), stamp,
                      packets.Timebase(ch.cfg.sample_rate, ch.N).microsecond(stamp), host('height'), host('dt'))

    def packed(self, sec):
        """Second sec of the unbounded tables (ring=None) as a Second; the tables stay as they are."""
        self._rows_on()
        self._not_ring('packed')
        if not 0 <= int(sec) < self.n_seconds:
            raise ValueError('Observation.packed: second outside 0 .. n_seconds - 1')
        return self._packed(int(sec), self.n_seconds, False)

    def _ring_on(self):
        if self.R is None:
            raise ValueError('Observation: made without ring')

    def ready(self, final=False):
        """The seconds from the first undrained one on that are settled, by host arithmetic alone:
        second s is ready when every stamp of it lies below the settled bound,
        Timebase.first_row(s + 1) <= min(j_defer, j0 + rows - 1) of the last step. With final, also
        the seconds up to the last processed row. At most R, and none past the exposure."""
        self._ring_on()
        tb = packets.Timebase(self.chan.cfg.sample_rate, self.chan.N)
        last = int(tb.second(self.j_end - 1)) if final and self.j_end > 0 else -1
        return ready_seconds(tb, self.sec0, self.R, self.n_seconds, self.settled, last)

    def drain(self, final=False):
        """Take every ready second out of the ring, in order -> a list of Second. Each is packed,
        its slot cleared, and the window moved on by one; one synchronisation per second, none
        when nothing is ready. With final the seconds up to the last processed row leave too, the
        heights that never settled NaN."""
        out = []
        while True:                        # a final drain of more than R seconds frees slots as it goes
            todo = self.ready(final)
            if not todo:
                return out
            for s in todo:
                out.append(self._packed(s, self.R, True))
                self.sec0 = s + 1

    def overrun(self):
        """Packets whose second had no slot: the ring is too short, or was not drained in time."""
        self._ring_on()
        self._sync()
        return int(self.d_outside[3].item())

    def early(self):
        """Packets of a second that was already drained."""
        self._ring_on()
        self._sync()
        return int(self.d_outside[2].item())
