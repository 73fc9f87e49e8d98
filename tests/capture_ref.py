"""Numpy statement of the pulse-capture contract (include/mkidgpu.h mkid_capture_pulses,
k_capture.hip) over a list of calls, each (phase rows [rows][C] float32, j0, packets uint64).

A stream segment is a run of calls whose j0 each continue the previous call's rows; it covers rows
[j_first, j_end). A packet (channel c < C, 28-bit stamp unwrapped to jg with the j0 of the call
that delivers it) is eligible when s = jg - pre >= j_first, completes in the call where
s + L <= j_end first holds, and is then recorded (records[c][k] = phase[s : s + L, c], stamps[c][k]
= jg) while the channel holds fewer than R records, else counted in info[c][1]. Completion order in
a channel is list order, pending packets first; the lists are channel-major and time-ascending.
The context carries H = max(L - 1, pre + 1) rows between calls, enough for every packet stamped
at or after j0 - 1; an older hand-made stamp whose window starts before them is not eligible.
`pend_cap` (None: unbounded) is the per-channel room of the pending list,
(L - pre) // max(dead_time, 1) + 2 on the device; packets beyond it count as dropped.
"""
import numpy as np

CH_SHIFT = 52
TS_MASK = (1 << 28) - 1


def pack(ch, ts):
    return np.uint64((int(ch) << CH_SHIFT) | (int(ts) & TS_MASK))


def unwrap(ts, j0):
    base = max(j0 - (1 << 27), 0)
    return base + ((ts - base) % (1 << 28))


def pend_cap(length, pre, dead_time=32):
    return (length - pre) // max(dead_time, 1) + 2


class CaptureRef:
    def __init__(self, C, length, pre, max_per_ch, pend_cap=None, bank=None):
        self.C, self.L, self.pre, self.R, self.PC = C, length, pre, max_per_ch, pend_cap
        self.H = max(length - 1, pre + 1)
        if bank is None:
            bank = (np.zeros((C, max_per_ch, length), np.float32), np.zeros((C, max_per_ch), np.int64),
                    np.zeros((C, 2), np.int32))
        self.records, self.stamps, self.info = bank
        # what the inputs exercised: the tests assert these on the reference, not on the device
        self.stats = dict(recorded=0, skipped=0, other_channel=0, dropped=0, carried=0, prev_row=0, spanned=0,
                          waited3=0)
        self.reset()

    def reset(self):
        """mkid_reset_stream / a break in j0: carried rows and pending packets are forgotten."""
        self.end = None
        self.buf = None
        self.pending = [[] for _ in range(self.C)]   # per channel: [jg, calls seen]

    @property
    def n_pending(self):
        return sum(len(p) for p in self.pending)

    def call(self, phase, j0, events):
        phase = np.asarray(phase, np.float32).reshape(-1, self.C)
        rows = phase.shape[0]
        if self.end != j0:
            self.reset()
            self.buf = np.zeros((0, self.C), np.float32)
        carried = self.buf[max(self.buf.shape[0] - self.H, 0):]
        first = j0 - carried.shape[0]            # = max(j_first, j0 - H)
        self.buf = np.concatenate([carried, phase])
        j_end = j0 + rows
        ev = [int(w) for w in np.asarray(events, np.uint64).tolist()]
        chs = [w >> CH_SHIFT & 0xFFF for w in ev]
        assert chs == sorted(chs), 'packets must be channel-major'
        new = [[] for _ in range(self.C)]
        for w, c in zip(ev, chs):
            if c >= self.C:
                self.stats['other_channel'] += 1
                continue
            jg = unwrap(w & TS_MASK, j0)
            if jg - self.pre < first:
                self.stats['skipped'] += 1
                continue
            self.stats['prev_row'] += jg == j0 - 1
            new[c].append([jg, 0])
        for c in range(self.C):
            still = []
            for jg, seen in self.pending[c] + new[c]:
                s = jg - self.pre
                if s + self.L <= j_end:
                    k = self.info[c, 0]
                    if k < self.R:
                        self.records[c, k] = self.buf[s - first:s - first + self.L, c]
                        self.stamps[c, k] = jg
                        self.info[c, 0] = k + 1
                        self.stats['recorded'] += 1
                        self.stats['carried'] += seen == 0 and s < j0
                        self.stats['spanned'] += seen >= 1
                        self.stats['waited3'] += seen >= 2
                    else:
                        self.info[c, 1] += 1
                        self.stats['dropped'] += 1
                elif self.PC is not None and len(still) >= self.PC:
                    self.info[c, 1] += 1
                    self.stats['dropped'] += 1
                else:
                    still.append([jg, seen + 1])
            self.pending[c] = still
        self.end = j_end


def capture(calls, C, length, pre, max_per_ch, pend_cap=None, bank=None):
    """Run the calls through one CaptureRef; returns it (records, stamps, info, stats, n_pending)."""
    ref = CaptureRef(C, length, pre, max_per_ch, pend_cap, bank)
    for phase, j0, events in calls:
        ref.call(phase, j0, events)
    return ref
