"""mkid_phase_thresholds_host, the CPU statement of the device threshold call, against the host rule
codecs.threshold_from_phase (and the oracle's restatement of ROACH_Pulses.py:259-278) column by
column. Everything is exact: thresholds as integers, med and p05 bitwise as float64, lo and hi as
integers. The rule has integer counts and a fixed sequence of IEEE float64 operations only, so no
tolerance applies. No GPU."""
import ctypes
import os

import numpy as np
import pytest

import thr_cases
from mkids_sdr_amd import _lib, codecs
from oracle import setup_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROWS = (1, 2, 7, 8, 9, 100, 101, 10240)
NSIGMA = (0.0, 2.5, 6.0)


def numpy_rule(x, nsigma):
    """codecs.threshold_from_phase with the 5 % edge and the range reported too."""
    n, bins = np.histogram(x, bins=100)
    n = np.array(n, dtype='float32') / np.sum(n)
    tot = np.array([np.sum(n[:i]) for i in range(len(bins))])
    med = bins[np.abs(tot - 0.5).argmin()]
    p05 = bins[np.abs(tot - 0.05).argmin()]
    return max(int(-nsigma * abs(med - p05)), -25736), med, p05, int(np.min(x)), int(np.max(x))


def bits(v):
    """The bit pattern of one float64."""
    return int(np.float64(v).view(np.int64))


def check_block(raw, nch, nsigma):
    """The host entry point on columns 0..nch-1 of raw against the numpy rule; returns thr."""
    thr, med, st = codecs.phase_thresholds_host(raw, nsigma, nch=nch, want_stats=True)
    assert thr.shape == (nch,) and thr.dtype == np.int32
    for c in range(nch):
        x = raw[:, c]
        t, m, p, lo, hi = numpy_rule(x, nsigma)
        tc, mc = codecs.threshold_from_phase(x, nsigma)
        assert (t, bits(m)) == (tc, bits(mc))
        # the int64 samples the shim's decoders hand to the rule give the same histogram
        t64, m64 = codecs.threshold_from_phase(x.astype(np.int64), nsigma)
        assert (t, bits(m)) == (t64, bits(m64))
        got = (int(thr[c]), bits(med[c]), bits(st['p05'][c]), int(st['lo'][c]), int(st['hi'][c]))
        assert got == (t, bits(m), bits(p), lo, hi), (c, raw.shape, nsigma)
        assert bits(st['med'][c]) == bits(med[c])
    return thr


@pytest.mark.parametrize('rows', ROWS)
def test_host_rule_matches_numpy_on_every_channel_kind(rows):
    """Every channel kind at every row count, ld > nch with junk in the unused columns, the three
    nsigma; 36 columns per block, 288 per row count: 2304 random channels over the module."""
    rng = np.random.default_rng(1000 + rows)
    for trial in range(8):
        nsigma = NSIGMA[trial % 3]
        raw, kinds = thr_cases.block(rng, rows, 36, ld=36 + (trial % 2) * 5)
        thr = check_block(raw, 36, nsigma)
        if rows >= 100 and nsigma >= 2.5:   # a full-range channel: 2.5 x 45 % of 51 472 counts
            uni = [c for c, k in enumerate(kinds) if k == 'uniform']
            assert uni and all(thr[c] == -25736 for c in uni)
        if nsigma == 0.0:
            assert not thr.any()


def test_edge_ranges_and_constants_exhaustively():
    """Ranges of 1, 5, 99, 100, 101 and 200 counts with every value present (integer samples on bin
    edges), at offsets of both signs, and constant channels at the ends of the int16 range, where the
    unit-wide range's last cut point passes 32767."""
    rng = np.random.default_rng(5)
    cols = []
    for span in thr_cases.EDGE_RANGES:
        for off in (-20000, -span, -1, 0, 7, 19999):
            x = np.concatenate([np.arange(span + 1), rng.integers(0, span + 1, 199 - span if span < 199 else 50)])
            cols.append(rng.permutation(np.resize(x, 256)) + off)
    for v in (-32768, -25736, -1, 0, 1, 25736, 32767):
        cols.append(np.full(256, v))
    raw = np.stack(cols, axis=1).astype(np.int16)
    for nsigma in NSIGMA:
        check_block(raw, raw.shape[1], nsigma)


def test_reference_snapshot_and_oracle():
    """The reference's only real phase record and a few synthetic channels, against the oracle's
    restatement of the reference (oracle/setup_ref.threshold_from_phase)."""
    deg = np.loadtxt(os.path.join(GOLD, 'ch_snap_0.txt'))
    snap = np.rint(deg / codecs.fix16_13_to_deg(1)).astype(np.int64)
    rng = np.random.default_rng(9)
    cols = [snap, snap[::-1], snap // 2] + [np.resize(thr_cases.column(rng, k, 777), len(snap)) for k in thr_cases.KINDS]
    raw = np.stack(cols, axis=1).astype(np.int16)
    for nsigma in NSIGMA:
        thr = check_block(raw, raw.shape[1], nsigma)
        for c in range(raw.shape[1]):
            t, m = setup_ref.threshold_from_phase(raw[:, c].astype(np.int64), nsigma)
            assert int(thr[c]) == t
    thr, med = codecs.phase_thresholds_host(raw)
    assert np.array_equal(thr, codecs.thresholds_from_phase_block(raw))


def test_host_entry_point_argument_errors():
    L = _lib.load()
    raw = np.zeros((4, 6), np.int16)
    thr = np.full(6, 77, np.int32)
    st = np.zeros(6 * 3, np.float64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ok = (P(raw), 4, 6, 6, 2.5, P(thr), P(st))

    def call(**kw):
        names = ('raw', 'rows', 'ld', 'nch', 'nsigma', 'thr', 'stats')
        return L.mkid_phase_thresholds_host(*[kw.get(n, v) for n, v in zip(names, ok)])

    bad = [dict(raw=None), dict(thr=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(nch=0), dict(nch=-3),
           dict(nch=7), dict(nsigma=-0.5), dict(nsigma=float('inf')), dict(nsigma=float('nan'))]
    for kw in bad:
        assert call(**kw) == _lib.MKID_E_ARG, kw
        assert (thr == 77).all() and not st.any()
    assert call(stats=None) == 0 and not thr.any() and not st.any()
    thr[:] = 77
    assert call(nch=2) == 0 and list(thr) == [0, 0, 77, 77, 77, 77]
    with pytest.raises(_lib.MkidError):
        codecs.phase_thresholds_host(raw, nsigma=-1.0)


def test_binding_lists_the_threshold_calls():
    assert ctypes.sizeof(_lib.ThrStats) == 24
    for name in ('mkid_phase_thresholds', 'mkid_phase_thresholds_host', 'mkid_phase_thresholds_block_rows'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
