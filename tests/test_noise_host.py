"""mkid_phase_noise_spectra_host, the float64 CPU statement of the device noise-spectrum call, against
codecs.noise_spectrum (and the oracle's loop-for-loop restatement of ROACH_Pulses.py:521-532) column
by column. The host call runs the plan, the passes, the index maps and the unpacking of paired
pieces that the kernel runs (csrc/noise_common.h, plan_noise), so a wrong index shows here. No GPU.

Which bins are compared is decided from the reference alone (noise_cases.reference): a bin counts
when every piece's |X| is at least 1e-3 of the rms over the bins k > 0. At most 1 % of a channel's
bins may be left out, which is asserted for every case. It is a condition on the inputs, so
noise_cases.block draws a column again until it holds (the issue's own n <= 64 with 100 averages
and sigma 5 cannot meet it otherwise: bin n / 2 of integer samples is exactly zero in about one
piece in a hundred). Below the floor a value must be finite, or -inf where |X| is exactly 0, which
is what the rule prescribes there; never NaN.

The tail. n = rows // n_averages, so extra rows leave n alone only while there are fewer of them
than n_averages: the tail is 5 rows where n_averages > 5 and n_averages - 1 rows below that.

Tolerance. The largest |host - numpy| over the compared bins of all cases below is 1.41e-9 dB (at
n = 10485 with the (20000, 5) input, where numpy carries the mean of 20 000 counts through its
transform and the host call takes it off first); BAR is 4 x that. Float64 rounding at the floor
allows about 20 log10(1 + 1e-13 / 1e-3) = 1e-9 dB per piece, so the figure is rounding, not an
index."""
import ctypes

import numpy as np
import pytest

import noise_cases
from mkids_sdr_amd import _lib, codecs
from oracle import replay

BAR = 5.7e-9   # dB: 4 x the largest difference measured over this file's cases (1.41e-9)
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 25, 27, 49, 64, 105, 233, 466, 1000, 1024, 10485)
WORST = {}


def averages(n):
    return (1, 2, 3, 8, 100) if n <= 64 else (1, 2, 3, 8)


def tail(n_averages):
    return min(5, n_averages - 1)


def host(raw, nch, n_averages, norm1=50.0):
    freqs, spec = codecs.phase_noise_spectra_host(raw, n_averages, norm1, nch=nch)
    assert spec.shape == (nch, raw.shape[0] // n_averages) and spec.dtype == np.float64
    assert np.array_equal(freqs, np.fft.fftfreq(spec.shape[1]))
    return spec


@pytest.mark.parametrize('n', LENGTHS)
def test_host_matches_numpy(n):
    """Every n_averages, input kind, tail, nch in {1, 3} and ld in {nch, nch + 2} at this length.
    The eight block shapes of a case hold the same columns, so their channels must agree bit for bit
    (a channel depends on its own column only), and the three columns are compared with numpy once."""
    worst = 0.0
    for na in averages(n):
        for kind in range(len(noise_cases.INPUTS)):
            rows = n * na + tail(na)
            wide = noise_cases.block(100003 * n + 101 * na + kind, rows, 5, kind, na)   # nch 3, ld 5
            got = host(wide, 3, na)
            for c in range(3):
                _, ref_c = codecs.noise_spectrum(wide[:, c] * codecs.SCALE_TO_ANGLE, na)
                spec, compared = noise_cases.reference(wide[:, c:c + 1], na)
                assert np.abs(spec[0] - ref_c)[compared[0]].max() < 1e-11
                d = noise_cases.worst_db(got[c:c + 1], ref_c[None], compared)
                worst = max(worst, d)
                assert d <= BAR, (n, na, kind, c, d)
            for r in (0, tail(na)):                   # without and with the tail
                blk = wide[:n * na + r]
                for nch, ld in ((3, 3), (3, 5), (1, 1), (1, 3)):
                    shaped = np.ascontiguousarray(blk[:, :ld])
                    assert host(shaped, nch, na).tobytes() == got[:nch].tobytes(), (n, na, kind, r, nch, ld)
    WORST[n] = worst
    print('n = %d: largest |host - numpy| %.3g dB' % (n, worst))


def test_oracle_loop_spot_checks():
    """The reference's own loop (oracle.replay.noise_spectrum_loop) on a few columns."""
    for n, na, kind in ((16, 100, 0), (105, 3, 1), (233, 8, 2), (1024, 2, 0)):
        raw = noise_cases.block(7 + n, n * na, 2, kind, na)
        got = host(raw, 2, na)
        for c in range(2):
            freqs, ref = replay.noise_spectrum_loop(raw[:, c] * codecs.SCALE_TO_ANGLE, na)
            _, compared = noise_cases.reference(raw[:, c:c + 1], na)
            assert noise_cases.worst_db(got[c:c + 1], ref[None], compared) <= BAR
            assert np.array_equal(freqs, np.fft.fftfreq(n))


def test_zero_column_is_minus_infinity_and_neighbours_are_finite():
    for n, na in ((1, 1), (7, 3), (64, 2), (105, 1)):
        raw = noise_cases.block(n, n * na, 3, 2)
        raw[:, 1] = 0
        got = host(raw, 3, na)
        assert np.isneginf(got[1]).all()
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
        # one zero piece among non-zero ones: the mean over the pieces is -inf too, never NaN
        raw = noise_cases.block(n + 1, n * na, 1, 2)
        raw[:n] = 0
        assert np.isneginf(host(raw, 1, na)).all()


@pytest.mark.parametrize('n,row,amp', [(1, 0, 3), (8, 0, 1000), (105, 17, -25736), (233, 232, 25736), (1024, 500, -1)])
def test_single_sample_gives_a_flat_spectrum(n, row, amp):
    raw = np.zeros((n, 1), np.int16)
    raw[row, 0] = amp
    for norm1 in (50.0, 3.5):
        got = host(raw, 1, 1, norm1)[0]
        flat = 20 * np.log10(abs(amp) * codecs.SCALE_TO_ANGLE / norm1 / 1e-6)
        assert np.abs(got - flat).max() <= BAR


def test_scale_and_norm1_enter_as_one_constant():
    raw = noise_cases.block(3, 64 * 3, 2, 0)
    L = _lib.load()
    out = {}
    for scale, norm1 in ((codecs.SCALE_TO_ANGLE, 50.0), (1.0, 1.0), (0.25, 7.0)):
        spec = np.zeros((2, 64))
        assert L.mkid_phase_noise_spectra_host(raw.ctypes.data_as(ctypes.c_void_p), 192, 2, 2, 3, scale, norm1,
                                               spec.ctypes.data_as(ctypes.c_void_p)) == 0
        out[(scale, norm1)] = spec
        ref = np.stack([codecs.noise_spectrum(raw[:, c] * scale, 3, norm1)[1] for c in range(2)])
        assert np.abs(spec - ref).max() <= BAR
    assert np.abs(out[(1.0, 1.0)] - out[(0.25, 7.0)] - 20 * np.log10(28.0)).max() < 1e-10


def test_host_entry_point_argument_errors():
    L = _lib.load()
    raw = np.ones((12, 6), np.int16)
    spec = np.full((6, 4), 77.0)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ok = (P(raw), 12, 6, 6, 3, 1.0, 50.0, P(spec))

    def call(**kw):
        names = ('raw', 'rows', 'ld', 'nch', 'n_averages', 'scale', 'norm1', 'spec')
        return L.mkid_phase_noise_spectra_host(*[kw.get(n, v) for n, v in zip(names, ok)])

    bad = [dict(raw=None), dict(spec=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(nch=0), dict(nch=-3),
           dict(nch=7), dict(n_averages=0), dict(n_averages=-1), dict(n_averages=13),
           dict(rows=16385, n_averages=1), dict(rows=2 * 16384 + 2, n_averages=2),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=float('inf')), dict(scale=float('nan')),
           dict(norm1=0.0), dict(norm1=-50.0), dict(norm1=float('inf')), dict(norm1=float('nan'))]
    for kw in bad:
        assert call(**kw) == _lib.MKID_E_ARG, kw
        assert (spec == 77.0).all()
    assert call(nch=2) == 0
    assert (spec[:2] != 77.0).all() and (spec[2:] == 77.0).all()
    with pytest.raises(_lib.MkidError):
        codecs.phase_noise_spectra_host(raw, 0)


def test_binding_lists_the_noise_calls():
    for name in ('mkid_phase_noise_spectra', 'mkid_phase_noise_spectra_host'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
