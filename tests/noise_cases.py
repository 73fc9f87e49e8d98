"""Inputs and the numpy reference shared by tests/test_noise_host.py and tests/test_gpu_noise.py:
seeded Fix16_13 noise blocks, codecs.noise_spectrum restated for a whole block at once, and the rule
that says which bins of a case are compared."""
import numpy as np

from mkids_sdr_amd import codecs

# (offset, sigma) of rint(normal(offset, sigma)) clipped to the Fix16_13 range of +-pi
INPUTS = ((-8000, 300), (20000, 5), (0, 300))
FLOOR = 1e-3          # a bin counts when every piece's |X| is at least FLOOR x the rms over bins k > 0
MAX_LEFT_OUT = 0.01   # at most this share of a channel's bins may lie below the floor


def column(seed, rows, kind):
    off, sigma = INPUTS[kind]
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(off, sigma, rows)), -25736, 25736).astype(np.int16)


def block(seed, rows, ld, kind, n_averages=None):
    """int16 [rows][ld], column c seeded with seed + c. With n_averages, every column meets the
    condition on the bins left out (MAX_LEFT_OUT): a column that does not is drawn again with the
    next seed (+ 7919). That matters where n is small and the pieces many: integer samples put an
    exact zero into the bins that are plain sums and differences (k = n / 2, n / 4, ...) of about
    one piece in a hundred at sigma 5, and one bin of a short spectrum is more than 1 % of it.
    The choice looks at the reference only, never at the code under test."""
    cols = []
    for c in range(ld):
        for attempt in range(20000):
            x = column(seed + c + 7919 * attempt, rows, kind)
            if n_averages is None or rows // n_averages < 1:
                break
            _, compared = reference(x[:, None], n_averages)
            if 1.0 - compared.mean() <= MAX_LEFT_OUT:
                break
        else:
            raise AssertionError('no column with at most %g of its bins below the floor' % MAX_LEFT_OUT)
        cols.append(x)
    return np.stack(cols, axis=1)


def reference(raw, n_averages, norm1=50.0, scale=codecs.SCALE_TO_ANGLE):
    """raw int16 [rows][nch] -> (spec float64 [nch][n], compared bool [nch][n]): the computation of
    codecs.noise_spectrum for every column at once, and the bins at or above the floor."""
    rows, nch = raw.shape
    n = rows // n_averages
    x = (raw[:n * n_averages].T.astype(np.float64) * scale).reshape(nch, n_averages, n)
    mag = np.abs(np.fft.fft(x, axis=2))
    with np.errstate(divide='ignore'):
        spec = (20 * np.log10(mag / norm1 / 1e-6)).sum(axis=1) / n_averages
    rms = np.sqrt(np.mean(mag[:, :, 1:] ** 2, axis=(1, 2))) if n > 1 else np.zeros(nch)
    low = mag.min(axis=1)
    compared = (low >= FLOOR * rms[:, None]) & (low > 0)   # an exact zero is below any floor
    return spec, compared


def worst_db(got, spec, compared):
    """The largest |got - spec| in dB over the compared bins after checking the conditions every case
    has to meet: at most MAX_LEFT_OUT of a channel's bins left out; a finite value in every compared
    bin; below the floor a finite value or the -inf that the rule gives a bin with |X| == 0, never
    NaN or +inf."""
    left_out = 1.0 - compared.mean(axis=1)
    assert (left_out <= MAX_LEFT_OUT).all(), 'bins below the floor: %s' % left_out
    assert np.isfinite(got[compared]).all()
    assert (np.isfinite(got[~compared]) | np.isneginf(got[~compared])).all()
    return float(np.abs(got - spec)[compared].max())
