"""Phase blocks for the threshold-rule tests (test_thresholds_host.py, test_gpu_thresholds.py): the
channel kinds on which the reference's histogram rule can go wrong, one kind per column, mixed so
that neighbouring columns (neighbouring lanes on the device) are of different kinds."""
import numpy as np

FLOOR = -25736
EDGE_RANGES = (1, 5, 99, 100, 101, 200)
KINDS = ('constant', 'edges', 'gauss', 'uniform', 'outlier', 'int16')


def column(rng, kind, rows):
    """One channel of `rows` Fix16_13 samples (int64 values within int16)."""
    if kind == 'constant':
        x = np.full(rows, int(rng.integers(FLOOR, -FLOOR + 1)))
    elif kind == 'edges':      # integer samples land on the bin edges of a 1..200-count range
        x = rng.integers(0, int(rng.choice(EDGE_RANGES)) + 1, rows) + int(rng.integers(-20000, 20001))
    elif kind == 'gauss':      # sigma 0.3 .. 3000 around offsets up to +-20000
        x = np.rint(rng.normal(float(rng.integers(-20000, 20001)), 10 ** rng.uniform(np.log10(0.3), np.log10(3000)), rows))
    elif kind == 'uniform':    # the whole phase range: the -25736 clamp
        x = rng.integers(FLOOR, -FLOOR + 1, rows)
    elif kind == 'outlier':    # a narrow Gaussian with one sample at -pi
        x = np.rint(rng.normal(float(rng.integers(-2000, 2001)), 10 ** rng.uniform(0, 1.5), rows))
        x[int(rng.integers(0, rows))] = FLOOR
    elif kind == 'int16':      # anything an int16 holds
        x = rng.integers(-32768, 32768, rows)
    else:
        raise ValueError(kind)
    return np.clip(x, -32768, 32767).astype(np.int64)


def block(rng, rows, nch, ld=None, kinds=KINDS):
    """int16 [rows][ld]: columns 0..nch-1 cycle through `kinds` from a random start, the columns
    past nch hold junk. Returns (block, kind of each channel)."""
    ld = nch if ld is None else ld
    k0 = int(rng.integers(0, len(kinds)))
    names = [kinds[(k0 + c) % len(kinds)] for c in range(nch)]
    raw = rng.integers(-32768, 32768, (rows, ld)).astype(np.int16)
    for c, kind in enumerate(names):
        raw[:, c] = column(rng, kind, rows)
    return raw, names
