"""mkid_phase_noise_spectra on the device against codecs.noise_spectrum on the same block, through the
C ABI, the Channelizer front end and the register shim; and the properties the call promises bit for
bit: a channel's spectrum depends on its own column only, repeats from run to run, and survives a
change of the context's tables in between.

Bins are compared by the rule of tests/test_noise_host.py (noise_cases.reference / worst_db: at or
above 1e-3 of the rms over the bins k > 0 in every piece, at most 1 % of a channel's bins left out,
below the floor finite or the rule's -inf, never NaN); the inputs are the same three kinds.

The tail. n = rows // n_averages: extra rows leave n alone only while they are fewer than
n_averages, so the tail is 3 rows at n_averages = 4 and 5 rows at n_averages = 8.

Tolerance. The largest |device - numpy| over the compared bins of every case of
test_device_matches_numpy, measured on an MI355X, is MEASURED dB; BAR is 4 x that. The composite
lengths stay below 4.3e-4 dB (n = 10485), the short ones below 1e-5 dB. Single-precision
rounding of about 2e-6 of the spectrum's rms moves a bin at the floor by 20 log10(1 + 2e-3) =
0.02 dB, which a correct transform must stay below."""
import numpy as np
import pytest

import noise_cases
import signals
from mkids_sdr_amd import _lib, codecs

pytestmark = pytest.mark.gpu

MEASURED = 3.89e-3   # dB, at n = 16381 (prime: one direct 16381-term sum per bin); 4.3e-4 at n = 10485
BAR = 4 * MEASURED
GUARD = 8         # float64 elements past the spectra that must stay as they were
FILL = 777.0
SHAPES = [(1, 3, 2, 2), (2, 2, 1, 1), (16, 3, 3, 5), (105, 3, 2, 3), (233, 4, 65, 80), (466, 2, 3, 3),
          (1000, 5, 64, 64), (1024, 8, 64, 72), (64, 100, 3, 3), (10485, 3, 2, 2), (16384, 1, 1, 1),
          (16381, 1, 1, 1)]


@pytest.fixture(scope='module')
def ctx(gpu):
    from mkids_sdr_amd.channelizer import Channelizer
    ch = Channelizer(64, max_chunk=1 << 16)
    yield ch
    ch.close()


def device_call(ch, raw, nch, n_averages, offset=0, norm1=50.0):
    """One device call on columns 0..nch-1 of the host block raw [rows][ld], placed `offset` int16
    into a 16-byte-aligned allocation. Returns spec [nch][n] after checking that the block and the
    elements past the spectra are untouched."""
    import torch
    dev = ch.torch_device()
    rows, ld = raw.shape
    n = rows // n_averages
    flat = np.concatenate([np.full(offset, 12345, np.int16), raw.ravel()])
    d_flat = torch.from_numpy(flat).to(dev)
    assert d_flat.data_ptr() % 16 == 0
    d_spec = torch.full((nch * n + GUARD,), FILL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ch.noise_spectra_device(d_flat.data_ptr() + 2 * offset, rows, ld, nch, n_averages, codecs.SCALE_TO_ANGLE, norm1,
                            d_spec)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_flat.cpu().numpy(), flat), 'the block was written'
    spec = d_spec.cpu().numpy()
    assert (spec[nch * n:] == FILL).all(), 'd_spec written past [nch][n]'
    return spec[:nch * n].reshape(nch, n)


@pytest.mark.parametrize('n,n_averages,nch,ld', SHAPES)
def test_device_matches_numpy(ctx, n, n_averages, nch, ld):
    worst = 0.0
    for kind in range(len(noise_cases.INPUTS)):
        raw = noise_cases.block(1000 * n + 10 * n_averages + kind, n * n_averages, ld, kind, n_averages)
        got = device_call(ctx, raw, nch, n_averages)
        spec, compared = noise_cases.reference(raw[:, :nch], n_averages)
        _, one = codecs.noise_spectrum(raw[:, nch - 1] * codecs.SCALE_TO_ANGLE, n_averages)
        assert np.abs(spec[nch - 1] - one)[compared[nch - 1]].max() < 1e-11   # the reference is codecs.noise_spectrum
        worst = max(worst, noise_cases.worst_db(got, spec, compared))
    print('n %d x %d, %d of %d channels: largest |device - numpy| %.3g dB' % (n, n_averages, nch, ld, worst))
    assert worst <= BAR
    assert device_call(ctx, raw, nch, n_averages).tobytes() == got.tobytes()   # from run to run


@pytest.mark.parametrize('n', [4095, 4096, 4097])
def test_lengths_around_the_workgroup_threshold(ctx, n):
    """Up to n = 4096 a workgroup has 256 threads of 16 positions, above it 1024: the last length
    that fills the small workgroup, its neighbour below and the first length of the large one."""
    raw = noise_cases.block(n, n * 3, 2, 0, 3)
    got = device_call(ctx, raw, 2, 3)
    spec, compared = noise_cases.reference(raw, 3)
    assert noise_cases.worst_db(got, spec, compared) <= BAR


def test_a_channel_depends_on_its_own_column_only(ctx):
    """The channel at column 1 of a (233, 4) block: alone, as column 0 and column 64 of a 65-wide
    block, with ld odd and even, one int16 off alignment, with other neighbours, with a tail."""
    n, na = 233, 4
    base = noise_cases.block(5, n * na, 3, 0, na)
    x = base[:, 1].copy()
    want = device_call(ctx, base, 3, na)[1].tobytes()
    assert device_call(ctx, x[:, None].copy(), 1, na)[0].tobytes() == want                  # alone
    wide = noise_cases.block(6, n * na, 65, 2)
    for col in (0, 64):
        w = wide.copy()
        w[:, col] = x
        assert device_call(ctx, w, 65, na)[col].tobytes() == want                           # ld 65, odd
        assert device_call(ctx, w, 65, na, offset=1)[col].tobytes() == want                 # unaligned
    w = np.concatenate([wide, wide[:, :7]], axis=1)                                         # ld 72
    w[:, 64] = x
    assert device_call(ctx, w, 65, na, offset=3)[64].tobytes() == want
    other = noise_cases.block(7, n * na, 3, 1)                                              # other neighbours
    other[:, 1] = x
    assert device_call(ctx, other, 3, na)[1].tobytes() == want
    assert device_call(ctx, other, 2, na)[1].tobytes() == want                              # nch < ld
    tailed = np.concatenate([other, noise_cases.block(8, 3, 3, 0)])                         # 3 rows more
    assert device_call(ctx, tailed, 3, na)[1].tobytes() == want


def test_tail_of_five_rows_changes_nothing(ctx):
    n, na = 64, 8
    raw = noise_cases.block(9, n * na + 5, 4, 0)
    assert device_call(ctx, raw, 4, na).tobytes() == device_call(ctx, raw[:n * na].copy(), 4, na).tobytes()


def test_zero_column_is_minus_infinity_beside_finite_neighbours(ctx):
    for n, na in ((105, 3), (1024, 2), (4099, 2)):
        raw = noise_cases.block(n, n * na, 3, 2)
        raw[:, 1] = 0
        got = device_call(ctx, raw, 3, na)
        assert np.isneginf(got[1]).all()
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
        raw[n:, 1] = raw[n:, 0]           # only the first piece is zero: still -inf, never NaN
        assert np.isneginf(device_call(ctx, raw, 3, na)[1]).all()


def test_tables_replaced_between_calls(ctx):
    """A call with another n replaces the context's tables; the call after it equals the first."""
    a = noise_cases.block(1, 233 * 3, 2, 0)
    b = noise_cases.block(2, 4100 * 2, 2, 2)
    first = device_call(ctx, a, 2, 3).tobytes()
    other = device_call(ctx, b, 2, 2).tobytes()
    assert device_call(ctx, a, 2, 3).tobytes() == first
    assert device_call(ctx, b, 2, 2).tobytes() == other


def test_argument_errors_leave_the_output(ctx):
    import torch
    dev = ctx.torch_device()
    raw = torch.ones((12, 6), dtype=torch.int16, device=dev)
    spec = torch.full((6 * 4,), FILL, dtype=torch.float64, device=dev)
    ok = dict(d_raw=raw, rows=12, ld=6, nch=6, n_averages=3, scale=1.0, norm1=50.0, d_spec=spec)
    bad = [dict(d_raw=None), dict(d_spec=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(nch=0),
           dict(nch=-3), dict(nch=7), dict(n_averages=0), dict(n_averages=-1), dict(n_averages=13),
           dict(rows=16385, n_averages=1), dict(rows=2 * 16384 + 2, n_averages=2),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=float('inf')), dict(scale=float('nan')),
           dict(norm1=0.0), dict(norm1=-50.0), dict(norm1=float('inf')), dict(norm1=float('nan'))]
    for kw in bad:
        with pytest.raises(_lib.MkidError) as e:
            ctx.noise_spectra_device(**dict(ok, **kw))
        assert e.value.code == _lib.MKID_E_ARG, kw
        torch.cuda.synchronize(dev)
        assert (spec == FILL).all(), kw
    ctx.noise_spectra_device(**ok)
    torch.cuda.synchronize(dev)
    assert not (spec == FILL).any()


def test_channelizer_noise_spectra_end_to_end(gpu):
    """A 64-channel context on a short quiet stream: noise_spectra() on the call's rows where they
    lie equals, bit for bit, the call on raw_phase() uploaded again, and agrees with the host rule."""
    from mkids_sdr_amd.channelizer import Channelizer
    C, S, na = 64, 1 << 17, 4
    quiet = signals.make_case(C, S, seed=21, pulses_per_ch=0)
    ch = Channelizer(C, max_chunk=S)
    try:
        ch.set_pfb(quiet.pfb)
        ch.set_bins(quiet.bins)
        ch.set_dds(quiet.lut_i, quiet.lut_q)
        ch.set_lpf(quiet.lpf12)
        ch.set_fir(quiet.fir12)
        ch.set_centers(quiet.ic, quiet.qc)
        ch.set_thresholds(np.full(C, -(1 << 30), np.int64))
        ch.process(quiet.iq, want_phase=False)      # the start-up transient
        ch.process(quiet.iq, want_phase=False)
        raw = ch.raw_phase()
        freqs, spec = ch.noise_spectra(n_averages=na)
        freqs2, again = ch.noise_spectra(raw, n_averages=na)
    finally:
        ch.close()
    n = raw.shape[0] // na
    assert spec.shape == (C, n) and np.array_equal(freqs, np.fft.fftfreq(n)) and np.array_equal(freqs2, freqs)
    assert spec.tobytes() == again.tobytes()
    ref, compared = noise_cases.reference(raw, na)
    with np.errstate(invalid='ignore'):
        d = float(np.abs(spec - ref)[compared].max())
    print('quiet stream, %d channels, n %d: largest |device - numpy| %.3g dB, %.3g of the bins below the floor'
          % (C, n, d, 1 - compared.mean()))
    assert d <= BAR and not np.isnan(spec).any()


def test_shim_noise_spectra_block(gpu):
    """RoachPulses.noiseSpectraBlock on a 256-channel FpgaClient: one block of the running stream,
    every channel < N_freqs in one device call, against the host rule on the rows it returns."""
    from mkids_sdr_amd.roach import FpgaClient, RoachPulses, RoachSetup
    C, nf = 256, 16
    roach = FpgaClient(n_channels=C, noise_sigma=40.0, seed=3)
    roach.progdev('pulse_trigger_2022_Jan_24_1322.bof')
    rng = np.random.default_rng(9)
    freqs = list(4.0e9 + rng.choice(np.arange(-250, 250), nf, replace=False) * 1e6 + 15625.0)
    rs = RoachSetup(roach, freqs, 4.0e9, n_channels=C)
    rs.define_LUTs()
    rs.toggleDAC()
    rs.rotateLoopsReady()
    rp = RoachPulses(roach, nf, None, n_channels=C)
    for rows in (4096, 2048):                 # run in pieces / one piece (its rows still on the device)
        out = rp.noiseSpectraBlock(rows=rows, n_averages=4, keep_raw=True)
        raw, spec = out['raw'], out['noiseFFT']
        n = rows // 4
        assert raw.shape == (rows, nf) and raw.dtype == np.int16 and spec.shape == (nf, n)
        assert np.array_equal(out['noiseFFTFreqs'], np.fft.fftfreq(n))
        worst = 0.0
        for c in range(nf):
            with np.errstate(divide='ignore', invalid='ignore'):
                _, ref = codecs.noise_spectrum(raw[:, c] * codecs.SCALE_TO_ANGLE, 4)
                _, compared = noise_cases.reference(raw[:, c:c + 1], 4)
                worst = max(worst, float(np.abs(spec[c] - ref)[compared[0]].max()))
        print('shim block of %d rows: largest |device - numpy| %.3g dB' % (rows, worst))
        assert worst <= BAR and not np.isnan(spec).any()
    assert 'raw' not in rp.noiseSpectraBlock(rows=2048, n_averages=4)
