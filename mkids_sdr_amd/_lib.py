"""ctypes binding of libmkidgpu.so (include/mkidgpu.h).

The shared library is the product: it is built in-tree (``mkids_sdr_amd/libmkidgpu.so``) by
``__graft_entry__.build()`` / ``make -C mkids_sdr_amd/csrc``. There is no CPU fallback: importing
the binding without the library, or creating a context without a GPU, raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MKID_LIB: a build variant to test in place of the in-tree library (tools/build_variant.sh A/Bs)
LIB_PATH = os.environ.get('MKID_LIB') or os.path.join(HERE, 'libmkidgpu.so')

MKID_OK = 0
MKID_E_ARG = -1
MKID_E_HIP = -2
MKID_E_STATE = -3
MKID_E_OVERFLOW = -4
MKID_E_NODEV = -5

BASE_NONE, BASE_EMA, BASE_SVF = 0, 1, 2
K_CHANNELIZE, K_FIR_PHASE, K_TRIGGER, K_COMPACT, K_FRONT, K_COPY, K_HEIGHTS, K_CAPTURE, K_COUNT = range(9)
FRONT_AUTO, FRONT_SPLIT = 0, 1

PKT_CH_SHIFT, PKT_PEAK_SHIFT, PKT_BASE_SHIFT = 52, 40, 28
PKT_TS_MASK = (1 << 28) - 1
ROW_WIDE, ROW_REFERENCE = 0, 1       # mkid_list_photons' row word layouts
CAL_MAX_LINES = 3                    # mkid_spectrum_lines
CAL_FEW_LINES, CAL_FIT_FAILED, CAL_BAD_SLOPE = 1, 2, 16   # status bits; CAL_FIT_FAILED << p for line p
CUBE_ENERGY, CUBE_WAVELENGTH = 0, 1  # mkid_energy_cube's modes
LOOP_NPAR = 10                       # mkid_fit_loops
LOOP_NONFINITE, LOOP_FLAT, LOOP_NO_FIT, LOOP_MAX_ITER = 1, 2, 4, 8   # its status bits
MAG_NPAR = 6                         # mkid_fit_mags (its status bits are the LOOP_* ones)
WELCH_STRIP, WELCH_LDS_MAX_N, WELCH_MAX_N = 32, 4096, 262144         # mkid_welch_psd
IQN_NONFINITE, IQN_BAD_RAD, IQN_BAD_Q = 1, 2, 4                      # mkid_iq_noise's status bits


class MkidError(RuntimeError):
    """Raised on a negative MKID_E_* return code (katcp raises RuntimeError too:
    pulse_triggering_v2.py:177-179 catches it)."""

    def __init__(self, code, msg):
        super().__init__('%s (code %d)' % (msg, code))
        self.code = code


class Cfg(ctypes.Structure):
    _fields_ = [('n_channels', ctypes.c_int32), ('fft_len', ctypes.c_int32),
                ('pfb_taps', ctypes.c_int32), ('fir_taps', ctypes.c_int32),
                ('dds_entries', ctypes.c_int32), ('dead_time', ctypes.c_int32),
                ('max_events_per_ch', ctypes.c_int32), ('front', ctypes.c_int32),
                ('max_chunk', ctypes.c_int64), ('sample_rate', ctypes.c_double)]


REPLAY_ROLLING, REPLAY_BLOCK = 0, 1


class ReplayCfg(ctypes.Structure):
    _fields_ = [('mode', ctypes.c_int32), ('length', ctypes.c_int32), ('start', ctypes.c_int32),
                ('need', ctypes.c_int32), ('skip', ctypes.c_int32), ('wrap_negative', ctypes.c_int32),
                ('threshold_deg', ctypes.c_double)]


class TemplateInfo(ctypes.Structure):
    _fields_ = [('count', ctypes.c_double), ('count1', ctypes.c_double), ('pm', ctypes.c_double),
                ('pdev', ctypes.c_double), ('flag', ctypes.c_int32), ('pstart', ctypes.c_int32)]


class BankCfg(ctypes.Structure):
    _fields_ = [('n_channels', ctypes.c_int32), ('max_per_ch', ctypes.c_int32), ('length', ctypes.c_int32),
                ('min_records', ctypes.c_int32), ('pre', ctypes.c_int32), ('ncoeff', ctypes.c_int32),
                ('ready_stride', ctypes.c_int32), ('group', ctypes.c_int32), ('sign', ctypes.c_float)]


class BankResult(ctypes.Structure):
    _fields_ = [('count', ctypes.c_double), ('count1', ctypes.c_double), ('pm', ctypes.c_double),
                ('pdev', ctypes.c_double), ('flag', ctypes.c_int32), ('pstart', ctypes.c_int32),
                ('status', ctypes.c_int32), ('ready', ctypes.c_int32)]


class ThrStats(ctypes.Structure):
    """mkid_thr_stats: the median and 5 % edges behind a channel's threshold and its raw range."""
    _fields_ = [('med', ctypes.c_double), ('p05', ctypes.c_double), ('lo', ctypes.c_int32), ('hi', ctypes.c_int32)]


class LineFit(ctypes.Structure):
    """mkid_line_fit: one laser line of one channel's pulse-height spectrum."""
    _fields_ = [('bin', ctypes.c_int32), ('nfit', ctypes.c_int32), ('peak_s', ctypes.c_int64),
                ('counts', ctypes.c_int64), ('mu', ctypes.c_double), ('sigma', ctypes.c_double),
                ('amp', ctypes.c_double)]


class EnergyCal(ctypes.Structure):
    """mkid_energy_cal: a channel's height -> energy polynomial, resolving powers and status."""
    _fields_ = [('c', ctypes.c_double * 3), ('r', ctypes.c_double * 3), ('n_found', ctypes.c_int32),
                ('status', ctypes.c_int32)]


class LoopFit(ctypes.Structure):
    """mkid_loop_fit: one channel's fitted resonator loop."""
    _fields_ = [('p', ctypes.c_double * 10), ('chisq', ctypes.c_double), ('qc', ctypes.c_double),
                ('qi', ctypes.c_double), ('dipdb', ctypes.c_double), ('cidx', ctypes.c_int32),
                ('low', ctypes.c_int32), ('high', ctypes.c_int32), ('n', ctypes.c_int32),
                ('best_start', ctypes.c_int32), ('evals', ctypes.c_int32), ('status', ctypes.c_int32),
                ('pad', ctypes.c_int32)]


class MagFit(ctypes.Structure):
    """mkid_mag_fit: one channel's fitted resonator magnitude."""
    _fields_ = [('p', ctypes.c_double * 6), ('chisq', ctypes.c_double), ('norm', ctypes.c_double),
                ('cidx', ctypes.c_int32), ('best_start', ctypes.c_int32), ('evals', ctypes.c_int32),
                ('status', ctypes.c_int32)]


class IqNoiseCfg(ctypes.Structure):
    """mkid_iqnoise_cfg: the two resolutions, the stitch, the fn1k line and the scaling of mkid_iq_noise."""
    _fields_ = [('nfft_low', ctypes.c_int32), ('nfft_high', ctypes.c_int32), ('k_join', ctypes.c_int32),
                ('fit_first', ctypes.c_int32), ('fit_count', ctypes.c_int32), ('group', ctypes.c_int32),
                ('samprate', ctypes.c_double), ('f_eval', ctypes.c_double), ('gain', ctypes.c_double),
                ('full_scale', ctypes.c_double)]


class IqNoiseResult(ctypes.Structure):
    """mkid_iqnoise_result: one channel's means, rotation, radius, fn1k, exact sums and status."""
    _fields_ = [('mean_i', ctypes.c_double), ('mean_q', ctypes.c_double), ('resang', ctypes.c_double),
                ('rad', ctypes.c_double), ('fn1k', ctypes.c_double), ('sum_i', ctypes.c_int64),
                ('sum_q', ctypes.c_int64), ('nseg_low', ctypes.c_int32), ('nseg_high', ctypes.c_int32),
                ('status', ctypes.c_int32), ('pad', ctypes.c_int32)]


LINE_FIT_DTYPE = [('bin', '<i4'), ('nfit', '<i4'), ('peak_s', '<i8'), ('counts', '<i8'), ('mu', '<f8'),
                  ('sigma', '<f8'), ('amp', '<f8')]
ENERGY_CAL_DTYPE = [('c', '<f8', (3,)), ('r', '<f8', (3,)), ('n_found', '<i4'), ('status', '<i4')]
LOOP_FIT_DTYPE = [('p', '<f8', (10,)), ('chisq', '<f8'), ('qc', '<f8'), ('qi', '<f8'), ('dipdb', '<f8'), ('cidx', '<i4'),
                  ('low', '<i4'), ('high', '<i4'), ('n', '<i4'), ('best_start', '<i4'), ('evals', '<i4'),
                  ('status', '<i4'), ('pad', '<i4')]
MAG_FIT_DTYPE = [('p', '<f8', (6,)), ('chisq', '<f8'), ('norm', '<f8'), ('cidx', '<i4'), ('best_start', '<i4'),
                 ('evals', '<i4'), ('status', '<i4')]
IQ_NOISE_DTYPE = [('mean_i', '<f8'), ('mean_q', '<f8'), ('resang', '<f8'), ('rad', '<f8'), ('fn1k', '<f8'),
                  ('sum_i', '<i8'), ('sum_q', '<i8'), ('nseg_low', '<i4'), ('nseg_high', '<i4'), ('status', '<i4'),
                  ('pad', '<i4')]

BANK_USED, BANK_FEW_RECORDS, BANK_NONE_PASS1, BANK_NONE_PASS2 = range(4)


class SynthTone(ctypes.Structure):
    _fields_ = [('amp', ctypes.c_float), ('phase0', ctypes.c_float),
                ('freq_index', ctypes.c_int32), ('pad', ctypes.c_int32)]


class Pulse(ctypes.Structure):
    _fields_ = [('start', ctypes.c_int64), ('tone', ctypes.c_int32), ('amp_rad', ctypes.c_float)]


P = ctypes.c_void_p
I32, I64 = ctypes.c_int32, ctypes.c_int64
_SIGS = {
    'mkid_default_cfg': [P, I32],
    'mkid_create': [P, I32, P],
    'mkid_destroy': [P],
    'mkid_get_cfg': [P, P],
    'mkid_set_stream': [P, P],
    'mkid_set_pfb': [P, P, I32],
    'mkid_pfb_effective_taps': [P, I32, I32, P, P],
    'mkid_slot_order': [P, I32, P],
    'mkid_set_bins': [P, P, I32],
    'mkid_set_dds': [P, P, P, I32],
    'mkid_set_lpf': [P, P, I32],
    'mkid_set_fir': [P, P, I32, I32],
    'mkid_set_centers': [P, P, P, I32],
    'mkid_set_thresholds': [P, P, I32],
    'mkid_set_baseline': [P, I32, I32, I32, I32, I32],
    'mkid_set_rearm': [P, I32],
    'mkid_reset_stream': [P],
    'mkid_process': [P, P, I64, P, P, I64, P],
    'mkid_process_device': [P, P, I64, P, P, I64, P],
    'mkid_trigger_phase': [P, P, I64, P, I64, P],
    'mkid_last_raw_phase': [P, P, P],
    'mkid_read_raw_phase': [P, P, I64, P],
    'mkid_set_iq_tap': [P, I32],
    'mkid_read_iq_tap': [P, P, I64, P],
    'mkid_set_accumulator': [P, I32],
    'mkid_avg_iq': [P, P, P],
    'mkid_trigger_reruns': [P, P],
    'mkid_pack_reference': [P, I64, P],
    'mkid_set_timing': [P, I32],
    'mkid_set_timing_mask': [P, ctypes.c_uint32],
    'mkid_get_timing': [P, I32, P, P],
    'mkid_replay_trigger': [P, P, I64, I64, I32, P, P, I32, P],
    'mkid_make_template': [P, P, P, I64, P, P, P],
    'mkid_optimal_filter': [P, P, P, I32, I32, P],
    'mkid_bank_filters': [P, P, P, P, P, P, P, P, P],
    'mkid_set_pulse_filter': [P, P, I32, I32, I32],
    'mkid_pulse_heights': [P, P, I64, I64, P, I64, P],
    'mkid_pulse_heights_counted': [P, P, I64, I64, P, P, I64, P],
    'mkid_set_pulse_filter_device': [P, P, I32, I32, I32],
    'mkid_set_pulse_fit': [P, I32, I32],
    'mkid_pulse_fit': [P, P, I64, I64, P, I64, P, P, P, P],
    'mkid_pulse_fit_counted': [P, P, I64, I64, P, P, I64, P, P, P, P],
    'mkid_pulse_fit_host': [P, I64, I32, I64, P, I64, P, I32, I32, I32, I32, P, P, P, P],
    'mkid_count_photons': [P, P, I64, I64, I32, P, P],
    'mkid_count_photons_counted': [P, P, P, I64, I64, I32, P, P],
    'mkid_height_spectra': [P, P, P, I64, I64, I64, P, P, I32, P, P, I64, P],
    'mkid_height_spectra_counted': [P, P, P, P, I64, I64, I64, P, P, I32, P, P, I64, P],
    'mkid_concat_packets': [P, P, P, I64, P, P, I64, P, I64, P],
    'mkid_count_photons_host': [P, I64, I64, I32, ctypes.c_double, I32, I32, P, P],
    'mkid_height_spectra_host': [P, P, I64, I64, I64, I32, P, P, I32, P, P, I64, P],
    'mkid_list_photons': [P, P, I64, I64, I32, I32, I32, P, P, P, P, P],
    'mkid_list_photons_counted': [P, P, P, I64, I64, I32, I32, I32, P, P, P, P, P],
    'mkid_fill_photon_heights': [P, P, P, P, I64, I64, I64, I32, I32, P, P, P, P, P],
    'mkid_fill_photon_heights_counted': [P, P, P, P, P, I64, I64, I64, I32, I32, P, P, P, P, P],
    'mkid_list_photons_host': [P, I64, I64, I32, ctypes.c_double, I32, I32, I32, I32, P, P, P, P, P],
    'mkid_fill_photon_heights_host': [P, P, P, I64, I64, I64, I32, ctypes.c_double, I32, I32, I32, P, P, P, P, P],
    'mkid_list_photons_ring': [P, P, I64, I64, I64, I32, I64, I32, I32, P, P, P, P, P],
    'mkid_list_photons_ring_counted': [P, P, P, I64, I64, I64, I32, I64, I32, I32, P, P, P, P, P],
    'mkid_fill_photon_heights_ring': [P, P, P, P, I64, I64, I64, I64, I32, I64, I32, P, P, P, P, P],
    'mkid_fill_photon_heights_ring_counted': [P, P, P, P, P, I64, I64, I64, I64, I32, I64, I32, P, P, P, P, P],
    'mkid_pack_second': [P, I64, I32, I32, P, P, P, P, P, I64, P, P, P, P, P, P, P],
    'mkid_clear_second': [P, I64, I32, I32, P, P, P],
    'mkid_list_photons_ring_host': [P, I64, I64, I32, ctypes.c_double, I32, I64, I32, I64, I32, I32, P, P, P, P, P],
    'mkid_fill_photon_heights_ring_host': [P, P, P, I64, I64, I64, I32, ctypes.c_double, I32, I64, I32, I64, I32, P, P,
                                           P, P, P],
    'mkid_pack_second_host': [I64, I32, I32, I32, P, P, P, P, P, I64, P, P, P, P, P, P, P],
    'mkid_clear_second_host': [I64, I32, I32, I32, P, P, P],
    'mkid_spectrum_lines': [P, P, P, P, I32, I32, I32, P, I32, I32, I64, I32, P, P, P],
    'mkid_spectrum_lines_host': [P, P, P, I32, I32, I32, P, I32, I32, I64, I32, P, P, P],
    'mkid_energy_cube': [P, P, P, I64, I64, I64, P, I32, ctypes.c_float, ctypes.c_float, ctypes.c_float, I32, P, P],
    'mkid_energy_cube_counted': [P, P, P, P, I64, I64, I64, P, I32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                 I32, P, P],
    'mkid_energy_cube_host': [P, P, I64, I64, I64, I32, P, I32, ctypes.c_float, ctypes.c_float, ctypes.c_float, I32,
                              P, P],
    'mkid_fit_loops': [P, P, P, P, P, P, P, P, I32, I32, I32, I32, ctypes.c_double, P, P],
    'mkid_fit_loops_host': [P, P, P, P, P, P, P, I32, I32, I32, I32, ctypes.c_double, P, P],
    'mkid_fit_mags': [P, P, P, P, P, I32, I32, I32, I32, ctypes.c_double, P, P, P],
    'mkid_fit_mags_host': [P, P, P, P, I32, I32, I32, I32, ctypes.c_double, P, P, P],
    'mkid_welch_psd': [P, P, P, I64, I64, I32, I32, ctypes.c_double, I32, P, P],
    'mkid_welch_psd_host': [P, P, I64, I64, I32, I32, ctypes.c_double, I32, P, P],
    'mkid_iq_noise': [P, P, P, I64, I64, I32, P, P, P, P, P, P, P, P, P],
    'mkid_iq_noise_host': [P, P, I64, I64, I32, P, P, P, P, P, P, P, P, P],
    'mkid_iq_noise_freqs': [P, P],
    'mkid_set_capture': [P, I32, I32, I32],
    'mkid_capture_pulses': [P, P, I64, I64, P, I64, P, P, P],
    'mkid_capture_pulses_counted': [P, P, I64, I64, P, P, I64, P, P, P],
    'mkid_phase_thresholds': [P, P, I64, I64, I32, ctypes.c_double, P, P],
    'mkid_phase_thresholds_host': [P, I64, I64, I32, ctypes.c_double, P, P],
    'mkid_phase_thresholds_block_rows': [P, I64, I64, I32, I32, P],
    'mkid_phase_noise_spectra': [P, P, I64, I64, I32, I32, ctypes.c_double, ctypes.c_double, P],
    'mkid_phase_noise_spectra_host': [P, I64, I64, I32, I32, ctypes.c_double, ctypes.c_double, P],
    'mkid_stream_copy': [P, P, P, I64],
    'mkid_synth_adc': [P, P, I64, I64, P, P, P, I64, ctypes.c_float, ctypes.c_float, I32,
                       ctypes.c_float, ctypes.c_uint32],
}
# every symbol include/mkidgpu.h declares (tests/test_abi.py checks the header against this)
EXPORTS = sorted(list(_SIGS) + ['mkid_last_error', 'mkid_global_error', 'mkid_kernel_name'])

_lib = None


def load(path=None):
    """Load the in-tree HIP library; raise if it was not built. `path` loads a build variant
    (tools/kbench.py) as a separate library instance."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lp = path or LIB_PATH
    if not os.path.exists(lp):
        raise ImportError('libmkidgpu.so not built at %s: run __graft_entry__.build() '
                          '(make -C mkids_sdr_amd/csrc); there is no CPU fallback' % lp)
    L = ctypes.CDLL(lp)
    for name, args in _SIGS.items():
        if path is not None and not hasattr(L, name):
            continue  # an older build variant (tools/kbench.py A/B) may predate a symbol
        f = getattr(L, name)
        f.argtypes = args
        f.restype = ctypes.c_int
    for name in ('mkid_last_error',):
        getattr(L, name).argtypes = [P]
        getattr(L, name).restype = ctypes.c_char_p
    L.mkid_global_error.argtypes = []
    L.mkid_global_error.restype = ctypes.c_char_p
    L.mkid_kernel_name.argtypes = [I32]
    L.mkid_kernel_name.restype = ctypes.c_char_p
    if path is None:
        _lib = L
    return L


def check(rc, ctx=None):
    if rc != MKID_OK:
        L = load()
        msg = (L.mkid_last_error(ctx) if ctx else L.mkid_global_error()) or b''
        raise MkidError(rc, msg.decode(errors='replace'))
    return rc
