// C ABI of libmkidgpu.so (include/mkidgpu.h): the observing products after the heights — the
// per-second count image, the per-channel pulse-height spectra with the list of packets that still
// wait for their height, joining two counted lists, the per-pixel, per-second photon rows and the
// heights filled into them, their ring forms, a settled second packed out of its slot and the slot
// cleared, the energy cube, and the host twins of all but the join. The rules are obs_common.h (the
// cube's: wavecal_common.h); the kernels k_observe.hip, k_photons.hip, k_pack.hip and k_wavecal.hip.
#include "mkid_ctx.h"
#include "obs_common.h"
#include "wavecal_common.h"

using namespace mkid;

extern "C" {

static int count_photons(mkid_ctx* c, const uint64_t* d_events, const int64_t* d_n, int64_t n, int64_t j0,
                         int32_t n_seconds, int32_t* d_image, int64_t* d_outside) {
    if (!c || !d_image || !d_outside || (n > 0 && !d_events)) return MKID_E_ARG;
    if (n < 0 || !obs::j0_ok(j0, c->N)) FAIL(c, MKID_E_ARG, "count photons: negative n / j0, or j0 N past int64");
    if (!obs::seconds_ok(n_seconds)) FAIL(c, MKID_E_ARG, "count photons: need 1 <= n_seconds <= 2^20");
    if (!obs::fs_ok(c->cfg.sample_rate))
        FAIL(c, MKID_E_ARG, "count photons: the sample rate must be a positive integer number of samples per second");
    HIPCHK(c, hipSetDevice(c->device));
    const ObsCountArgs a{d_events, d_n, d_image, d_outside, n, j0, c->N, (int64_t)c->cfg.sample_rate,
                         c->C, n_seconds, c->ncu, 0};
    HIPCHK(c, launch_count_photons(a, c->stream));
    return MKID_OK;
}

int mkid_count_photons(mkid_ctx* c, const uint64_t* d_events, int64_t n, int64_t j0, int32_t n_seconds,
                       int32_t* d_image, int64_t* d_outside) {
    return count_photons(c, d_events, nullptr, n, j0, n_seconds, d_image, d_outside);
}

int mkid_count_photons_counted(mkid_ctx* c, const uint64_t* d_events, const int64_t* d_count, int64_t cap, int64_t j0,
                               int32_t n_seconds, int32_t* d_image, int64_t* d_outside) {
    if (!d_count) return MKID_E_ARG;
    return count_photons(c, d_events, d_count, cap, j0, n_seconds, d_image, d_outside);
}

static int height_spectra(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const int64_t* d_n, int64_t n,
                          int64_t j0, int64_t j_defer, const float* d_lo, const float* d_inv, int32_t nbins,
                          int32_t* d_spectra, uint64_t* d_deferred, int64_t cap_def, int64_t* d_ndef) {
    if (!c) return MKID_E_ARG;
    if (!obs::spectra_args_ok(d_events, d_heights, n, j0, c->C, d_lo, d_inv, nbins, d_spectra, d_deferred, cap_def,
                              d_ndef))
        FAIL(c, MKID_E_ARG,
             "height spectra: need pointers, n, j0, cap_def >= 0, 1 <= nbins <= 16384, d_ndef with d_deferred");
    HIPCHK(c, hipSetDevice(c->device));
    if (d_deferred && !c->d_obs_count.get()) {   // first use: nothing enqueued reads them yet
        DevBuf<int32_t> cnt;
        DevBuf<int64_t> off;
        HIPCHK(c, cnt.alloc(kObsMaxBlocks));
        HIPCHK(c, off.alloc(kObsMaxBlocks));
        c->d_obs_count = std::move(cnt), c->d_obs_off = std::move(off);
    }
    ObsSpectraArgs a{};
    a.events = d_events, a.heights = d_heights, a.d_n = d_n, a.lo = d_lo, a.inv = d_inv, a.spectra = d_spectra;
    a.deferred = d_deferred, a.ndef = d_ndef, a.wg_count = c->d_obs_count.get(), a.wg_off = c->d_obs_off.get();
    a.n = n, a.j0 = j0, a.j_defer = j_defer, a.cap_def = cap_def, a.C = c->C, a.nbins = nbins;
    HIPCHK(c, launch_height_spectra(a, plan_spectra(n, nbins, c->obs_lds), c->stream));
    return MKID_OK;
}

int mkid_height_spectra(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, int64_t n, int64_t j0,
                        int64_t j_defer, const float* d_lo, const float* d_inv, int32_t nbins, int32_t* d_spectra,
                        uint64_t* d_deferred, int64_t cap_def, int64_t* d_ndef) {
    return height_spectra(c, d_events, d_heights, nullptr, n, j0, j_defer, d_lo, d_inv, nbins, d_spectra, d_deferred,
                          cap_def, d_ndef);
}

int mkid_height_spectra_counted(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const int64_t* d_count,
                                int64_t cap, int64_t j0, int64_t j_defer, const float* d_lo, const float* d_inv,
                                int32_t nbins, int32_t* d_spectra, uint64_t* d_deferred, int64_t cap_def,
                                int64_t* d_ndef) {
    if (!d_count) return MKID_E_ARG;
    return height_spectra(c, d_events, d_heights, d_count, cap, j0, j_defer, d_lo, d_inv, nbins, d_spectra, d_deferred,
                          cap_def, d_ndef);
}

int mkid_concat_packets(mkid_ctx* c, const uint64_t* d_a, const int64_t* d_na, int64_t cap_a, const uint64_t* d_b,
                        const int64_t* d_nb, int64_t cap_b, uint64_t* d_out, int64_t cap_out, int64_t* d_nout) {
    if (!c || !d_na || !d_nb || !d_nout) return MKID_E_ARG;
    if (cap_a < 0 || cap_b < 0 || cap_out < 0) FAIL(c, MKID_E_ARG, "concat packets: negative capacity");
    if ((cap_a > 0 && !d_a) || (cap_b > 0 && !d_b) || (cap_out > 0 && !d_out))
        FAIL(c, MKID_E_ARG, "concat packets: a list with a capacity needs a pointer");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_concat_packets(d_a, d_na, cap_a, d_b, d_nb, cap_b, d_out, cap_out, d_nout, c->ncu, c->stream));
    return MKID_OK;
}

// The plain forms (w == nullptr) are the ring forms over the whole window obs::whole(n_seconds), with
// an argument check and a message of their own. For that window obs::ring_cell gives neither kEarly
// (no second is below sec0 = 0) nor kOverrun (sec < sec_end = n_slots is inside the slots), so the
// kernels touch only outside[0] and outside[1] of the plain forms' int64 [2].
static int list_photons(mkid_ctx* c, const uint64_t* d_events, const int64_t* d_n, int64_t n, int64_t j0,
                        int32_t n_seconds, const obs::Window* w, int32_t K, int32_t layout, int32_t* d_image,
                        int64_t* d_outside, uint64_t* d_words, int64_t* d_stamps, int64_t* d_dropped) {
    if (!c) return MKID_E_ARG;
    if (!w && !obs::list_args_ok(d_events, n, j0, c->N, c->cfg.sample_rate, c->C, n_seconds, K, layout, d_image, d_outside,
                                 d_words, d_stamps, d_dropped))
        FAIL(c, MKID_E_ARG,
             "list photons: need pointers, n, j0 >= 0 (j0 N inside int64), 1 <= n_seconds <= 2^20, 1 <= K <= 65536, "
             "a known layout (REFERENCE: C <= 254), an integer sample rate <= 2^43");
    if (w && !obs::list_ring_args_ok(d_events, n, j0, c->N, c->cfg.sample_rate, c->C, *w, K, layout, d_image, d_outside,
                                     d_words, d_stamps, d_dropped))
        FAIL(c, MKID_E_ARG,
             "list photons ring: need pointers, n, j0 >= 0 (j0 N inside int64), 1 <= n_slots <= 2^20, "
             "0 <= sec0 <= sec_end ((sec_end + 1) sample_rate inside int64), 1 <= K <= 65536, a known layout "
             "(REFERENCE: C <= 254), an integer sample rate <= 2^43");
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return MKID_OK;
    if (int rc = c->phws.reserve(c, photon_ws_bytes(n))) return rc;
    const obs::Window win = w ? *w : obs::whole(n_seconds);   // whole: outside[2] and [3] are never reached (above)
    PhotonArgs a{};
    a.events = d_events, a.d_n = d_n, a.image = d_image, a.outside = d_outside, a.words = d_words, a.stamps = d_stamps;
    a.dropped = d_dropped, a.n = n, a.j0 = j0, a.N = c->N, a.fs = (int64_t)c->cfg.sample_rate;
    a.C = c->C, a.n_slots = win.n_slots, a.K = K, a.layout = layout, a.sec0 = win.sec0, a.sec_end = win.sec_end;
    photon_ws_carve(a, c->phws.get());
    HIPCHK(c, launch_list_photons(a, c->stream));
    return MKID_OK;
}

int mkid_list_photons(mkid_ctx* c, const uint64_t* d_events, int64_t n, int64_t j0, int32_t n_seconds, int32_t K,
                      int32_t layout, int32_t* d_image, int64_t* d_outside, uint64_t* d_words, int64_t* d_stamps,
                      int64_t* d_dropped) {
    return list_photons(c, d_events, nullptr, n, j0, n_seconds, nullptr, K, layout, d_image, d_outside, d_words,
                        d_stamps, d_dropped);
}

int mkid_list_photons_counted(mkid_ctx* c, const uint64_t* d_events, const int64_t* d_count, int64_t cap, int64_t j0,
                              int32_t n_seconds, int32_t K, int32_t layout, int32_t* d_image, int64_t* d_outside,
                              uint64_t* d_words, int64_t* d_stamps, int64_t* d_dropped) {
    if (!d_count) return MKID_E_ARG;
    return list_photons(c, d_events, d_count, cap, j0, n_seconds, nullptr, K, layout, d_image, d_outside, d_words,
                        d_stamps, d_dropped);
}

int mkid_list_photons_ring(mkid_ctx* c, const uint64_t* d_events, int64_t n, int64_t j0, int64_t sec0, int32_t n_slots,
                           int64_t sec_end, int32_t K, int32_t layout, int32_t* d_image, int64_t* d_outside,
                           uint64_t* d_words, int64_t* d_stamps, int64_t* d_dropped) {
    const obs::Window w{sec0, sec_end, n_slots};
    return list_photons(c, d_events, nullptr, n, j0, 0, &w, K, layout, d_image, d_outside, d_words, d_stamps, d_dropped);
}

int mkid_list_photons_ring_counted(mkid_ctx* c, const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                                   int64_t j0, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K, int32_t layout,
                                   int32_t* d_image, int64_t* d_outside, uint64_t* d_words, int64_t* d_stamps,
                                   int64_t* d_dropped) {
    if (!d_count) return MKID_E_ARG;
    const obs::Window w{sec0, sec_end, n_slots};
    return list_photons(c, d_events, d_count, cap, j0, 0, &w, K, layout, d_image, d_outside, d_words, d_stamps,
                        d_dropped);
}

static int fill_photon_heights(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const float* d_dt,
                               const int64_t* d_n, int64_t n, int64_t j0, int64_t j_defer, int32_t n_seconds,
                               const obs::Window* w, int32_t K, const int32_t* d_image, const int64_t* d_stamps,
                               float* d_row_height, float* d_row_dt, int64_t* d_fill) {
    if (!c) return MKID_E_ARG;
    if (!w && !obs::fill_args_ok(d_events, d_heights, n, j0, c->N, c->cfg.sample_rate, c->C, n_seconds, K, d_image,
                                 d_stamps, d_row_height, d_fill))
        FAIL(c, MKID_E_ARG,
             "fill photon heights: need pointers, n, j0 >= 0 (j0 N inside int64), 1 <= n_seconds <= 2^20, "
             "1 <= K <= 65536, an integer sample rate <= 2^43");
    if (w && !obs::fill_ring_args_ok(d_events, d_heights, n, j0, c->N, c->cfg.sample_rate, c->C, *w, K, d_image, d_stamps,
                                     d_row_height, d_fill))
        FAIL(c, MKID_E_ARG,
             "fill photon heights ring: need pointers, n, j0 >= 0 (j0 N inside int64), 1 <= n_slots <= 2^20, "
             "0 <= sec0 <= sec_end ((sec_end + 1) sample_rate inside int64), 1 <= K <= 65536, an integer sample rate "
             "<= 2^43");
    HIPCHK(c, hipSetDevice(c->device));
    const obs::Window win = w ? *w : obs::whole(n_seconds);   // outside is not written: see list_photons
    PhotonFillArgs a{};
    a.events = d_events, a.heights = d_heights, a.dt = d_dt, a.d_n = d_n, a.image = d_image, a.stamps = d_stamps;
    a.row_height = d_row_height, a.row_dt = d_row_dt, a.fill = d_fill;
    a.n = n, a.j0 = j0, a.j_defer = j_defer, a.N = c->N, a.fs = (int64_t)c->cfg.sample_rate;
    a.C = c->C, a.n_slots = win.n_slots, a.K = K, a.ncu = c->ncu, a.sec0 = win.sec0, a.sec_end = win.sec_end;
    HIPCHK(c, launch_fill_photon_heights(a, c->stream));
    return MKID_OK;
}

int mkid_fill_photon_heights(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const float* d_dt, int64_t n,
                             int64_t j0, int64_t j_defer, int32_t n_seconds, int32_t K, const int32_t* d_image,
                             const int64_t* d_stamps, float* d_row_height, float* d_row_dt, int64_t* d_fill) {
    return fill_photon_heights(c, d_events, d_heights, d_dt, nullptr, n, j0, j_defer, n_seconds, nullptr, K, d_image,
                               d_stamps, d_row_height, d_row_dt, d_fill);
}

int mkid_fill_photon_heights_counted(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const float* d_dt,
                                     const int64_t* d_count, int64_t cap, int64_t j0, int64_t j_defer, int32_t n_seconds,
                                     int32_t K, const int32_t* d_image, const int64_t* d_stamps, float* d_row_height,
                                     float* d_row_dt, int64_t* d_fill) {
    if (!d_count) return MKID_E_ARG;
    return fill_photon_heights(c, d_events, d_heights, d_dt, d_count, cap, j0, j_defer, n_seconds, nullptr, K, d_image,
                               d_stamps, d_row_height, d_row_dt, d_fill);
}

int mkid_fill_photon_heights_ring(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const float* d_dt,
                                  int64_t n, int64_t j0, int64_t j_defer, int64_t sec0, int32_t n_slots, int64_t sec_end,
                                  int32_t K, const int32_t* d_image, const int64_t* d_stamps, float* d_row_height,
                                  float* d_row_dt, int64_t* d_fill) {
    const obs::Window w{sec0, sec_end, n_slots};
    return fill_photon_heights(c, d_events, d_heights, d_dt, nullptr, n, j0, j_defer, 0, &w, K, d_image, d_stamps,
                               d_row_height, d_row_dt, d_fill);
}

int mkid_fill_photon_heights_ring_counted(mkid_ctx* c, const uint64_t* d_events, const float* d_heights,
                                          const float* d_dt, const int64_t* d_count, int64_t cap, int64_t j0,
                                          int64_t j_defer, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                          const int32_t* d_image, const int64_t* d_stamps, float* d_row_height,
                                          float* d_row_dt, int64_t* d_fill) {
    if (!d_count) return MKID_E_ARG;
    const obs::Window w{sec0, sec_end, n_slots};
    return fill_photon_heights(c, d_events, d_heights, d_dt, d_count, cap, j0, j_defer, 0, &w, K, d_image, d_stamps,
                               d_row_height, d_row_dt, d_fill);
}

int mkid_pack_second(mkid_ctx* c, int64_t sec, int32_t n_slots, int32_t K, const int32_t* d_image,
                     const uint64_t* d_words, const int64_t* d_stamps, const float* d_row_height, const float* d_row_dt,
                     int64_t cap_out, int32_t* d_counts, int64_t* d_offsets, uint64_t* d_out_words,
                     int64_t* d_out_stamps, float* d_out_height, float* d_out_dt, int64_t* d_total) {
    if (!c) return MKID_E_ARG;
    if (!obs::pack_args_ok(sec, n_slots, K, c->C, d_image, d_words, d_stamps, d_row_height, d_row_dt, cap_out, d_counts,
                           d_offsets, d_out_words, d_out_stamps, d_out_height, d_out_dt, d_total))
        FAIL(c, MKID_E_ARG,
             "pack second: need the tables, counts, offsets and total, sec >= 0, 1 <= n_slots <= 2^20, 1 <= K <= 65536, "
             "cap_out >= 0 (with it, out words and heights), d_stamps with out stamps, d_row_dt with out dt");
    HIPCHK(c, hipSetDevice(c->device));
    const PackArgs a{d_image,     d_words,      d_stamps,     d_row_height, d_row_dt, d_counts,
                     d_offsets,   d_out_words,  d_out_stamps, d_out_height, d_out_dt, d_total,
                     obs::slot_of(sec, n_slots) * c->C, cap_out, c->C, K};
    HIPCHK(c, launch_pack_second(a, c->stream));
    return MKID_OK;
}

int mkid_clear_second(mkid_ctx* c, int64_t sec, int32_t n_slots, int32_t K, int32_t* d_image, float* d_row_height,
                      float* d_row_dt) {
    if (!c) return MKID_E_ARG;
    if (!obs::clear_args_ok(sec, n_slots, K, c->C, d_image, d_row_height))
        FAIL(c, MKID_E_ARG, "clear second: need d_image and d_row_height, sec >= 0, 1 <= n_slots <= 2^20, 1 <= K <= 65536");
    HIPCHK(c, hipSetDevice(c->device));
    const ClearArgs a{d_image, d_row_height, d_row_dt, obs::slot_of(sec, n_slots) * c->C, c->C, K};
    HIPCHK(c, launch_clear_second(a, c->stream));
    return MKID_OK;
}

// ---- the energy cube (wavecal_common.h) -----------------------------------------------------------
static int energy_cube(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const int64_t* d_n, int64_t n,
                       int64_t j0, int64_t j_defer, const float* d_cal_f, int32_t mode, float hc, float vlo, float vinv,
                       int32_t nb, int32_t* d_cube, float* d_energy) {
    if (!c) return MKID_E_ARG;
    if (!wcal::cube_args_ok(d_events, d_heights, n, j0, c->C, d_cal_f, mode, nb, d_cube))
        FAIL(c, MKID_E_ARG, "energy cube: need pointers, n, j0 >= 0, a known mode, 1 <= nb <= 16384");
    HIPCHK(c, hipSetDevice(c->device));
    WcalCubeArgs a{};
    a.events = d_events, a.heights = d_heights, a.d_n = d_n, a.cal_f = d_cal_f, a.cube = d_cube, a.energy = d_energy;
    a.n = n, a.j0 = j0, a.j_defer = j_defer, a.C = c->C, a.nb = nb, a.mode = mode, a.ncu = c->ncu;
    a.hc = hc, a.vlo = vlo, a.vinv = vinv;
    HIPCHK(c, launch_energy_cube(a, c->stream));
    return MKID_OK;
}

int mkid_energy_cube(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, int64_t n, int64_t j0,
                     int64_t j_defer, const float* d_cal_f, int32_t mode, float hc, float vlo, float vinv, int32_t nb,
                     int32_t* d_cube, float* d_energy) {
    return energy_cube(c, d_events, d_heights, nullptr, n, j0, j_defer, d_cal_f, mode, hc, vlo, vinv, nb, d_cube,
                       d_energy);
}

int mkid_energy_cube_counted(mkid_ctx* c, const uint64_t* d_events, const float* d_heights, const int64_t* d_count,
                             int64_t cap, int64_t j0, int64_t j_defer, const float* d_cal_f, int32_t mode, float hc,
                             float vlo, float vinv, int32_t nb, int32_t* d_cube, float* d_energy) {
    if (!d_count) return MKID_E_ARG;
    return energy_cube(c, d_events, d_heights, d_count, cap, j0, j_defer, d_cal_f, mode, hc, vlo, vinv, nb, d_cube,
                       d_energy);
}

int mkid_energy_cube_host(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int64_t j_defer,
                          int32_t n_channels, const float* cal_f, int32_t mode, float hc, float vlo, float vinv,
                          int32_t nb, int32_t* cube, float* energy) {
    if (!wcal::cube_args_ok(events, heights, n, j0, n_channels, cal_f, mode, nb, cube)) return MKID_E_ARG;
    const wcal::CubeRule r{j0, j_defer, n_channels, nb, mode, hc, vlo, vinv};
    wcal::cube_host(events, heights, n, cal_f, r, cube, energy);
    return MKID_OK;
}

// The CPU statements of the device calls: the loops of obs_common.h.
int mkid_list_photons_host(const uint64_t* events, int64_t n, int64_t j0, int32_t fft_len, double sample_rate,
                           int32_t n_channels, int32_t n_seconds, int32_t K, int32_t layout, int32_t* image,
                           int64_t* outside, uint64_t* words, int64_t* stamps, int64_t* dropped) {
    if (!obs::list_args_ok(events, n, j0, fft_len, sample_rate, n_channels, n_seconds, K, layout, image, outside, words,
                           stamps, dropped))
        return MKID_E_ARG;
    obs::list_host(events, n, j0, fft_len, sample_rate, n_channels, n_seconds, K, layout, image, outside, words, stamps,
                   dropped);
    return MKID_OK;
}

int mkid_fill_photon_heights_host(const uint64_t* events, const float* heights, const float* dt, int64_t n, int64_t j0,
                                  int64_t j_defer, int32_t fft_len, double sample_rate, int32_t n_channels,
                                  int32_t n_seconds, int32_t K, const int32_t* image, const int64_t* stamps,
                                  float* row_height, float* row_dt, int64_t* fill) {
    if (!obs::fill_args_ok(events, heights, n, j0, fft_len, sample_rate, n_channels, n_seconds, K, image, stamps,
                           row_height, fill))
        return MKID_E_ARG;
    obs::fill_host(events, heights, dt, n, j0, j_defer, fft_len, sample_rate, n_channels, n_seconds, K, image, stamps,
                   row_height, row_dt, fill);
    return MKID_OK;
}

int mkid_list_photons_ring_host(const uint64_t* events, int64_t n, int64_t j0, int32_t fft_len, double sample_rate,
                                int32_t n_channels, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                int32_t layout, int32_t* image, int64_t* outside, uint64_t* words, int64_t* stamps,
                                int64_t* dropped) {
    const obs::Window w{sec0, sec_end, n_slots};
    if (!obs::list_ring_args_ok(events, n, j0, fft_len, sample_rate, n_channels, w, K, layout, image, outside, words,
                                stamps, dropped))
        return MKID_E_ARG;
    obs::list_ring_host(events, n, j0, fft_len, sample_rate, n_channels, w, K, layout, image, outside, words, stamps,
                        dropped);
    return MKID_OK;
}

int mkid_fill_photon_heights_ring_host(const uint64_t* events, const float* heights, const float* dt, int64_t n,
                                       int64_t j0, int64_t j_defer, int32_t fft_len, double sample_rate,
                                       int32_t n_channels, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                       const int32_t* image, const int64_t* stamps, float* row_height, float* row_dt,
                                       int64_t* fill) {
    const obs::Window w{sec0, sec_end, n_slots};
    if (!obs::fill_ring_args_ok(events, heights, n, j0, fft_len, sample_rate, n_channels, w, K, image, stamps, row_height,
                                fill))
        return MKID_E_ARG;
    obs::fill_ring_host(events, heights, dt, n, j0, j_defer, fft_len, sample_rate, n_channels, w, K, image, stamps,
                        row_height, row_dt, fill);
    return MKID_OK;
}

int mkid_pack_second_host(int64_t sec, int32_t n_slots, int32_t K, int32_t n_channels, const int32_t* image,
                          const uint64_t* words, const int64_t* stamps, const float* row_height, const float* row_dt,
                          int64_t cap_out, int32_t* counts, int64_t* offsets, uint64_t* out_words, int64_t* out_stamps,
                          float* out_height, float* out_dt, int64_t* total) {
    if (!obs::pack_args_ok(sec, n_slots, K, n_channels, image, words, stamps, row_height, row_dt, cap_out, counts, offsets,
                           out_words, out_stamps, out_height, out_dt, total))
        return MKID_E_ARG;
    obs::pack_host(sec, n_slots, K, n_channels, image, words, stamps, row_height, row_dt, cap_out, counts, offsets,
                   out_words, out_stamps, out_height, out_dt, total);
    return MKID_OK;
}

int mkid_clear_second_host(int64_t sec, int32_t n_slots, int32_t K, int32_t n_channels, int32_t* image,
                           float* row_height, float* row_dt) {
    if (!obs::clear_args_ok(sec, n_slots, K, n_channels, image, row_height)) return MKID_E_ARG;
    obs::clear_host(sec, n_slots, K, n_channels, image, row_height, row_dt);
    return MKID_OK;
}

int mkid_count_photons_host(const uint64_t* events, int64_t n, int64_t j0, int32_t fft_len, double sample_rate,
                            int32_t n_channels, int32_t n_seconds, int32_t* image, int64_t* outside) {
    if (!obs::count_args_ok(events, n, j0, fft_len, sample_rate, n_channels, n_seconds, image, outside))
        return MKID_E_ARG;
    obs::count_host(events, n, j0, fft_len, sample_rate, n_channels, n_seconds, image, outside);
    return MKID_OK;
}

int mkid_height_spectra_host(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int64_t j_defer,
                             int32_t n_channels, const float* lo, const float* inv, int32_t nbins, int32_t* spectra,
                             uint64_t* deferred, int64_t cap_def, int64_t* ndef) {
    if (!obs::spectra_args_ok(events, heights, n, j0, n_channels, lo, inv, nbins, spectra, deferred, cap_def, ndef))
        return MKID_E_ARG;
    obs::spectra_host(events, heights, n, j0, j_defer, n_channels, lo, inv, nbins, spectra, deferred, cap_def, ndef);
    return MKID_OK;
}

}  // extern "C"
