// C ABI of libmkidgpu.so (include/mkidgpu.h): context creation and teardown, configuration, timing and
// the host-only entry points. The streaming calls are in mkid_stream.hip, calibration in mkid_calib.hip.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "mkid_ctx.h"

using namespace mkid;

namespace {

// error text of a failed mkid_create (no context yet); per thread, so that contexts created
// concurrently from several host threads do not overwrite each other's message
thread_local std::string g_err;

// Default IQ low-pass: LUT/BlackmanFilter_250kHz.txt quantised as int(x*(2**11-1))
// (ROACH_Pulses.py:69, 88; importFIRcoeffs default ROACH_Pulses.py:1101).
const int16_t kBlackman250k[kFirTaps] = {0,   0,   3,   8,   17,  32,  53,  80,  111, 142, 172, 194, 206,
                                         206, 194, 172, 142, 111, 80,  53,  32,  17,  8,   3,   0,   0};

}  // namespace

static hipEvent_t get_event(mkid_ctx* c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void tstart(mkid_ctx* c, int k, KTime* kt, hipStream_t s) {
    kt->k = -1;
    if (!c->timing || !((c->timing_mask >> k) & 1u)) return;
    kt->a = get_event(c);
    kt->b = get_event(c);
    if (!kt->a || !kt->b) return;
    kt->k = k;
    (void)hipEventRecord(kt->a, s);
}

void tstop(mkid_ctx* c, KTime* kt, hipStream_t s) {
    if (kt->k < 0) return;
    (void)hipEventRecord(kt->b, s);
    c->pending.push_back(*kt);
}

int flush_timing(mkid_ctx* c) {
    for (auto& kt : c->pending) {
        HIPCHK(c, hipEventSynchronize(kt.b));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, kt.a, kt.b));
        c->tot_ms[kt.k] += ms;
        c->launches[kt.k] += 1;
        c->pool.push_back(kt.a);
        c->pool.push_back(kt.b);
    }
    c->pending.clear();
    return MKID_OK;
}

static void default_pfb(int N, int T, std::vector<float>& h) {
    const int L = T * N;
    std::vector<double> d(L);
    double s = 0;
    for (int n = 0; n < L; ++n) {
        const double x = (n - (L - 1) / 2.0) / N;
        const double sinc = x == 0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        d[n] = sinc * (0.54 - 0.46 * std::cos(2 * M_PI * n / (L - 1)));
        s += d[n];
    }
    h.resize(L);
    for (int n = 0; n < L; ++n) h[n] = (float)(d[n] / s);
}

// teardown: the context's members release what they own (mkid_ctx.h)
static void drop_ctx(mkid_ctx* c) {
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c;
}

static int upload_lo_folded(mkid_ctx* c);
static int upload_slot_order(mkid_ctx* c);
static int upload_centring(mkid_ctx* c);
static int upload_pfb(mkid_ctx* c, const float* coeffs);

extern "C" {

const char* mkid_global_error(void) { return g_err.c_str(); }

int mkid_default_cfg(mkid_cfg* cfg, int32_t n_channels) {
    if (!cfg || n_channels <= 0 || 65536 % n_channels != 0) return MKID_E_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_channels = n_channels;
    cfg->fft_len = 2 * n_channels;
    cfg->pfb_taps = kPfbTaps;
    cfg->fir_taps = kFirTaps;
    cfg->dds_entries = 65536 / n_channels;
    cfg->dead_time = 32;
    cfg->max_events_per_ch = 0;
    cfg->max_chunk = (int64_t)1 << 22;
    cfg->sample_rate = 512e6;
    return MKID_OK;
}

int mkid_create(const mkid_cfg* cfg, int32_t device, mkid_ctx** out) {
    if (!cfg || !out) { g_err = "null argument"; return MKID_E_ARG; }
    *out = nullptr;
    const int C = cfg->n_channels, N = cfg->fft_len;
    if (N != 2 * C || !channelize_supported(N)) { g_err = "unsupported geometry: need N = 2C, N in {128..4096}"; return MKID_E_ARG; }
    if (cfg->pfb_taps != kPfbTaps || cfg->fir_taps != kFirTaps) { g_err = "pfb_taps must be 4 and fir_taps 26"; return MKID_E_ARG; }
    const int P = cfg->dds_entries;
    if (P < 2 || (P & (P - 1)) != 0) { g_err = "dds_entries must be a power of two >= 2"; return MKID_E_ARG; }
    if (cfg->max_chunk < N || cfg->max_chunk % N != 0) { g_err = "max_chunk must be a positive multiple of N"; return MKID_E_ARG; }
    if (cfg->dead_time < 0) { g_err = "dead_time < 0"; return MKID_E_ARG; }
    if (cfg->front != MKID_FRONT_AUTO && cfg->front != MKID_FRONT_SPLIT) { g_err = "bad front mode"; return MKID_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device"; return MKID_E_NODEV; }
    if (device < 0 || device >= ndev) { g_err = "bad device index"; return MKID_E_ARG; }
    mkid_ctx* c = new (std::nothrow) mkid_ctx();
    if (!c) { g_err = "out of host memory"; return MKID_E_ARG; }
    c->cfg = *cfg;
    c->device = device;
    c->C = C; c->N = N; c->M = N / 2; c->T = kPfbTaps; c->P = P;
    c->fused = cfg->front == MKID_FRONT_AUTO && fused_supported(N);
    {
        const char* so = getenv("MKID_SLOT_ORDER");
        c->slot_order_on = !(so && atoi(so) == 0);
        if (const char* fl = getenv("MKID_FAULT_LAUNCH")) c->fault_launch = atoll(fl);
        if (const char* ol = getenv("MKID_OBS_LDS")) c->obs_lds = atoi(ol) != 0;
    }
    int64_t trig_slots = trigger_wave_slots(device);
    // tuning/test knob: pretend the GPU holds this many trigger waves (forces longer segments)
    if (const char* ev = getenv("MKID_TRIG_WAVE_SLOTS")) trig_slots = std::max<int64_t>(1, atoll(ev));
    int64_t svf_lanes = 0, svf_w = plan::kSvfW;
    {   // SVF segments: one per SIMD lane (4 SIMDs x 64 lanes per CU, round 6); test/tuning knobs
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0)
            ncu = 256;
        c->ncu = ncu;
        svf_lanes = (int64_t)ncu * 256;
        if (const char* ev = getenv("MKID_SVF_LANES")) svf_lanes = std::max<int64_t>(1, atoll(ev));
        if (const char* ev = getenv("MKID_SVF_WARMUP"))
            svf_w = std::max<int64_t>(1, atoll(ev) / kFirTaps) * kFirTaps;
    }
    if (const char* msg = plan::size_workspace(*cfg, trig_slots, svf_lanes, svf_w, c->ws)) {
        g_err = msg;
        delete c;
        return MKID_E_ARG;
    }
    const plan::Workspace& ws = c->ws;
    auto fail = [&](hipError_t e, const char* what) {
        g_err = std::string(what) + ": " + hipGetErrorString(e);
        drop_ctx(c);
        return MKID_E_HIP;
    };
    hipError_t e;
#define AL(p, ...) if ((e = c->p.alloc(__VA_ARGS__)) != hipSuccess) return fail(e, "hipMalloc " #p)
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
    c->stream = c->own;
    AL(d_pfb, (size_t)c->T * N);
    AL(d_pfbq, (size_t)N);
    AL(d_bins, C);
    AL(d_lo, (size_t)C * P);
    AL(d_fir, (size_t)C * kFirTaps);
    AL(d_ncen, C);
    AL(d_cor, C);
    AL(d_thr, C);
    AL(d_rearm, C);
    AL(xhist, c->fused ? front_hist_samples(N) : (int64_t)c->T * N - c->M, 4);
    AL(zhist, kLpfHist, (int64_t)C * 8);
    AL(rhist, kRawHist, (int64_t)C * 2);
    AL(d_tstate, C);
    if (!c->fused) AL(d_z, (size_t)ws.Kmax * C);
    AL(d_raw, (size_t)ws.Jmax * C);
    AL(d_iqtap, (size_t)ws.Jmax * 2);
    AL(d_ysum, (size_t)2 * C);
    AL(d_slots, (size_t)ws.slot_cap);
    AL(d_chcounts, (size_t)C * ws.nseg_max);
    AL(d_scan, (size_t)C * ws.nseg_max + 64);  // >= 3 int64 per compaction tile
    AL(d_sspec, (size_t)C * ws.nseg_max);
    AL(d_send, (size_t)C * ws.nseg_max);
    AL(d_scratch, (size_t)C * ws.scratch_cap);
    AL(d_reruns, C);
    AL(d_counts, 2);
    AL(d_slot_ch, C);
#undef AL
    // defaults: identity bins, unit LO, Blackman 250 kHz low-pass, zero matched filter (no
    // triggers), zero centres, thresholds off, EMA baseline alpha=41 gate=8192.
    std::vector<float> h;
    default_pfb(N, c->T, h);
    std::vector<int32_t> bins(C), thr(C, INT_MIN / 2);
    for (int i = 0; i < C; ++i) bins[i] = i;
    std::vector<float2> lo((size_t)C * P, make_float2(32767.f / 32768.f, 0.f));
    std::vector<int16_t> fir((size_t)C * kFirTaps, 0);
    for (int i = 0; i < kFirTaps; ++i) c->lpf.g[i] = kBlackman250k[i] / 2048.0f;
    c->h_thr = thr;
    c->h_ic.assign(C, 0.f);
    c->h_qc.assign(C, 0.f);
    c->acc_off.assign(2 * (size_t)C, 0.0);
    if ((e = hipMemcpy(c->d_bins.get(), bins.data(), C * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(c->d_thr.get(), thr.data(), C * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(c->d_rearm.get(), thr.data(), C * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(c->d_lo.get(), lo.data(), lo.size() * 8, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(c->d_fir.get(), fir.data(), fir.size() * 2, hipMemcpyHostToDevice)) != hipSuccess)
        return fail(e, "hipMemcpy defaults");
    c->h_lo = lo;
    c->h_bins = bins;
    *out = c;
    if (upload_pfb(c, h.data()) != MKID_OK || upload_slot_order(c) != MKID_OK || upload_centring(c) != MKID_OK ||
        mkid_reset_stream(c) != MKID_OK) {
        g_err = c->err;
        drop_ctx(c);
        *out = nullptr;
        return MKID_E_HIP;
    }
    return MKID_OK;
}

int mkid_destroy(mkid_ctx* c) {
    if (!c) return MKID_E_ARG;
    drop_ctx(c);
    return MKID_OK;
}

const char* mkid_last_error(const mkid_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }

int mkid_get_cfg(const mkid_ctx* c, mkid_cfg* out) {
    if (!c || !out) return MKID_E_ARG;
    *out = c->cfg;
    return MKID_OK;
}

int mkid_set_stream(mkid_ctx* c, void* s) {
    if (!c) return MKID_E_ARG;
    c->stream = s ? (hipStream_t)s : c->own;
    return MKID_OK;
}

static int upload_pfb(mkid_ctx* c, const float* coeffs) {
    const int T = c->T, N = c->N;
    std::vector<int16_t> hq;
    const int S = plan::quantize_pfb(coeffs, T, N, hq);
    std::vector<float> hf(hq.size());
    for (size_t i = 0; i < hq.size(); ++i) hf[i] = (float)std::ldexp((double)hq[i], -S);
    std::vector<uint2> hp(N);
    for (int p = 0; p < N; ++p) {
        auto u16 = [&](int t) { return (uint32_t)(uint16_t)hq[(size_t)t * N + p]; };
        hp[p] = make_uint2(u16(0) | (u16(1) << 16), u16(2) | (u16(3) << 16));
    }
    int r = upload(c, c->d_pfb.get(), hf.data(), hf.size() * 4);
    if (r) return r;
    r = upload(c, c->d_pfbq.get(), hp.data(), hp.size() * 8);
    if (r) return r;
    c->pfb_shift = S;
    return upload_lo_folded(c);  // the fused path folds 2^-S into the LO table
}

int mkid_pfb_effective_taps(const float* coeffs, int32_t T, int32_t N, float* out, int32_t* shift) {
    if (!coeffs || !out || T <= 0 || N <= 0) return MKID_E_ARG;
    std::vector<int16_t> hq;
    const int S = plan::quantize_pfb(coeffs, T, N, hq);
    for (size_t i = 0; i < hq.size(); ++i) out[i] = (float)std::ldexp((double)hq[i], -S);
    if (shift) *shift = S;
    return MKID_OK;
}

int mkid_set_pfb(mkid_ctx* c, const float* coeffs, int32_t n) {
    if (!c || !coeffs) return MKID_E_ARG;
    if (n != c->T * c->N) FAIL(c, MKID_E_ARG, "pfb coefficient count must be T*N");
    return upload_pfb(c, coeffs);
}

int mkid_set_bins(mkid_ctx* c, const int32_t* bins, int32_t n) {
    if (!c || !bins) return MKID_E_ARG;
    if (n != c->C) FAIL(c, MKID_E_ARG, "need one bin per channel");
    std::vector<int32_t> b(bins, bins + n);
    for (auto& v : b) v = ((v % c->N) + c->N) % c->N;
    int r = upload(c, c->d_bins.get(), b.data(), (size_t)n * 4);
    if (r) return r;
    c->h_bins = b;
    r = upload_slot_order(c);
    if (r) return r;
    return upload_lo_folded(c);
}

int mkid_set_dds(mkid_ctx* c, const int16_t* li, const int16_t* lq, int32_t P) {
    if (!c || !li || !lq) return MKID_E_ARG;
    if (P != c->P) FAIL(c, MKID_E_ARG, "entries_per_ch must equal cfg.dds_entries");
    // device layout [P][C] (input is [C][P]): one frame reads one contiguous row
    std::vector<float2> lo((size_t)c->C * P);
    for (int ch = 0; ch < c->C; ++ch)
        for (int p = 0; p < P; ++p) {
            const size_t i = (size_t)ch * P + p;
            lo[(size_t)p * c->C + ch] = make_float2(li[i] / 32768.f, -lq[i] / 32768.f);
        }
    c->h_lo = std::move(lo);
    return upload_lo_folded(c);
}

static int upload_slot_order(mkid_ctx* c) {
    std::vector<int16_t> so;
    if (c->slot_order_on) {
        plan::slot_order(c->h_bins, c->C, so);   // k_front3 select-slot order
    } else {
        so.resize(c->C);
        for (int i = 0; i < c->C; ++i) so[i] = (int16_t)i;
    }
    return upload(c, c->d_slot_ch.get(), so.data(), so.size() * 2);
}

int mkid_slot_order(const int32_t* bins, int32_t C, int16_t* out) {
    if (!bins || !out || C <= 0) return MKID_E_ARG;
    std::vector<int32_t> b(bins, bins + C);
    std::vector<int16_t> so;
    plan::slot_order(b, C, so);
    std::copy(so.begin(), so.end(), out);
    return MKID_OK;
}

// d_lo[p][c] = h_lo[p][c] * (-1)^(b_c (k+1)) for any frame k = p (mod P): odd bins flip the sign
// on even rows (P is even). The kernels then multiply by d_lo only.
static int upload_lo_folded(mkid_ctx* c) {
    std::vector<float2> lo = c->h_lo;
    // fused path: the PFB output is the integer h_q . x, so the 2^-S tap scale joins the LO
    const float sc = c->fused ? (float)std::ldexp(1.0, -c->pfb_shift) : 1.0f;
    for (int p = 0; p < c->P; ++p)
        for (int ch = 0; ch < c->C; ++ch) {
            float2& v = lo[(size_t)p * c->C + ch];
            const float sg = ((p & 1) == 0 && (c->h_bins[ch] & 1)) ? -sc : sc;
            v = make_float2(v.x * sg, v.y * sg);
        }
    return upload(c, c->d_lo.get(), lo.data(), lo.size() * 8);
}

int mkid_set_lpf(mkid_ctx* c, const int16_t* taps, int32_t n) {
    if (!c || !taps) return MKID_E_ARG;
    if (n != kFirTaps) FAIL(c, MKID_E_ARG, "low-pass must have 26 taps");
    for (int i = 0; i < n; ++i) c->lpf.g[i] = taps[i] / 2048.0f;
    return upload_centring(c);   // c' = c / G depends on the taps' sum G
}

// Centred low-pass constants (mkid_internal.h Centring): G = sum_i g_i (exact: g_i = k_i / 2^11),
// c' = fp32(c / G), r = fp32(G c' - c) evaluated in float64 (G c' is exact there: 16 x 24 bits), so
// y' + r = y - c up to the rounding of r (|r| ~ 2^-24 |c|). |G| < kCentringMinGain (taps with a
// small DC gain, all-zero taps): c' = 0, r = -c, the uncentred form — c' = c / G would grow as 1 / G
// and the low-pass accumulation's fp32 rounding with it.
static constexpr double kCentringMinGain = 0.25;
static int upload_centring(mkid_ctx* c) {
    double G = 0.0;
    for (int i = 0; i < kFirTaps; ++i) G += (double)c->lpf.g[i];
    const bool centred = std::fabs(G) >= kCentringMinGain;
    std::vector<float2> nc((size_t)c->C), cr((size_t)c->C);
    c->h_gc.assign(2 * (size_t)c->C, 0.0);
    for (int ch = 0; ch < c->C; ++ch) {
        const double ci = c->h_ic[ch], cq = c->h_qc[ch];
        const float pi = centred ? (float)(ci / G) : 0.f, pq = centred ? (float)(cq / G) : 0.f;
        nc[ch] = make_float2(-pi, -pq);
        cr[ch] = make_float2((float)(G * pi - ci), (float)(G * pq - cq));
        c->h_gc[2 * ch] = G * pi;
        c->h_gc[2 * ch + 1] = G * pq;
    }
    int r = upload(c, c->d_ncen.get(), nc.data(), nc.size() * 8);
    return r ? r : upload(c, c->d_cor.get(), cr.data(), cr.size() * 8);
}


int mkid_set_fir(mkid_ctx* c, const int16_t* taps, int32_t nch, int32_t nt) {
    if (!c || !taps) return MKID_E_ARG;
    if (nch != c->C || nt != kFirTaps) FAIL(c, MKID_E_ARG, "matched filter must be [C][26]");
    for (int64_t i = 0; i < (int64_t)nch * nt; ++i)
        if (taps[i] < -2048 || taps[i] > 2047) FAIL(c, MKID_E_ARG, "matched-filter tap outside 12-bit range");
    return upload(c, c->d_fir.get(), taps, (size_t)nch * nt * 2);
}

int mkid_set_centers(mkid_ctx* c, const float* ic, const float* qc, int32_t n) {
    if (!c || !ic || !qc) return MKID_E_ARG;
    if (n != c->C) FAIL(c, MKID_E_ARG, "need one centre per channel");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(ic[i]) || !std::isfinite(qc[i])) FAIL(c, MKID_E_ARG, "centres must be finite");
    c->h_ic.assign(ic, ic + n);
    c->h_qc.assign(qc, qc + n);
    return upload_centring(c);
}

// re-arm levels from the thresholds and the hysteresis fraction (plan::rearm_level)
static int upload_rearm(mkid_ctx* c) {
    std::vector<int32_t> lv(c->h_thr.size());
    for (size_t i = 0; i < lv.size(); ++i) lv[i] = plan::rearm_level(c->h_thr[i], c->rearm_q8);
    return upload(c, c->d_rearm.get(), lv.data(), lv.size() * 4);
}

int mkid_set_thresholds(mkid_ctx* c, const int32_t* thr, int32_t n) {
    if (!c || !thr) return MKID_E_ARG;
    if (n != c->C) FAIL(c, MKID_E_ARG, "need one threshold per channel");
    int r = upload(c, c->d_thr.get(), thr, (size_t)n * 4);
    if (r) return r;
    c->h_thr.assign(thr, thr + n);
    return upload_rearm(c);
}

int mkid_set_rearm(mkid_ctx* c, int32_t frac_q8) {
    if (!c) return MKID_E_ARG;
    if (frac_q8 < 0 || frac_q8 > 256) FAIL(c, MKID_E_ARG, "re-arm fraction must be 0..256 (/256)");
    c->rearm_q8 = frac_q8;
    return upload_rearm(c);
}

int mkid_set_baseline(mkid_ctx* c, int32_t mode, int32_t alpha, int32_t kf, int32_t kq, int32_t base_thr) {
    if (!c) return MKID_E_ARG;
    if (mode < MKID_BASE_NONE || mode > MKID_BASE_SVF) FAIL(c, MKID_E_ARG, "bad baseline mode");
    // Fix12_9; above 2.0 (1024) the EMA diverges and its int32 arithmetic overflows
    if (alpha < 0 || alpha > 1024) FAIL(c, MKID_E_ARG, "alpha must be Fix12_9 in 0..1024 (gain <= 2.0)");
    if (kf < 0 || kf >= (1 << 18) || kq < 0 || kq >= (1 << 18)) FAIL(c, MKID_E_ARG, "kf/kq must be Fix18_16");
    if (base_thr < 0 || base_thr > 65535) FAIL(c, MKID_E_ARG, "base_thr must be Fix16_13 (0..65535)");
    if (mode == MKID_BASE_SVF && !c->svf.ready()) {   // allocated on first use
        HIPCHK(c, hipSetDevice(c->device));
        if (c->svf.alloc(c->ws, c->C) != hipSuccess) FAIL(c, MKID_E_HIP, "hipMalloc of the SVF tables failed");
    }
    c->mode = mode; c->alpha = alpha; c->kf = kf; c->kq = kq; c->base_thr = base_thr;
    return MKID_OK;
}

int mkid_reset_stream(mkid_ctx* c) {
    if (!c) return MKID_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->xhist.get(), 0, c->xhist.bytes(), c->stream));
    HIPCHK(c, hipMemsetAsync(c->zhist.get(), 0, c->zhist.bytes(), c->stream));
    HIPCHK(c, hipMemsetAsync(c->rhist.get(), 0, c->rhist.bytes(), c->stream));
    {   // start-of-stream hold-off: DEAD for kHoldOff samples, no baseline (trig_common.h)
        std::vector<TrigState> st0((size_t)c->C, TrigState{0, 0, 2 /*ST_DEAD*/, kHoldOff, 0, 0, 0, 0, 0, 0});
        HIPCHK(c, hipMemcpyAsync(c->d_tstate.get(), st0.data(), st0.size() * sizeof(TrigState), hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->d_ysum.get(), 0, (size_t)c->C * 16, c->stream));   // avgIQ: sums restart
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->acc_rows = 0;
    std::fill(c->acc_off.begin(), c->acc_off.end(), 0.0);
    c->k0 = 0;
    c->j0 = 0;
    c->stream_kind = 0;
    c->last_J = 0;
    c->pcarry.drop();   // pulse-height phase history: a reset starts a new stream
    c->fcarry.drop();   // and the pulse fit's
    c->ccarry.drop();   // pulse capture: the next call starts a segment (rows and pending list forgotten)
    return MKID_OK;
}

int mkid_set_timing_mask(mkid_ctx* c, uint32_t mask) {
    if (!c) return MKID_E_ARG;
    if ((mask & ~((1u << MKID_K_COUNT) - 1u)) != 0) FAIL(c, MKID_E_ARG, "timing mask: an OR of MKID_TIMING_ONLY(k)");
    int r = flush_timing(c);
    if (r) return r;
    c->timing = mask != 0;
    c->timing_mask = mask;
    for (int k = 0; k < MKID_K_COUNT; ++k) { c->tot_ms[k] = 0; c->launches[k] = 0; }
    return MKID_OK;
}

int mkid_set_timing(mkid_ctx* c, int32_t enable) {
    return mkid_set_timing_mask(c, enable != 0 ? (1u << MKID_K_COUNT) - 1u : 0u);
}

int mkid_get_timing(mkid_ctx* c, int32_t k, double* total_ms, int64_t* launches) {
    if (!c || k < 0 || k >= MKID_K_COUNT || !total_ms || !launches) return MKID_E_ARG;
    int r = flush_timing(c);
    if (r) return r;
    *total_ms = c->tot_ms[k];
    *launches = c->launches[k];
    return MKID_OK;
}

const char* mkid_kernel_name(int32_t k) {
    static const char* names[MKID_K_COUNT] = {"k_channelize", "k_lpf_phase", "k_trigger", "k_compact",
                                              "k_front",      "k_stream_copy", "k_pulse_heights", "k_capture"};
    return (k >= 0 && k < MKID_K_COUNT) ? names[k] : "?";
}

int mkid_pack_reference(const uint64_t* wide, int64_t n, uint64_t* out) {
    if ((!wide || !out) && n > 0) return MKID_E_ARG;
    return plan::pack_reference(wide, n, out) == 0 ? MKID_OK : MKID_E_ARG;
}

}  // extern "C"
