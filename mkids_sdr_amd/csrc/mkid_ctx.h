// The context behind the C ABI and what owns its device memory; private to the host translation
// units of libmkidgpu.so (mkid_api.hip, mkid_stream.hip, mkid_calib.hip, mkid_observe.hip,
// mkid_iqnoise.hip).
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "mkid_internal.h"
#include "mkid_plan.h"

// Device memory with one owner: move-only, freed by the destructor. alloc() never allocates zero
// bytes and replaces the held buffer only on success, so a failed (re)allocation leaves it as it was.
template <typename T>
class DevBuf {
    T* p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t n) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) return e;
        reset();
        p_ = (T*)q;
        return hipSuccess;
    }
    T* get() const { return p_; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
};

// A workspace grown on demand. reserve() does nothing while the buffer holds `need` elements;
// otherwise it allocates into a local, synchronises the context's stream once (an enqueued call may
// still use the old buffer) and moves the new one in. A failed allocation leaves buffer and size.
template <typename T>
struct GrowBuf {
    DevBuf<T> buf;
    size_t n = 0;
    T* get() const { return buf.get(); }
    int reserve(mkid_ctx* c, size_t need);   // MKID_OK, or MKID_E_HIP with the context's error set
};

// A history carried between calls: `rows` rows of `row_bytes` in `cur`, rolled into `spare` (the
// last `rows` of old rows + fresh rows), after which the two swap roles — enqueued kernels keep the
// pointers they were launched with, so there is no device-to-device copy per call.
template <typename T>
struct RollBuf {
    DevBuf<T> cur, spare;
    int64_t rows = 0, row_bytes = 0;

    hipError_t alloc(int64_t nrows, int64_t nrow_bytes) {   // both or neither
        DevBuf<T> a, b;
        const size_t n = (size_t)(nrows * nrow_bytes) / sizeof(T);
        hipError_t e = a.alloc(n);
        if (e == hipSuccess) e = b.alloc(n);
        if (e != hipSuccess) return e;
        cur = std::move(a);
        spare = std::move(b);
        rows = nrows;
        row_bytes = nrow_bytes;
        return hipSuccess;
    }
    T* get() const { return cur.get(); }
    size_t bytes() const { return (size_t)(rows * row_bytes); }
    // the roll of `fresh_rows` rows at `fresh` behind the history into spare
    mkid::RollJob job(const void* fresh, int64_t fresh_rows) const {
        return mkid::RollJob{spare.get(), cur.get(), fresh, rows, fresh_rows, row_bytes};
    }
    void swap() { std::swap(cur, spare); }
    hipError_t roll(const void* fresh, int64_t fresh_rows, hipStream_t s) {
        const mkid::RollJob j = job(fresh, fresh_rows);
        const hipError_t e =
            mkid::launch_hist_roll(j.dst, j.old_hist, j.fresh, j.hist_rows, j.fresh_rows, j.row_bytes, s);
        if (e == hipSuccess) swap();
        return e;
    }
};

// The SVF trigger path's device tables (TrigSpecArgs filt / refix / refix_pk), allocated on the
// first mkid_set_baseline(SVF): all three or none, and a failed alloc() is tried again by the next.
struct SvfTables {
    DevBuf<int16_t> filt;            // [Jmax][C] filter pre-pass output (k_mf_rows)
    DevBuf<mkid::RefixRes> refix;    // [C][nseg_max] parallel re-run results (k_trig_refix)
    DevBuf<uint64_t> refix_pk;       // [slot_cap] their true packets (the slot table's geometry)
    bool ready() const { return filt.get() != nullptr; }
    hipError_t alloc(const mkid::plan::Workspace& ws, int C) {
        SvfTables t;
        hipError_t e = t.filt.alloc((size_t)ws.Jmax * C);
        if (e == hipSuccess) e = t.refix.alloc((size_t)C * (size_t)ws.nseg_max);
        if (e == hipSuccess) e = t.refix_pk.alloc((size_t)ws.slot_cap);
        if (e == hipSuccess) *this = std::move(t);
        return e;
    }
};

struct KTime { int k; hipEvent_t a, b; };

// The stream and the timing events of a context. A base of mkid_ctx, so that it is destroyed after
// the members: buffers first, then events, then the stream.
struct CtxHandles {
    hipStream_t own = nullptr;
    std::vector<KTime> pending;     // timing
    std::vector<hipEvent_t> pool;
    ~CtxHandles() {
        for (auto& kt : pending) {
            (void)hipEventDestroy(kt.a);
            (void)hipEventDestroy(kt.b);
        }
        for (auto e : pool) (void)hipEventDestroy(e);
        if (own) (void)hipStreamDestroy(own);
    }
};

struct mkid_ctx : CtxHandles {
    mkid_cfg cfg{};
    int device = 0;
    hipStream_t stream = nullptr;   // the caller's (mkid_set_stream) or `own`: all work runs on it
    std::string err;
    int C = 0, N = 0, M = 0, T = 0, P = 0;
    int ncu = 256;  // compute units of the device (launch grids are per-CU multiples)
    // what the carried stream state belongs to: 0 none (fresh / reset), 1 an ADC stream
    // (mkid_process*), 2 a phase-row stream (mkid_trigger_phase); mixing them needs a reset
    int stream_kind = 0;
    mkid::plan::Workspace ws;      // what the context was sized for (plan::size_workspace)
    // configuration
    DevBuf<float> d_pfb;         // effective taps h_q 2^-S (float, split path)
    DevBuf<uint2> d_pfbq;        // [N] {h_q[0]|h_q[1]<<16, h_q[2]|h_q[3]<<16} (fused path, int16 dot2)
    int pfb_shift = 0;           // S
    DevBuf<int32_t> d_bins;
    DevBuf<float2> d_lo;
    DevBuf<int16_t> d_fir;
    // IQ-loop centres (loadIQcenters) and the centred low-pass constants derived from them and the
    // low-pass taps (upload_centring): d_ncen = -c', d_cor = r (mkid_internal.h Centring)
    std::vector<float> h_ic, h_qc;
    DevBuf<float2> d_ncen, d_cor;
    std::vector<double> h_gc;   // [2C] G c' (= r + c): added back to y' for the raw IQ
    DevBuf<int32_t> d_thr;
    DevBuf<int32_t> d_rearm;         // [C] re-arm levels (upload_rearm)
    std::vector<int32_t> h_thr;
    int32_t rearm_q8 = 0;            // mkid_set_rearm hysteresis fraction (/256)
    mkid::LpfTaps lpf{};
    int32_t mode = MKID_BASE_EMA, alpha = 41, kf = 82, kq = 93623, base_thr = 8192;
    // stream state
    RollBuf<uint32_t> xhist;    // ADC samples carried between calls (front_hist_samples / T N - M)
    RollBuf<float2> zhist;      // [kLpfHist][C]
    RollBuf<int16_t> rhist;     // [kRawHist][C]
    DevBuf<mkid::TrigState> d_tstate;
    int64_t k0 = 0, j0 = 0;
    // test hook (MKID_FAULT_LAUNCH=n at mkid_create): the n-th front-end launch of the context (one
    // per process call; the split front end's three count as one) reports a HIP failure after it
    // was enqueued, to test the state a partly enqueued call leaves
    int64_t fault_launch = 0, launch_count = 0;
    bool fused = false;  // K1-K6 in one kernel (k_front / k_front3 / k_front5: no z buffer)
    // workspace
    DevBuf<float2> d_z;              // [Kmax][C] baseband of the call (split front end only)
    DevBuf<int16_t> d_raw;           // [Jmax][C] Fix16_13 phase of the call
    SvfTables svf;                   // none until the SVF baseline is first selected
    DevBuf<long long> d_ysum;        // [C][2] fixed point 2^-kYsumFrac: sums of y' while armed
    // avgIQ accumulator (K9; startAccumulator / avgIQ_ctrl, ROACH_Setup.py:654-659): armed by
    // mkid_set_accumulator; rows accumulated since arming and the host-side sums of G c' over them
    bool acc_on = false;
    int64_t acc_rows = 0;
    std::vector<double> acc_off;   // [2C]
    DevBuf<uint64_t> d_slots;        // [C][nseg][capseg]
    DevBuf<int32_t> d_chcounts;      // [C][nseg]
    DevBuf<int64_t> d_scan;          // [C][nseg]
    DevBuf<mkid::TrigState> d_sspec, d_send;  // [nseg][C]
    DevBuf<uint64_t> d_scratch;      // [C][capseg]
    DevBuf<int32_t> d_reruns;        // [C]
    DevBuf<int64_t> d_counts;        // [2] used by the host-pointer API
    int64_t last_J = 0;     // phase rows of the last call (held in d_raw from row 0)
    // IQ snapshot tap: low-pass output of one channel for the rows of the last call
    int32_t iq_ch = -1;
    DevBuf<int16_t> d_iqtap;        // [max_chunk/N][2]
    int64_t iq_rows = 0;
    // pulse heights (mkid_set_pulse_filter): the filter and the last phase rows seen by pulse_heights
    DevBuf<float> d_hcoeff;         // [C][h_ncoeff]; none: not configured
    int32_t h_ncoeff = 0, h_pre = 0;
    RollBuf<float> phist;           // [h_ncoeff][C]
    mkid::plan::Carry pcarry;
    // pulse fit (mkid_set_pulse_fit): the search, and carried rows of its own, so that
    // mkid_pulse_heights and mkid_pulse_fit may be given the same rows; allocated once both the
    // filter and the search are known
    int32_t fit_L = -1, fit_s = -1;   // fit_L < 0: not configured
    RollBuf<float> fhist;             // [h_ncoeff + 2 fit_L][C]
    mkid::plan::Carry fcarry;
    // pulse capture (mkid_set_capture): carried phase rows and the double-buffered pending list
    int32_t cap_L = 0, cap_pre = 0, cap_R = 0, cap_PC = 0;   // cap_L = 0: not configured
    RollBuf<float> chist;                                    // [max(L - 1, pre + 1)][C]
    mkid::plan::Carry ccarry;                                // end = -1: no segment
    DevBuf<int64_t> d_cpend[2];                              // [C][cap_PC] unwrapped stamps
    DevBuf<int32_t> d_cpend_n[2], d_cwork;                   // [C]; [C][2]
    int cpend_cur = 0;
    // host copies behind the folded LO table (d_lo = conj(LUT)/2^15 with the (-1)^(b (k+1))
    // bin-parity sign of K4 folded in: P is even, so the sign depends on k mod P only)
    std::vector<float2> h_lo;      // [P][C]
    std::vector<int32_t> h_bins;   // [C]
    // select-slot order of the N = 2048 front end (k_front3): d_slot_ch[slot] = channel (slot_order;
    // MKID_SLOT_ORDER=0 keeps the identity)
    DevBuf<int16_t> d_slot_ch;
    bool slot_order_on = true;
    // replay-trigger workspace (lazy, grown on demand)
    GrowBuf<uint32_t> rflags;
    GrowBuf<double> rmeans;
    // workspace of mkid_bank_filters and mkid_make_template (lazy, grown on demand; plan::plan_bank
    // carves it), and what mkid_make_template's one channel reads and writes besides (lazy)
    GrowBuf<char> bankws;
    struct TplSlot { mkid_bank_result result; int32_t ready; };
    DevBuf<TplSlot> d_tplslot;
    // workspace of mkid_phase_thresholds (lazy, grown on demand; plan::plan_thresholds carves it)
    GrowBuf<char> thrws;
    // tables of mkid_phase_noise_spectra for the last call's n (lazy; noise_plan.n == 0: none;
    // plan::noise_pack_tables lays them out; noise_plan keeps the passes and offsets only)
    DevBuf<char> d_noisetab;
    mkid::plan::NoisePlan noise_plan;
    // mkid_welch_psd and mkid_iq_noise: the workspace (strip sums and the four-step transform's
    // segments; lazy, grown on demand inside plan::kBankBudget unless one channel needs more) and the
    // window and twiddle tables kept per nfft (lazy; a context sees a handful of lengths)
    GrowBuf<char> welchws;
    struct WelchTab {
        int32_t nfft = 0;
        double S2 = 0.0;
        DevBuf<double> w, tw;   // [nfft], [nfft][2]
    };
    std::vector<WelchTab> welch_tabs;
    // mkid_height_spectra: per-workgroup deferred counts and offsets (lazy; their size is fixed,
    // mkid_internal.h kObsMaxBlocks), and the form of the spectra kernel: the plain one (one global
    // atomic per packet) unless MKID_OBS_LDS=1 at mkid_create asks for the LDS table, which the
    // same-process A/B of tools/observe_rate.py did not find clear of it
    DevBuf<int32_t> d_obs_count;
    DevBuf<int64_t> d_obs_off;
    bool obs_lds = false;
    // workspace of mkid_list_photons (lazy, grown on demand with the list's n or cap;
    // mkid_internal.h photon_ws_bytes)
    GrowBuf<char> phws;
    // host-API staging (lazy)
    DevBuf<uint32_t> d_in;
    DevBuf<float> d_phase_ws;
    DevBuf<uint64_t> d_ev_ws;
    // timing
    bool timing = false;
    uint32_t timing_mask = 0;   // bit k: kernel k is timed
    double tot_ms[MKID_K_COUNT] = {0};
    int64_t launches[MKID_K_COUNT] = {0};
};

#define FAIL(ctx, code, msg)       \
    do {                           \
        (ctx)->err = (msg);        \
        return (code);             \
    } while (0)

#define HIPCHK(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);               \
            return MKID_E_HIP;                                                             \
        }                                                                                  \
    } while (0)

template <typename T>
int GrowBuf<T>::reserve(mkid_ctx* c, size_t need) {
    if (need <= n) return MKID_OK;
    DevBuf<T> fresh;
    HIPCHK(c, fresh.alloc(need));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    buf = std::move(fresh), n = need;
    return MKID_OK;
}

// per-kernel timing (mkid_api.hip): events around a launch when kernel k is in the timing mask
void tstart(mkid_ctx* c, int k, KTime* kt, hipStream_t s);
void tstop(mkid_ctx* c, KTime* kt, hipStream_t s);
int flush_timing(mkid_ctx* c);

// host -> device, complete on return (and with it everything enqueued on the stream before)
inline int upload(mkid_ctx* c, void* dst, const void* src, size_t bytes) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKID_OK;
}
