// C ABI of libmkidgpu.so (include/mkidgpu.h): the streaming calls — mkid_process*, mkid_trigger_phase,
// the raw-phase and IQ-tap reads, the avgIQ accumulator.
#include "mkid_ctx.h"

using namespace mkid;
using plan::TrigPlan;

// r + c of the IQ-tap channel (the tap reports y = y' + r + c)
static float2 tap_offset(const mkid_ctx* c) {
    if (c->iq_ch < 0) return make_float2(0.f, 0.f);
    return make_float2((float)c->h_gc[2 * c->iq_ch], (float)c->h_gc[2 * c->iq_ch + 1]);
}

// the avgIQ accumulator after an armed call of J rows: the device summed y', the host adds J G c'.
// acc_rows < 0: a failed call left partial sums; the average stays invalid until re-armed.
static void acc_account(mkid_ctx* c, int64_t J) {
    if (!c->acc_on || c->acc_rows < 0) return;
    c->acc_rows += J;
    for (size_t i = 0; i < c->acc_off.size(); ++i) c->acc_off[i] += (double)J * c->h_gc[i];
}

// Plans a call of n samples within the context's workspace (plan::plan_call, mkid_plan.cpp), then
// marks what the carried state belongs to: from the first launch on the context carries that kind of
// stream, even if a later step of the call fails (a failed planning leaves the stream kind as it was).
static int begin_call(mkid_ctx* c, int64_t n, int kind, TrigPlan& p) {
    if (const char* msg = plan::plan_call(c->ws, c->C, c->N, c->mode, c->cfg.dead_time, n, p)) FAIL(c, MKID_E_ARG, msg);
    c->stream_kind = kind;
    return MKID_OK;
}

// Fused front end: one launch, ADC -> phase and Fix16_13 phase (d_raw). (Round 2 also had an opt-in
// two-stream pipeline running a register-lean trigger beside the front end; it never paid — the
// front ends keep their SIMDs ~77 % VALU-busy, and the lean kernel alone is no faster than
// k_trig_spec — and was removed in round 3: profiles/r02/r02_v7_kbench_pipeline.json,
// r03_h_kbench_trig_lean_standalone*.json.)
static int front_fused(mkid_ctx* c, const uint32_t* x, int64_t K, float* d_phase) {
    KTime kt;
    FrontArgs fa{};
    fa.x = x;
    fa.xhist = c->xhist.get();
    fa.pfbq = c->d_pfbq.get();
    fa.bins = c->d_bins.get();
    fa.lo = c->d_lo.get();
    fa.cen = Centring{c->d_ncen.get(), c->d_cor.get(), tap_offset(c)};
    fa.phase = d_phase;
    fa.raw = c->d_raw.get();
    fa.ysum = c->acc_on ? c->d_ysum.get() : nullptr;
    fa.K = K;
    fa.k0 = c->k0;
    fa.P = c->P;
    fa.ncu = c->ncu;
    fa.taps = c->lpf;
    fa.iqtap = c->iq_ch >= 0 ? c->d_iqtap.get() : nullptr;
    fa.iq_ch = c->iq_ch;
    fa.slot_ch = c->N == 2048 ? c->d_slot_ch.get() : nullptr;   // k_front3 at N = 2048 only
    tstart(c, MKID_K_FRONT, &kt, c->stream);
    HIPCHK(c, launch_fused(c->N, fa, c->stream));
    tstop(c, &kt, c->stream);
    return MKID_OK;
}

// Split front end: the channeliser stages the call's K baseband frames in d_z, the low-pass reads
// them behind the 24 frames carried in zhist, then zhist takes the call's last 24.
static int front_split(mkid_ctx* c, const uint32_t* x, int64_t K, float* d_phase) {
    KTime kt;
    float2* z = c->d_z.get();
    ChanArgs ca{x, c->xhist.get(), c->d_pfb.get(), c->d_bins.get(), c->d_lo.get(), z, K, c->k0, c->P, 0};
    tstart(c, MKID_K_CHANNELIZE, &kt, c->stream);
    HIPCHK(c, launch_channelize(c->N, ca, c->stream));
    tstop(c, &kt, c->stream);
    LpfArgs la{z, c->zhist.get(), Centring{c->d_ncen.get(), c->d_cor.get(), tap_offset(c)}, d_phase,
               c->d_raw.get(), c->acc_on ? c->d_ysum.get() : nullptr, K / 2, c->C, c->lpf,
               c->iq_ch >= 0 ? c->d_iqtap.get() : nullptr, c->iq_ch};
    tstart(c, MKID_K_FIR_PHASE, &kt, c->stream);
    HIPCHK(c, launch_lpf_phase(la, c->stream));
    tstop(c, &kt, c->stream);
    HIPCHK(c, c->zhist.roll(z, K, c->stream));
    return MKID_OK;
}

// What every call ends with, on the context stream: K7 over the call's p.J phase rows at `raw`
// (matched filter, baseline, trigger state machine: speculative segments + fix-up) into the
// [C][nseg][capseg] slot table, then K8, one compaction -> channel-major, time-ascending. The
// raw-phase history roll, and the ADC history's (xroll, or null), ride along as extra blocks of the
// compaction's gather launch: no kernel of the call reads the rolled-to buffers, and the buffers
// swap roles once the launch is enqueued (enqueued kernels keep the pointers they were launched with).
static int finish_call(mkid_ctx* c, const TrigPlan& p, const int16_t* raw, const RollJob* xroll,
                       uint64_t* d_events, int64_t cap, int64_t* d_counts) {
    hipStream_t s = c->stream;
    KTime kt;
    TrigSpecArgs ta{raw, c->rhist.get(), c->d_fir.get(), c->d_thr.get(), c->d_rearm.get(), c->d_tstate.get(),
                    c->d_tstate.get(), c->d_sspec.get(), c->d_send.get(), c->d_slots.get(), c->d_chcounts.get(),
                    c->d_scratch.get(), c->d_reruns.get(),
                    p.J,        c->j0,      c->C,       p.nseg,        p.L,          p.W,
                    p.capseg,   c->mode,    c->alpha,   c->kf,         c->kq,        c->base_thr,
                    c->cfg.dead_time, p.nseg, 0, c->svf.filt.get(), c->svf.refix.get(), c->svf.refix_pk.get()};
    tstart(c, MKID_K_TRIGGER, &kt, s);
    HIPCHK(c, launch_trigger(ta, s));
    tstop(c, &kt, s);
    const RollJob rroll = c->rhist.job(raw, p.J);
    tstart(c, MKID_K_COMPACT, &kt, s);
    HIPCHK(c, launch_compact(c->d_slots.get(), c->d_chcounts.get(), (int64_t)c->C * p.nseg, p.capseg, d_events, cap,
                             d_counts, c->d_scan.get(), &rroll, xroll, s));
    tstop(c, &kt, s);
    c->rhist.swap();
    c->j0 += p.J;
    return MKID_OK;
}

// One process call, one piece: the front-end stage (the only difference between a fused and a split
// context) over the call's n samples into d_raw, then the shared tail.
static int process_call(mkid_ctx* c, const uint32_t* x, int64_t n, float* d_phase, uint64_t* d_events, int64_t cap,
                        int64_t* d_counts) {
    TrigPlan p;
    if (int r = begin_call(c, n, 1, p)) return r;
    const int64_t K = n / c->M;
    c->last_J = 0;   // d_raw is being rewritten
    if (int r = c->fused ? front_fused(c, x, K, d_phase) : front_split(c, x, K, d_phase)) return r;
    if (c->fault_launch > 0 && ++c->launch_count == c->fault_launch)
        FAIL(c, MKID_E_HIP, "injected launch failure (MKID_FAULT_LAUNCH)");
    c->k0 += K;
    c->last_J = p.J;
    c->iq_rows = c->iq_ch >= 0 ? p.J : 0;
    const RollJob xroll = c->xhist.job(x, n);
    if (int r = finish_call(c, p, c->d_raw.get(), &xroll, d_events, cap, d_counts)) return r;
    c->xhist.swap();
    return MKID_OK;
}

extern "C" {

int mkid_process_device(mkid_ctx* c, const int16_t* d_iq, int64_t n, float* d_phase, uint64_t* d_events,
                        int64_t cap, int64_t* d_counts) {
    if (!c || !d_iq || !d_counts || (cap > 0 && !d_events)) return MKID_E_ARG;
    if (n <= 0 || n % c->N != 0) FAIL(c, MKID_E_ARG, "nsamples must be a positive multiple of N");
    // the workspace (z, raw rows, IQ tap, slot table) is sized for max_chunk samples per call
    if (n > c->cfg.max_chunk) FAIL(c, MKID_E_ARG, "nsamples exceeds cfg.max_chunk");
    if (((uintptr_t)d_iq & 15) != 0) FAIL(c, MKID_E_ARG, "d_iq must be 16-byte aligned");
    if (c->stream_kind == 2)
        FAIL(c, MKID_E_STATE, "the context carries a phase-row stream (mkid_trigger_phase); mkid_reset_stream first");
    HIPCHK(c, hipSetDevice(c->device));
    const int r = process_call(c, (const uint32_t*)d_iq, n, d_phase, d_events, cap, d_counts);
    if (r == MKID_OK) acc_account(c, n / c->N);
    else if (c->acc_on) c->acc_rows = -1;   // the front-end launch may have added to the sums
    return r;
}

int mkid_trigger_phase(mkid_ctx* c, const int16_t* d_raw, int64_t rows, uint64_t* d_events, int64_t cap,
                       int64_t* d_counts) {
    if (!c || !d_raw || !d_counts || (cap > 0 && !d_events)) return MKID_E_ARG;
    if (rows <= 0 || rows > c->cfg.max_chunk / c->N) FAIL(c, MKID_E_ARG, "rows must be in 1 .. max_chunk/N");
    if (((uintptr_t)d_raw & 3) != 0) FAIL(c, MKID_E_ARG, "d_raw must be 4-byte aligned");
    if (c->stream_kind == 1)
        FAIL(c, MKID_E_STATE, "the context carries an ADC stream (mkid_process); mkid_reset_stream first");
    HIPCHK(c, hipSetDevice(c->device));
    TrigPlan p;
    if (int r = begin_call(c, rows * c->N, 2, p)) return r;
    return finish_call(c, p, d_raw, nullptr, d_events, cap, d_counts);
}

int mkid_process(mkid_ctx* c, const int16_t* iq, int64_t n, float* phase_out, uint64_t* events_out, int64_t cap,
                 int64_t* nevents) {
    if (!c || !iq || !nevents || (cap > 0 && !events_out)) return MKID_E_ARG;
    if (n <= 0 || n % c->N != 0) FAIL(c, MKID_E_ARG, "nsamples must be a positive multiple of N");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t chunk = c->cfg.max_chunk;
    // hard bound for a whole call of `chunk` samples (per channel: J/(dead+3)+2 packets)
    const int64_t evcap = (int64_t)c->C * ((chunk / c->N) / (c->cfg.dead_time + 3) + 2);
    if (!c->d_in.get()) {   // staging, on first use; d_in last: it stands for all three
        HIPCHK(c, c->d_phase_ws.alloc((size_t)(chunk / c->N) * c->C));
        HIPCHK(c, c->d_ev_ws.alloc((size_t)evcap));
        HIPCHK(c, c->d_in.alloc((size_t)chunk));
    }
    int64_t produced = 0, written = 0;
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t S = std::min(chunk, n - off);
        HIPCHK(c, hipMemcpyAsync(c->d_in.get(), iq + 2 * off, (size_t)S * 4, hipMemcpyHostToDevice, c->stream));
        int r = mkid_process_device(c, (const int16_t*)c->d_in.get(), S, phase_out ? c->d_phase_ws.get() : nullptr,
                                    c->d_ev_ws.get(), evcap, c->d_counts.get());
        if (r) return r;
        int64_t cnt[2];
        HIPCHK(c, hipMemcpyAsync(cnt, c->d_counts.get(), 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (phase_out)
            HIPCHK(c, hipMemcpyAsync(phase_out + (off / c->N) * c->C, c->d_phase_ws.get(),
                                     (size_t)(S / c->N) * c->C * 4, hipMemcpyDeviceToHost, c->stream));
        const int64_t take = std::max<int64_t>(0, std::min(cnt[1], cap - written));
        if (take > 0)
            HIPCHK(c, hipMemcpyAsync(events_out + written, c->d_ev_ws.get(), (size_t)take * 8, hipMemcpyDeviceToHost,
                                     c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        produced += cnt[0];
        written += take;
    }
    *nevents = produced;
    if (n > chunk) plan::merge_channel_major(events_out, written);   // chunks were compacted separately
    if (produced > written) FAIL(c, MKID_E_OVERFLOW, "event capacity exceeded; events dropped");
    return MKID_OK;
}

int mkid_last_raw_phase(mkid_ctx* c, const int16_t** d_raw, int64_t* nrows) {
    if (!c || !d_raw || !nrows) return MKID_E_ARG;
    *d_raw = c->d_raw.get();
    *nrows = c->last_J;
    return MKID_OK;
}

int mkid_read_raw_phase(mkid_ctx* c, int16_t* host_out, int64_t cap_rows, int64_t* rows) {
    if (!c || !rows || (cap_rows > 0 && !host_out)) return MKID_E_ARG;
    *rows = c->last_J;
    const int64_t n = std::min(c->last_J, cap_rows);
    if (n <= 0) return MKID_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_raw.get(), (size_t)n * c->C * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKID_OK;
}

int mkid_set_iq_tap(mkid_ctx* c, int32_t channel) {
    if (!c) return MKID_E_ARG;
    if (channel >= c->C) FAIL(c, MKID_E_ARG, "iq tap channel out of range");
    c->iq_ch = channel < 0 ? -1 : channel;
    c->iq_rows = 0;
    return MKID_OK;
}

int mkid_read_iq_tap(mkid_ctx* c, int16_t* host_iq, int64_t cap_rows, int64_t* rows) {
    if (!c || !rows || (cap_rows > 0 && !host_iq)) return MKID_E_ARG;
    *rows = c->iq_rows;
    const int64_t n = std::min(c->iq_rows, cap_rows);
    if (n <= 0) return MKID_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_iq, c->d_iqtap.get(), (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKID_OK;
}

int mkid_trigger_reruns(mkid_ctx* c, int64_t* total) {
    if (!c || !total) return MKID_E_ARG;
    std::vector<int32_t> r(c->C);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(r.data(), c->d_reruns.get(), (size_t)c->C * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t s = 0;
    for (int v : r) s += v;
    *total = s;
    return MKID_OK;
}

int mkid_set_accumulator(mkid_ctx* c, int32_t enable) {
    if (!c) return MKID_E_ARG;
    if (enable != 0 && enable != 1) FAIL(c, MKID_E_ARG, "enable must be 0 or 1");
    if (enable) {   // every arm starts a new average (avgIQ_ctrl strobe + startAccumulator 1)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipMemsetAsync(c->d_ysum.get(), 0, (size_t)c->C * 16, c->stream));
        c->acc_rows = 0;
        std::fill(c->acc_off.begin(), c->acc_off.end(), 0.0);
    }
    c->acc_on = enable != 0;
    return MKID_OK;
}

int mkid_avg_iq(mkid_ctx* c, float* mi, float* mq) {
    if (!c || !mi || !mq) return MKID_E_ARG;
    if (c->acc_rows < 0)
        FAIL(c, MKID_E_STATE, "a process call failed while the avgIQ accumulator was armed: re-arm it");
    if (c->acc_rows == 0)
        FAIL(c, MKID_E_STATE, "the avgIQ accumulator holds no rows: arm it (mkid_set_accumulator) before processing");
    std::vector<long long> s(2 * (size_t)c->C);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(s.data(), c->d_ysum.get(), (size_t)c->C * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double inv = 1.0 / (double)c->acc_rows, scale = 1.0 / (double)(1 << kYsumFrac);
    for (int i = 0; i < c->C; ++i) {
        mi[i] = (float)(((double)s[2 * i] * scale + c->acc_off[2 * i]) * inv);
        mq[i] = (float)(((double)s[2 * i + 1] * scale + c->acc_off[2 * i + 1]) * inv);
    }
    return MKID_OK;
}

}  // extern "C"
