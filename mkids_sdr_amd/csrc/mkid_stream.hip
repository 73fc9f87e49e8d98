// C ABI of libmkidgpu.so (include/mkidgpu.h): the streaming calls — mkid_process*, mkid_trigger_phase,
// the raw-phase and IQ-tap reads, the avgIQ accumulator.
#include "mkid_ctx.h"

using namespace mkid;
using plan::SubPlan;

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

// One call's trigger plan: its sub-chunks (each with its place in the slot table) and the table's geometry
struct CallPlan {
    std::vector<SubPlan> subs;
    int32_t stride = 0, capseg = 0;
};

// Plans a call of n samples within the context's workspace (plan::plan_call, mkid_plan.cpp), then
// marks what the carried state belongs to: from the first launch on the context carries that kind of
// stream, even if a later step of the call fails (a failed planning leaves the stream kind as it was).
static int begin_call(mkid_ctx* c, int64_t n, int kind, CallPlan& p) {
    if (const char* msg = plan::plan_call(c->ws, c->C, c->N, c->mode, c->cfg.dead_time, n, p.subs, p.stride, p.capseg))
        FAIL(c, MKID_E_ARG, msg);
    c->stream_kind = kind;
    return MKID_OK;
}

// K7 on stream s for the sub-chunk's phase rows in d_raw: matched filter, baseline, trigger state
// machine (speculative segments + fix-up) into segments sp.seg_off.. of the call's slot table, then
// the raw-phase history roll. Compaction (K8) runs once per call (compact_call).
static int run_trigger(mkid_ctx* c, const int16_t* raw, const CallPlan& p, const SubPlan& sp, hipStream_t s,
                       bool roll = true) {
    KTime kt;
    TrigSpecArgs ta{raw, c->rhist.get(), c->d_fir.get(), c->d_thr.get(), c->d_rearm.get(), c->d_tstate.get(),
                    c->d_tstate.get(), c->d_sspec.get(), c->d_send.get(), c->d_slots.get(), c->d_chcounts.get(),
                    c->d_scratch.get(), c->d_reruns.get(),
                    sp.J,       c->j0,      c->C,       sp.nseg,       sp.L,         sp.W,
                    p.capseg,   c->mode,    c->alpha,   c->kf,         c->kq,        c->base_thr,
                    c->cfg.dead_time, p.stride, sp.seg_off, c->svf.filt.get(), c->svf.refix.get(), c->svf.refix_pk.get()};
    tstart(c, MKID_K_TRIGGER, &kt, s);
    HIPCHK(c, launch_trigger(ta, s));
    tstop(c, &kt, s);
    // roll = false: the caller rolls the history together with the ADC history (process_fused)
    if (roll) HIPCHK(c, c->rhist.roll(raw, sp.J, s));
    return MKID_OK;
}

// K8: one compaction over the call's [C][stride] slot table -> channel-major, time-ascending.
// Up to two history rolls ride along as extra blocks of the gather launch.
static int compact_call(mkid_ctx* c, const CallPlan& p, uint64_t* d_events, int64_t cap, int64_t* d_counts,
                        hipStream_t s, const RollJob* roll1 = nullptr, const RollJob* roll2 = nullptr) {
    KTime kt;
    tstart(c, MKID_K_COMPACT, &kt, s);
    HIPCHK(c, launch_compact(c->d_slots.get(), c->d_chcounts.get(), (int64_t)c->C * p.stride, p.capseg, d_events,
                             cap, d_counts, c->d_scan.get(), roll1, roll2, s));
    tstop(c, &kt, s);
    return MKID_OK;
}

// Fused front end: one front-end launch per sub-chunk (ADC -> phase, raw), then K7, one
// compaction per call, all on the context stream. (Round 2 also had an opt-in two-stream pipeline
// running a register-lean trigger beside the front end; it never paid — the front ends keep their
// SIMDs ~77 % VALU-busy, and the lean kernel alone is no faster than k_trig_spec — and was removed
// in round 3: profiles/r02/r02_v7_kbench_pipeline.json, r03_h_kbench_trig_lean_standalone*.json.)
static int process_fused(mkid_ctx* c, const int16_t* d_iq, int64_t n, float* d_phase, uint64_t* d_events,
                         int64_t cap, int64_t* d_counts) {
    const int C = c->C, N = c->N, M = c->M;
    const int64_t G = c->ws.G;
    hipStream_t A = c->stream;
    CallPlan p;
    if (int r = begin_call(c, n, 1, p)) return r;
    const uint32_t* x = (const uint32_t*)d_iq;
    c->last_J = 0;
    size_t si = 0;
    RollJob last_roll{};
    const Centring cen{c->d_ncen.get(), c->d_cor.get(), tap_offset(c)};
    for (int64_t off = 0; off < n; off += G, ++si) {
        const int64_t S = std::min<int64_t>(G, n - off);
        const int64_t K = S / M, J = S / N;
        int16_t* raw = c->d_raw.get() + (off / N) * C;
        KTime kt;
        FrontArgs fa{};
        fa.x = x + off;
        fa.xhist = c->xhist.get();
        fa.pfbq = c->d_pfbq.get();
        fa.bins = c->d_bins.get();
        fa.lo = c->d_lo.get();
        fa.cen = cen;
        fa.phase = d_phase ? d_phase + (off / N) * C : nullptr;
        fa.raw = raw;
        fa.ysum = c->acc_on ? c->d_ysum.get() : nullptr;
        fa.K = K;
        fa.k0 = c->k0;
        fa.avail = off;
        fa.P = c->P;
        fa.ncu = c->ncu;
        fa.taps = c->lpf;
        fa.iqtap = c->iq_ch >= 0 ? c->d_iqtap.get() + (off / N) * 2 : nullptr;
        fa.iq_ch = c->iq_ch;
        fa.slot_ch = c->N == 2048 ? c->d_slot_ch.get() : nullptr;   // k_front3 at N = 2048 only
        tstart(c, MKID_K_FRONT, &kt, A);
        HIPCHK(c, launch_fused(N, fa, A));
        tstop(c, &kt, A);
        if (c->fault_launch > 0 && ++c->launch_count == c->fault_launch)
            FAIL(c, MKID_E_HIP, "injected launch failure (MKID_FAULT_LAUNCH)");
        const bool last = off + S >= n;
        if (int r = run_trigger(c, raw, p, p.subs[si], A, !last)) return r;
        if (last) last_roll = c->rhist.job(raw, p.subs[si].J);
        c->k0 += K;
        c->j0 += J;
        c->last_J += J;
        c->last_subJ = J;
        c->last_raw_row = off / N;
    }
    // with the last sub-chunk's raw-phase history and the call's ADC history rolled in the
    // compaction's gather launch (no kernel of the call reads the rolled-to buffers). The buffers
    // swap roles once the launch is enqueued: enqueued kernels keep the pointers they were launched with
    const RollJob xroll = c->xhist.job(x, n);
    if (int r = compact_call(c, p, d_events, cap, d_counts, A, &last_roll, &xroll)) return r;
    c->rhist.swap();
    c->xhist.swap();
    c->iq_rows = c->iq_ch >= 0 ? n / N : 0;
    return MKID_OK;
}

// Split front end (channeliser on stream A, low-pass / trigger / compaction on stream B).
static int process_split(mkid_ctx* c, const int16_t* d_iq, int64_t n, float* d_phase, uint64_t* d_events,
                         int64_t cap, int64_t* d_counts) {
    const int C = c->C, N = c->N, M = c->M;
    const int64_t G = c->ws.G;
    hipStream_t A = c->stream, B = c->sB;
    CallPlan p;
    if (int r = begin_call(c, n, 1, p)) return r;
    // B joins A's order (inputs written by earlier work on A, previous calls) ...
    HIPCHK(c, hipEventRecord(c->ev_start, A));
    HIPCHK(c, hipStreamWaitEvent(B, c->ev_start, 0));
    const uint32_t* x = (const uint32_t*)d_iq;
    const Centring cen{c->d_ncen.get(), c->d_cor.get(), tap_offset(c)};
    c->last_J = 0;
    size_t si = 0;
    const float2* zprev = c->zhist.get();  // the 24 frames before the current sub-chunk
    for (int64_t off = 0; off < n; off += G, ++si) {
        const int64_t S = std::min<int64_t>(G, n - off);
        const int64_t K = S / M, J = S / N;
        const int b = c->zi;
        float2* z = c->d_zb[b].get();
        KTime kt;
        // ---- stream A: channeliser into z[b] once its last reader is done ----
        HIPCHK(c, hipStreamWaitEvent(A, c->ev_zfree[b], 0));
        ChanArgs ca{x + off, c->xhist.get(), c->d_pfb.get(), c->d_bins.get(), c->d_lo.get(), z, K, c->k0, c->P,
                    0, 0, off};
        tstart(c, MKID_K_CHANNELIZE, &kt, A);
        HIPCHK(c, launch_channelize(N, ca, A));
        tstop(c, &kt, A);
        HIPCHK(c, hipEventRecord(c->ev_zready[b], A));

        // ---- stream B: low-pass + phase and trigger of this sub-chunk ----
        HIPCHK(c, hipStreamWaitEvent(B, c->ev_zready[b], 0));
        LpfArgs la{z, zprev, cen, d_phase ? d_phase + (off / N) * C : nullptr,
                   c->d_raw.get(), c->acc_on ? c->d_ysum.get() : nullptr, J, C, c->lpf,
                   c->iq_ch >= 0 ? c->d_iqtap.get() + (off / N) * 2 : nullptr, c->iq_ch};
        tstart(c, MKID_K_FIR_PHASE, &kt, B);
        HIPCHK(c, launch_lpf_phase(la, B));
        tstop(c, &kt, B);
        if (off + S >= n || K < kLpfHist) {
            // carry the trailing 24 frames through zhist: always at the end of a call (next
            // call's history), and between sub-chunks too short to hold them
            HIPCHK(c, c->zhist.roll(z, K, B, zprev));
            zprev = c->zhist.get();
            HIPCHK(c, hipEventRecord(c->ev_zfree[b], B));
        } else {
            zprev = z + (K - kLpfHist) * C;  // read in place by the next sub-chunk's low-pass
        }
        // the previous sub-chunk's buffer (history of the low-pass above) may now be overwritten
        HIPCHK(c, hipEventRecord(c->ev_zfree[b ^ 1], B));
        c->zi ^= 1;

        if (int r = run_trigger(c, c->d_raw.get(), p, p.subs[si], B)) return r;
        c->k0 += K;
        c->j0 += J;
        c->last_J += J;
        c->last_subJ = J;
        c->last_raw_row = 0;
    }
    if (int r = compact_call(c, p, d_events, cap, d_counts, B)) return r;
    // ADC history for the next call (all readers of xhist are channeliser launches on A)
    HIPCHK(c, c->xhist.roll(x, n, A));
    // ... and A (the caller's stream) waits for everything B did
    HIPCHK(c, hipEventRecord(c->ev_done, B));
    HIPCHK(c, hipStreamWaitEvent(A, c->ev_done, 0));
    c->iq_rows = c->iq_ch >= 0 ? n / N : 0;
    return MKID_OK;
}

extern "C" {

int mkid_process_device(mkid_ctx* c, const int16_t* d_iq, int64_t n, float* d_phase, uint64_t* d_events,
                        int64_t cap, int64_t* d_counts) {
    if (!c || !d_iq || !d_counts || (cap > 0 && !d_events)) return MKID_E_ARG;
    if (n <= 0 || n % c->N != 0) FAIL(c, MKID_E_ARG, "nsamples must be a positive multiple of N");
    // the workspace (raw rows, IQ tap, slot table) is sized for max_chunk samples per call
    if (n > c->cfg.max_chunk) FAIL(c, MKID_E_ARG, "nsamples exceeds cfg.max_chunk");
    if (((uintptr_t)d_iq & 15) != 0) FAIL(c, MKID_E_ARG, "d_iq must be 16-byte aligned");
    if (c->stream_kind == 2)
        FAIL(c, MKID_E_STATE, "the context carries a phase-row stream (mkid_trigger_phase); mkid_reset_stream first");
    HIPCHK(c, hipSetDevice(c->device));
    const int r = c->fused ? process_fused(c, d_iq, n, d_phase, d_events, cap, d_counts)
                           : process_split(c, d_iq, n, d_phase, d_events, cap, d_counts);
    if (r == MKID_OK) acc_account(c, n / c->N);
    else if (c->acc_on) c->acc_rows = -1;   // some front-end launches may have added to the sums
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
    CallPlan p;
    if (int r = begin_call(c, rows * c->N, 2, p)) return r;
    int64_t r0 = 0;
    for (const SubPlan& sp : p.subs) {
        if (int r = run_trigger(c, d_raw + r0 * c->C, p, sp, c->stream)) return r;
        r0 += sp.J;
        c->j0 += sp.J;
    }
    return compact_call(c, p, d_events, cap, d_counts, c->stream);
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
    *d_raw = c->d_raw.get() + c->last_raw_row * c->C;
    *nrows = std::min(c->last_subJ, c->ws.Jmax);
    return MKID_OK;
}

int mkid_read_raw_phase(mkid_ctx* c, int16_t* host_out, int64_t cap_rows, int64_t* rows) {
    if (!c || !rows || (cap_rows > 0 && !host_out)) return MKID_E_ARG;
    const int64_t avail = std::min(c->last_subJ, c->ws.Jmax);
    *rows = avail;
    const int64_t n = std::min(avail, cap_rows);
    if (n <= 0) return MKID_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_raw.get() + c->last_raw_row * c->C, (size_t)n * c->C * 2,
                             hipMemcpyDeviceToHost, c->stream));
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
