/*
 * mkidgpu.h — flat C ABI of the MI355X MKID channeliser + phase/pulse-trigger hot path.
 *
 * This library replaces the ROACH FPGA firmware that creanero/MKIDS_SDR configures over katcp
 * (the firmware itself is absent from the reference: .MISSING_LARGE_BLOBS:1-27). Each entry point
 * below replaces one group of register/BRAM accesses the reference's host code makes; the
 * reference call site is cited on every declaration (paths relative to the reference root).
 *
 * ABI rules
 *   - every entry point returns int: 0 = ok, negative = MKID_E_* ; mkid_last_error() gives text.
 *   - no C++ exception crosses the ABI; buffers are caller-owned; plain pointers and sizes only.
 *   - one HIP stream per context (its own, or one handed in by mkid_set_stream); a context is not
 *     thread-safe; distinct contexts (one per GPU / feedline) may run concurrently.
 *   - *_device entry points take device pointers and are fully asynchronous on the context's
 *     stream (graph-capturable); the host-pointer entry points copy in/out and synchronise.
 *
 * Geometry: C channels, N = 2C point FFT, hop M = N/2 (2x oversampled), T PFB taps per branch.
 * Input: int16 I/Q pairs (interleaved, I first) at fs. Output: per-channel phase at fs/N
 * (layout [J][C], time-major, J = nsamples/N) and 64-bit photon packets (see MKID_PKT_*).
 */
#ifndef MKIDGPU_H
#define MKIDGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKID_OK 0
#define MKID_E_ARG (-1)       /* bad argument / shape mismatch                      */
#define MKID_E_HIP (-2)       /* HIP runtime failure (message in mkid_last_error)   */
#define MKID_E_STATE (-3)     /* call order violated (e.g. process before config)    */
#define MKID_E_OVERFLOW (-4)  /* event capacity exceeded; events were dropped         */
#define MKID_E_NODEV (-5)     /* no HIP device                                       */

/* Baseline modes of the trigger (K7). The reference writes these registers:
 *   capture_Baseline_alpha  (DataReadout/ChannelizerControls/lib/set_alpha.py:10-17, Fix12_9)
 *   capture_base_Kf/Kq      (lib/set_svf.py:29-35, Fix18_16)
 *   capture_base_thresh     (lib/set_base_thresh.py:9-17, Fix16_13; B_BASE_THRESH setEnvironment.sh:26) */
#define MKID_BASE_NONE 0
#define MKID_BASE_EMA 1
#define MKID_BASE_SVF 2

/* Wide 64-bit photon packet emitted by the device (channel field widened for C > 255):
 *   [63:52] channel (12b) | [51:40] peak Fix12_9 offset (x/2^9-4 rad) | [39:28] baseline Fix12_9
 *   offset | [27:0] phase-sample index mod 2^28.
 * The reference 64-bit packet (ch 8b | peak 12b | p1 12b | base 12b | ts 20b,
 * ROACH_Pulses.py:796-832, PacketMaster.c:291-292) is produced on the host by
 * mkid_pack_reference() for C <= 254. */
#define MKID_PKT_CH_SHIFT 52
#define MKID_PKT_PEAK_SHIFT 40
#define MKID_PKT_BASE_SHIFT 28
#define MKID_PKT_TS_MASK ((1ull << 28) - 1)

/* Front-end (K1-K6) execution: one fused kernel (z stays on-chip) or two kernels with the complex
 * baseband z staged in HBM. Results agree to float rounding; AUTO picks fused where supported. */
#define MKID_FRONT_AUTO 0
#define MKID_FRONT_SPLIT 1

typedef struct mkid_ctx mkid_ctx;

typedef struct mkid_cfg {
    int32_t n_channels;        /* C; ROACH_Setup.py:515 (256)                                  */
    int32_t fft_len;           /* N = 2C; ROACH_Setup.py:507 fft_len = 2**9                    */
    int32_t pfb_taps;          /* T taps per PFB branch (build decision, 4)                    */
    int32_t fir_taps;          /* 26; ROACH_Pulses.py:61                                      */
    int32_t dds_entries;       /* P = 2^16 / C LO samples per channel; ROACH_Setup.py:521-530 */
    int32_t dead_time;         /* trigger dead time in phase samples (build decision)         */
    int32_t max_events_per_ch; /* per-call event capacity per channel (0 = derive from chunk) */
    int32_t front;             /* MKID_FRONT_AUTO (fused K1-K6 kernel, N = 128..4096) or
                                  MKID_FRONT_SPLIT (channeliser + low-pass kernels one after the
                                  other, the call's z in HBM: the reference for the fused kernels,
                                  which every supported N has; it is not built for speed)        */
    int64_t max_chunk;         /* largest nsamples per process call (workspace sizing)        */
    double sample_rate;        /* fs, complex S/s; ROACH_Setup.py:82                           */
} mkid_cfg;

/* Fill *cfg with defaults for C channels (N=2C, T=4, 26 taps, P=65536/C, fs=512e6). */
int mkid_default_cfg(mkid_cfg* cfg, int32_t n_channels);

/* Create a context on HIP device `device`. Replaces FpgaClient(ip,7147)+progdev(bof):
 * ROACH_Setup.py:112-115, ROACH_Pulses.py:51-52. */
int mkid_create(const mkid_cfg* cfg, int32_t device, mkid_ctx** out);
int mkid_destroy(mkid_ctx* ctx);
const char* mkid_last_error(const mkid_ctx* ctx);
/* Error text for failures that happen before a context exists (mkid_create). */
const char* mkid_global_error(void);
int mkid_get_cfg(const mkid_ctx* ctx, mkid_cfg* out);

/* Run the context's kernels on an external hipStream_t (e.g. torch's current stream). NULL
 * restores the context's own stream. All device work of either front end runs on that one stream,
 * in call order: work enqueued on it after a call sees the call's results. */
int mkid_set_stream(mkid_ctx* ctx, void* hip_stream);

/* PFB prototype filter, T*N float coefficients (build decision: the firmware's taps are not in
 * the reference). Applied as 16-bit integers, like an FPGA PFB's fixed-point coefficients:
 * h_q = rint(h * 2^S) with the largest S such that every point's sum_tau |h_q[tau N + p]| <= 65535
 * and every |h_q| <= 32767; the effective taps are h_q * 2^-S (mkids_sdr_amd.pfb.effective_taps). */
int mkid_set_pfb(mkid_ctx* ctx, const float* coeffs, int32_t n);
/* Host-only (no device needed): the effective taps h_q * 2^-S of mkid_set_pfb and S. */
int mkid_pfb_effective_taps(const float* coeffs, int32_t T, int32_t N, float* out, int32_t* shift);
/* Host-only: the channel order the fused front ends give their select threads for a bin set:
 * out[slot] = channel. C = 1024 (k_front3, N = 2048): slot st + 512 q is read by thread st in
 * instruction q, and each select wave keeps its own 128 channels. C = 2048 (the k_front5 layout,
 * N = 4096): slot 64 sw + l + 512 q (select waves sw < 8, q < 3) or 1536 + 64 v + l + 256 q (v < 4,
 * q < 2), each wave keeping the natural channels of its slots; reported for tools/lds_assign.py,
 * not applied (it cut k_front5's LDS conflict cycles 2.6x but cost 2.5-6 % in time, DESIGN.md
 * §5.3). Within a wave the order puts each
 * half-wave's 32 Y reads on distinct LDS bank pairs where the bins allow. A permutation of 0..C-1
 * (the identity for C other than 1024 and 2048). Results do not depend on it: each channel's
 * arithmetic is unchanged. Exposed for tests and tools/lds_assign.py; MKID_SLOT_ORDER=0 at context
 * creation disables it. */
int mkid_slot_order(const int32_t* bins, int32_t C, int16_t* out);

/* Coarse FFT bin per channel: replaces write_int('bins'), write_int('load_bins',(i<<1)+1)
 * (ROACH_Setup.py:534-550; ROACH_Pulses.py:958-974). bins[c] in [0,N). */
int mkid_set_bins(mkid_ctx* ctx, const int32_t* bins, int32_t n);

/* Per-channel DDS LO LUT, de-interleaved and un-shifted: lut_i/lut_q are [C][P] int16, the
 * freqCombLUT('no',...) output of define_DDS_LUT (ROACH_Setup.py:506-532) before it is woven
 * into dram_memory (ROACH_Setup.py:552-570). The device mixes by conj(LUT)/2^15. */
int mkid_set_dds(mkid_ctx* ctx, const int16_t* lut_i, const int16_t* lut_q, int32_t entries_per_ch);

/* IQ low-pass (K5) taps, int12 Fix12_11 (int(lpf*(2**11-1)), ROACH_Pulses.py:69,88-92), shared
 * by all channels, applied to the DDC output with decimation by 2. */
int mkid_set_lpf(mkid_ctx* ctx, const int16_t* taps12, int32_t ntaps);

/* Per-channel matched-filter taps [C][26] int12: replaces FIR_b{2n}b{2n+1} + FIR_load_coeff
 * (ROACH_Pulses.py:59-111). All-zero taps delete a channel (no triggers). */
int mkid_set_fir(mkid_ctx* ctx, const int16_t* taps12, int32_t n_channels, int32_t ntaps);

/* IQ loop centres [C] in channel-output units: replaces conv_phase_centers /
 * conv_phase_load_centers (ROACH_Setup.py:595-605). phase = atan2(Q - qc, I - ic) is evaluated
 * with the centre subtracted inside the low-pass (sum_i g_i (z_i - c/G) + r, G = sum of the
 * low-pass taps, r the float64 residual of G c'), so the fp32 error of the phase does not grow
 * with |centre| / loop radius. Centres must be finite. */
int mkid_set_centers(mkid_ctx* ctx, const float* ic, const float* qc, int32_t n);

/* Per-channel trigger thresholds [C], Fix16_13 raw units relative to baseline (negative-going):
 * replaces capture_threshold / capture_load_thresh (ROACH_Pulses.py:211-354). */
int mkid_set_thresholds(mkid_ctx* ctx, const int32_t* thr, int32_t n);

/* Baseline: mode MKID_BASE_*, alpha Fix12_9 in 0..1024 (gain <= 2.0; larger gains diverge),
 * kf/kq Fix18_16, base_thr Fix16_13 (0 = no gate). */
int mkid_set_baseline(mkid_ctx* ctx, int32_t mode, int32_t alpha, int32_t kf, int32_t kq,
                      int32_t base_thr);

/* Trigger re-arm hysteresis (K7 state machine, build decision: the firmware is absent): after its
 * dead time a channel re-arms once e = f - baseline >= thr_c - floor(thr_c * frac_q8 / 256), i.e.
 * at a level moved from its threshold toward the baseline by frac_q8 / 256 (0..256). 0 (the
 * default) re-arms at the threshold, the round-1..4 rule, bit-identical. Without it a slow baseline
 * (SVF) lets the pulse tail re-cross the threshold after the dead time; the
 * reference's host replay holds off a fixed 1000 samples instead (pulse_triggering_v2.py:104-174).
 * Kept across mkid_set_thresholds (the levels follow the thresholds). */
int mkid_set_rearm(mkid_ctx* ctx, int32_t frac_q8);

/* Forget all stream state (PFB/FIR history, baselines, trigger state, sample counter). */
int mkid_reset_stream(mkid_ctx* ctx);

/* Process nsamples (multiple of N) I/Q pairs, host pointers, synchronous. phase_out (nullable)
 * receives [nsamples/N][C] float32 rad; events_out receives up to cap packets, channel-major and
 * time-ascending within a channel over the whole call (a call longer than cfg.max_chunk runs as
 * max_chunk pieces whose lists are merged on the host); *nevents = packets produced (> cap =>
 * MKID_E_OVERFLOW; the packets kept are then the first cap entries of the pieces' channel-major
 * lists concatenated in piece order: earlier pieces whole, the low channels of the piece that
 * overflows, nothing of later pieces; merged channel-major as above). */
int mkid_process(mkid_ctx* ctx, const int16_t* iq, int64_t nsamples, float* phase_out,
                 uint64_t* events_out, int64_t cap, int64_t* nevents);

/* Same with device pointers, asynchronous on the context stream; nsamples <= cfg.max_chunk (the
 * workspace size; MKID_E_ARG otherwise). d_counts is a device int64[2]: [0] = packets produced
 * (may exceed cap), [1] = packets written, channel-major and time-ascending within a channel over
 * the whole call. d_phase may be NULL (the phase stream is then not materialised; the trigger
 * still runs on the Fix16_13 phase). */
int mkid_process_device(mkid_ctx* ctx, const int16_t* d_iq, int64_t nsamples, float* d_phase,
                        uint64_t* d_events, int64_t cap, int64_t* d_counts /* [2] */);

/* K7 + K8 alone on caller-supplied Fix16_13 phase rows [rows][C] int16 (device pointer, e.g. a
 * snapshot uploaded by the caller: the reference runs its trigger on snapshots too,
 * ROACH_Pulses.py:211-354, 614-727): matched filter, baseline, trigger, packets, with the
 * context's carried trigger state and phase-sample counter (advanced by rows). rows <=
 * max_chunk/N. d_counts / packet order as mkid_process_device. Asynchronous on the context stream.
 * A context carries ONE stream: ADC samples (mkid_process*) or phase rows (this call). Calling one
 * kind after the other without mkid_reset_stream fails with MKID_E_STATE, so a snapshot never
 * advances the trigger state, the raw history or the packet stamps of a live ADC stream (use a
 * second context for snapshots taken beside a running feedline). */
int mkid_trigger_phase(mkid_ctx* ctx, const int16_t* d_raw, int64_t rows, uint64_t* d_events,
                       int64_t cap, int64_t* d_counts /* [2] */);

/* Fixed-point phase of the last processed call, [J][C] int16 Fix16_13 (the trigger's input),
 * device pointer valid until the next process call. Replaces the snapPhase_bram source
 * (ROACH_Pulses.py:357-378). */
int mkid_last_raw_phase(mkid_ctx* ctx, const int16_t** d_raw, int64_t* nrows);
/* Host copy of the same rows (at most cap_rows rows of C int16; *rows = rows available): the
 * snapshot readback (conv_phase_snapPhase_bram / qdr0 longsnapshot, ROACH_Pulses.py:433-551). */
int mkid_read_raw_phase(mkid_ctx* ctx, int16_t* host_out, int64_t cap_rows, int64_t* rows);

/* IQ snapshot tap (conv_phase_ch_we_IQ / conv_phase_snapIQ_bram, pulse_triggering_IQ.py:36,
 * 113-147): record the low-pass output y of one channel (channel < 0: off) for the rows of each
 * process call, as int16 I/Q pairs in ADC-count units (the units of mkid_avg_iq and the IQ
 * centres; saturated). mkid_read_iq_tap copies the last call's rows [rows][2] to the host. */
int mkid_set_iq_tap(mkid_ctx* ctx, int32_t channel);
int mkid_read_iq_tap(mkid_ctx* ctx, int16_t* host_iq, int64_t cap_rows, int64_t* rows);

/* Diagnostic: trigger segments of the last call whose speculative start state had to be
 * re-run by the exact fix-up pass (0 = all speculation was right; results are exact either way). */
int mkid_trigger_reruns(mkid_ctx* ctx, int64_t* total);

/* avgIQ accumulator (K9): replaces startAccumulator / avgIQ_ctrl (ROACH_Setup.py:654-659,
 * rotateLoopsReady). enable = 1 arms it — the sums restart on every call with 1, armed or not
 * (the avgIQ_ctrl strobe the reference writes before each startAccumulator 1) — and every
 * following process call adds its rows; 0 stops it and keeps the sums. Off after mkid_create; the
 * front ends skip the accumulation while it is off. mkid_reset_stream clears the sums and keeps
 * the armed state. */
int mkid_set_accumulator(mkid_ctx* ctx, int32_t enable);
/* Per-channel mean I/Q (low-pass output y, ADC-count units) over the rows accumulated since the
 * accumulator was last armed (avgIQ_bram, ROACH_Setup.py:654-662), [C] each. MKID_E_STATE when it
 * holds no rows, or when a process call failed while it was armed (its sums may hold part of that
 * call; re-arm to start a new average). */
int mkid_avg_iq(mkid_ctx* ctx, float* mean_i, float* mean_q);

/* Re-encode wide device packets as the reference 64-bit packet (host memory, C <= 254):
 *   [63:56] ch | [55:44] peak | [43:32] p1 = peak-base+2048 | [31:20] base | [19:0] ts mod 2^20
 * (ROACH_Pulses.py:805-832 decode; PacketMaster.c:291-292 assembly; ch 255 = end-of-second). */
int mkid_pack_reference(const uint64_t* wide, int64_t n, uint64_t* out);

/* Host-replay triggers of the reference on device phase. Input: Fix16_13
 * phase int16 [n][ld] (e.g. mkid_last_raw_phase, or snapshots uploaded by the caller), columns
 * 0..nch-1 are channels. Phase in degrees = raw*360/2^16*4/pi (pulse_triggering_v2.py:93-95).
 *   MKID_REPLAY_ROLLING  pulse_triggering_v2.py:104-174: start = 100+m, need = skip = pulselength,
 *                        length = m (meanlength, 20), |mean(x[j-m:j]) - x[j]| > threshold
 *   MKID_REPLAY_BLOCK    pulse_triggering.py:109-208 (start 100, need 300, skip 200, wrap on) and
 *                        ROACH_Pulses.py:614-727 (start 500): length = averagelength (2^k),
 *                        |mean(block(j)) - x[j]| > threshold
 * Hits (sample indices) go to d_hits[c*cap + i], i < cap; d_counts[c] = hits found (may exceed
 * cap: then hits were dropped). Means use numpy's pairwise float64 summation order, so the hit
 * lists equal the reference's numpy loops exactly. Runs on the context stream. */
#define MKID_REPLAY_ROLLING 0
#define MKID_REPLAY_BLOCK 1
typedef struct mkid_replay_cfg {
    int32_t mode;          /* MKID_REPLAY_ROLLING / MKID_REPLAY_BLOCK                       */
    int32_t length;        /* rolling: meanlength m; block: averagelength A                 */
    int32_t start;         /* first index tested ("bob")                                    */
    int32_t need;          /* stop when bob + need > n                                      */
    int32_t skip;          /* advance after a hit                                           */
    int32_t wrap_negative; /* add 360 deg to negative phase first (pulse_triggering.py:110)  */
    double threshold_deg;  /* strict: |mean - x| > threshold                                */
} mkid_replay_cfg;
int mkid_replay_trigger(mkid_ctx* ctx, const int16_t* d_raw, int64_t n, int64_t ld, int32_t nch,
                        const mkid_replay_cfg* cfg, int32_t* d_hits, int32_t cap, int32_t* d_counts);

/* Pulse template and near-optimal filter: MakeTemplate
 * (DataReadout/ReadoutControls/lib/pulses.py:239-427) on device for one resonator's pulses, the
 * reference's RawPulse rows I, Q float32 [npulses][2000] (pulses.py:30-43; not modified).
 * Outputs the PulseAnalysis fields (pulses.py:44-51): template [2000] f64 (deg-normalised,
 * peak at pstart), noise PSD [800] f64, and the scalars below. Fails with MKID_E_STATE when no
 * pulse survives the first pass or none survives the second; d_template, d_noise and info are
 * then left as they were. 1 <= npulses <= 2^31 - 1 (MKID_E_ARG otherwise). Device pointers for
 * the pulses, template and noise, a host pointer for info; complete on return.
 * The call is mkid_bank_filters' pipeline on one channel whose npulses records are all ready,
 * without the filter, and shares that call's workspace: the context keeps it after the call,
 * sized by the largest call of either kind so far (for this call 22 432 B per pulse plus 64.1 KB
 * of fixed tables; mkid_destroy frees it). */
typedef struct mkid_template_info {
    double count;   /* pulses in the final template (pass 2)                         */
    double count1;  /* pulses in the preliminary template (pass 1, first 1000 pulses) */
    double pm;      /* median of first-pass peaks > 15 deg (pulses.py:335)            */
    double pdev;    /* their std                                                      */
    int32_t flag;   /* 1 if count < 500 or pm < 10 or pm > 150 (pulses.py:409-412)    */
    int32_t pstart; /* index of the template maximum (pulses.py:415)                  */
} mkid_template_info;
int mkid_make_template(mkid_ctx* ctx, const float* d_I, const float* d_Q, int64_t npulses,
                       double* d_template, double* d_noise, mkid_template_info* info);
/* The optimal filter the reference stubs (pulses.py:398; PulseAnalysis.coeff Float32Col(100)):
 * correlation weights g = ifft(S / J) (S = fft of the 800-sample template window starting `pre`
 * samples before its peak, deg->rad; J = noise PSD; DC bin zeroed), normalised to unit response
 * to the template; d_coeff[0..ncoeff) = g[pre-10 ...]. Where the window leaves the record, its
 * samples outside [0, 2000) are zero, and so are the weights g[m] at m >= 800. 10 <= pre <= 2000,
 * 1 <= ncoeff <= 800. Device in, device out. */
int mkid_optimal_filter(mkid_ctx* ctx, const double* d_template, const double* d_noise, int32_t pre,
                        int32_t ncoeff, double* d_coeff);

/* Per-packet optimal-filter pulse height, fp32 (BASELINE config 5): the filter above (or any
 * per-channel FIR) applied to the phase stream at each photon packet,
 *     h = sum_{i < ncoeff} coeff[ch][i] * phase[ts - pre + i][ch]     (phase in rad)
 * the estimate the reference's PulseAnalysis.coeff was meant for (pulses.py:44-51, 398).
 * mkid_set_pulse_filter: host coeff [nch = C][ncoeff] fp32, 1 <= ncoeff <= 4096, 0 <= pre.
 * mkid_pulse_heights: d_phase holds the device phase rows of global phase indices
 * j0 .. j0 + rows - 1 ([rows][C], e.g. the d_phase of one mkid_process_device call; j0 = the
 * number of phase rows processed before it since the last reset); d_events n wide packets
 * (28-bit stamps unwrapped into [j0 - 2^27, j0 + 2^27)); d_heights n floats. The context keeps
 * the last ncoeff rows it was given: when a call's j0 continues the previous call's rows, windows
 * that start before row j0 read them. NaN where the window is not inside (carried rows, rows).
 * In a streamed run that is the packets of a call's last (ncoeff - pre) rows: pass them again
 * with the next contiguous call (j0 = this call's j0 + rows) and their windows are then complete
 * (carried rows + new rows); the heights of a call are otherwise final.
 * Asynchronous on the context stream; device pointers only. */
int mkid_set_pulse_filter(mkid_ctx* ctx, const float* coeff, int32_t nch, int32_t ncoeff, int32_t pre);
int mkid_pulse_heights(mkid_ctx* ctx, const float* d_phase, int64_t rows, int64_t j0,
                       const uint64_t* d_events, int64_t n, float* d_heights);
/* The same with the packet count read on the device: min(*d_count, cap) packets, e.g. d_count =
 * &d_counts[1] of the mkid_process_device call that wrote d_events (no host round trip). */
int mkid_pulse_heights_counted(mkid_ctx* ctx, const float* d_phase, int64_t rows, int64_t j0,
                               const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                               float* d_heights);
/* mkid_set_pulse_filter from a device table [nch = C][ncoeff] fp32, e.g. the d_coeff that
 * mkid_bank_filters wrote: one device-to-device copy on the context stream (so it follows whatever
 * that stream still has to write into the table), then one synchronisation, as the host form. The
 * same checks, and it resets the same state: the rows carried for mkid_pulse_heights and for
 * mkid_pulse_fit are forgotten. */
int mkid_set_pulse_filter_device(mkid_ctx* ctx, const float* d_coeff, int32_t nch, int32_t ncoeff,
                                 int32_t pre);

/* Pulse height with a lag search and a sub-sample arrival time: the filter of mkid_set_pulse_filter
 * applied at the 2 L + 1 alignments around the trigger's stamp, and the reference's peakfit
 * (Utils/bin.py:12-16, the 3-point parabolic vertex) on the best of them. Per packet, with ch, ts
 * and the unwrapped stamp jg exactly as for mkid_pulse_heights, r0 = jg - j0 - pre, search
 * half-width L and polarity s:
 *   lag values   H[d] = sum_{i < ncoeff} coeff[ch][i] * phase[r0 + d + i][ch],  d = -L .. L
 *   chosen lag   d* = the lowest d that maximises s H[d]
 *   edge         |d*| == L (always for L = 0): height = H[d*], dt = d*
 *   interior     y1, y2, y3 = s H[d*-1], s H[d*], s H[d*+1]; a = y2 - y1, b = y2 - y3, c = a + b;
 *                c == 0: height = H[d*], dt = d*; otherwise
 *                height = s (y2 + (a - b)^2 / (8 c)),  dt = d* + (a - b) / (2 c)   (|dt - d*| <= 1/2)
 *   outputs      d_heights [n] float; nullable d_dt [n] float (rows relative to the stamp: the
 *                arrival is jg + dt), d_lag [n] int32 (d*), d_h0 [n] float (H[0], the value
 *                mkid_pulse_heights gives)
 *   outside      a packet whose rows r0 - L .. r0 + L + ncoeff - 1 are not all inside (carried rows,
 *                rows), or whose ch >= C, gets NaN in every float output and INT32_MIN in d_lag
 * mkid_set_pulse_fit: 0 <= search <= 31 and polarity +1 or -1 (MKID_E_ARG otherwise). The fit
 * carries rows of its own, ncoeff + 2 search of them, apart from those of mkid_pulse_heights, which
 * behaves exactly as without the fit; both calls may be given the same rows. The call forgets the
 * fit's carried rows, and so does mkid_set_pulse_filter[_device], which also re-sizes them; the two
 * setters may come in either order.
 * mkid_pulse_fit: d_phase, rows, j0, d_events and n as for mkid_pulse_heights. When a call's j0
 * continues the previous call's rows, windows that start before row j0 read the carried rows. The
 * packets of a call's last (ncoeff - pre + L) rows come back NaN: pass them again with the next
 * contiguous call, as for mkid_pulse_heights; the outputs of a call are otherwise final. Every H[d]
 * is summed in an order that depends on ncoeff and L only, in fp32 with no atomics, and a carried
 * row holds the float it was given: a packet's outputs are the same bits from run to run and
 * whatever its place in the list, its neighbours, n, or the chunking of the stream into calls. A
 * non-finite phase inside a packet's window leaves that packet's outputs unspecified and touches no
 * other packet. Device pointers only; asynchronous on the context stream; no device-to-host copy
 * and no synchronisation; rows == 0 and n == 0 are valid. The counted form reads min(*d_count, cap)
 * packets and leaves the outputs of the others as they were. MKID_E_STATE when no filter is set or
 * before mkid_set_pulse_fit; MKID_E_ARG on a null required pointer (d_phase when rows > 0, d_events
 * and d_heights when n > 0, d_count) or a negative rows, j0 or n. Not timed (no MKID_K_ id).
 * mkid_pulse_fit_host: the same rule on host memory through the same definitions
 * (csrc/fit_common.h), H accumulated in float64; needs no device and no context. phase [rows][C]
 * float32 are global rows j0 .. j0 + rows - 1, coeff [C][ncoeff] float32; there are no carried
 * rows, so a window must lie inside the rows. Outputs float64 heights [n], nullable dt and h0 [n]
 * and int32 lag [n]. MKID_E_ARG: a null coeff, a null phase with rows > 0, null events or heights
 * with n > 0, negative rows, j0, n or pre, C outside 1..4096, ncoeff outside 1..4096, search outside
 * 0..31, polarity not +1 or -1. */
int mkid_set_pulse_fit(mkid_ctx* ctx, int32_t search, int32_t polarity);
int mkid_pulse_fit(mkid_ctx* ctx, const float* d_phase, int64_t rows, int64_t j0,
                   const uint64_t* d_events, int64_t n, float* d_heights, float* d_dt /* nullable */,
                   int32_t* d_lag /* nullable */, float* d_h0 /* nullable */);
int mkid_pulse_fit_counted(mkid_ctx* ctx, const float* d_phase, int64_t rows, int64_t j0,
                           const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                           float* d_heights, float* d_dt, int32_t* d_lag, float* d_h0);
int mkid_pulse_fit_host(const float* phase, int64_t rows, int32_t n_channels, int64_t j0,
                        const uint64_t* events, int64_t n, const float* coeff, int32_t ncoeff,
                        int32_t pre, int32_t search, int32_t polarity, double* heights,
                        double* dt /* nullable */, int32_t* lag /* nullable */, double* h0 /* nullable */);

/* The observing products after the heights: the per-second count image that the reference's
 * PacketMaster keeps as photon_counts[sec][pixel] (PacketMaster.c:371-381; the dashboard's quick-look
 * image), the per-channel pulse-height spectra, and the two list operations that keep the deferral
 * protocol of mkid_pulse_heights / mkid_pulse_fit on the device. All results are integers: they do
 * not depend on the order of the list, on the chunking of a stream into calls, or on the run. The
 * rules have one definition, csrc/obs_common.h. Per packet, ch and the unwrapped stamp jg are
 * exactly those of mkid_pulse_heights (base = max(j0 - 2^27, 0), jg = base + ((ts - base) mod 2^28)).
 *
 * mkid_count_photons: sec = (jg fft_len) / sample_rate in int64 integer division (the context's
 * configuration; phase row j is ADC sample j fft_len, and the first sample after a reset is a PPS
 * edge). image[sec][ch] += 1 for every packet with ch < C and sec < n_seconds; d_image is
 * [n_seconds][C] int32, caller-owned, zeroed by the caller to start an observation and continued
 * otherwise. d_outside int64[2], caller-owned likewise: [0] += packets with ch >= C (PacketMaster's
 * "photon from non-pixel"), [1] += packets with ch < C and sec >= n_seconds (PacketMaster ignores
 * seconds at or beyond exptime). Each packet is passed once, with the call that produced it (j0 =
 * that call's first global row). Correct for a list in any order; built for the device's order
 * (channel-major, time-ascending in a channel), where a cell's packets are one run and cost two
 * atomics together. MKID_E_ARG before any launch: a null d_image or d_outside, a null d_events with
 * n > 0, a null d_count, a negative n, cap or j0 (or one so large that jg fft_len leaves int64),
 * n_seconds outside 1 .. 2^20, a sample_rate that is not a positive integer below 2^53.
 *
 * mkid_height_spectra: spectra[ch][column] += 1 for every packet with ch < C; d_spectra is
 * [C][nbins + 3] int32, caller-owned as the image. The column of height h in channel ch, with the
 * device tables d_lo [C] and d_inv [C] (float32: lower edge of the first bin, 1 / bin width):
 *     t = h - lo[ch], u = t * inv[ch], each rounded once in fp32
 *     h not finite, or u NaN   -> nbins + 2  (no height)
 *     u < 0                    -> 0          (under)
 *     u >= (float)nbins        -> nbins + 1  (over)
 *     otherwise                -> 1 + (int)u
 * so -0.0 lands in column 1, and any lo / inv gives defined columns. Except a packet that is
 * deferred: d_deferred != NULL, its height is not finite and jg >= j_defer (the first stamp whose
 * window passes the call's last row: j0 + rows + pre - ncoeff - search + 1). Such a packet is
 * appended to d_deferred instead, in list order, at index d_ndef[1]; d_ndef int64[2], caller-owned:
 * [0] += packets that qualified, [1] += packets written (it stops at cap_def). Packets with ch >= C
 * touch nothing. So every packet with ch < C ends in exactly one column or in the deferred list.
 * MKID_E_ARG before any launch: a null d_lo, d_inv or d_spectra, null d_events or d_heights with
 * n > 0, a null d_count, a negative n, cap, j0 or cap_def, nbins outside 1 .. 16384, d_deferred
 * without d_ndef.
 *
 * mkid_concat_packets: d_out = the first min(*d_na, cap_a) words of d_a, then the first
 * min(*d_nb, cap_b) of d_b, cut at cap_out; d_nout int64[2] = {produced, written}. d_out overlaps
 * neither input; a list of capacity 0 may be NULL. MKID_E_ARG: a null count pointer, a negative
 * capacity, a null list with a capacity. A streamed step is then: count the call's packets; join
 * (deferred of the last step, the call's packets); one mkid_pulse_heights_counted or
 * mkid_pulse_fit_counted over the joined list; mkid_height_spectra_counted over it into the other
 * deferred list.
 *
 * Common to the five device calls: device pointers only; asynchronous on the context stream; no
 * device-to-host copy, and no synchronisation (mkid_height_spectra allocates two small tables on its
 * first call with d_deferred); n == 0 is valid; the counted forms read min(*d_count, cap) packets.
 * Not timed (no MKID_K_ id).
 * mkid_count_photons_host / mkid_height_spectra_host: the same rules on host memory through the
 * same definitions; no device, no context. The same MKID_E_ARG cases, and n_channels outside
 * 1 .. 4096 or fft_len < 1. */
int mkid_count_photons(mkid_ctx* ctx, const uint64_t* d_events, int64_t n, int64_t j0, int32_t n_seconds,
                       int32_t* d_image, int64_t* d_outside);
int mkid_count_photons_counted(mkid_ctx* ctx, const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                               int64_t j0, int32_t n_seconds, int32_t* d_image, int64_t* d_outside);
int mkid_height_spectra(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights, int64_t n, int64_t j0,
                        int64_t j_defer, const float* d_lo, const float* d_inv, int32_t nbins,
                        int32_t* d_spectra, uint64_t* d_deferred /* nullable */, int64_t cap_def,
                        int64_t* d_ndef /* nullable with d_deferred */);
int mkid_height_spectra_counted(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights,
                                const int64_t* d_count, int64_t cap, int64_t j0, int64_t j_defer,
                                const float* d_lo, const float* d_inv, int32_t nbins, int32_t* d_spectra,
                                uint64_t* d_deferred, int64_t cap_def, int64_t* d_ndef);
int mkid_concat_packets(mkid_ctx* ctx, const uint64_t* d_a, const int64_t* d_na, int64_t cap_a,
                        const uint64_t* d_b, const int64_t* d_nb, int64_t cap_b, uint64_t* d_out,
                        int64_t cap_out, int64_t* d_nout);
int mkid_count_photons_host(const uint64_t* events, int64_t n, int64_t j0, int32_t fft_len, double sample_rate,
                            int32_t n_channels, int32_t n_seconds, int32_t* image, int64_t* outside);
int mkid_height_spectra_host(const uint64_t* events, const float* heights, int64_t n, int64_t j0,
                             int64_t j_defer, int32_t n_channels, const float* lo, const float* inv,
                             int32_t nbins, int32_t* spectra, uint64_t* deferred /* nullable */,
                             int64_t cap_def, int64_t* ndef /* nullable with deferred */);

/* The time-tagged photon list: the reference's PacketMaster writes one variable-length row of
 * 64-bit packets per pixel per second (/r#/p#/t<obs>, PacketMaster.c:371-381, 978-1050) and keeps
 * at most MAX_EVENTS_PER_SEC - 1 = 2499 events in each (PacketMaster.c:55); the count image above
 * is that table's row lengths. Here the table is [n_seconds][C][K] on the device, 1 <= K <= 65536
 * chosen by the caller, filled inside the streamed step, with each photon's height (and arrival
 * offset) attached when the deferral protocol settles it. The rules have one definition,
 * csrc/obs_common.h; ch, jg and the cell (sec = (jg fft_len) / sample_rate) are those of
 * mkid_count_photons.
 *
 * mkid_list_photons: d_image and d_outside are updated exactly as mkid_count_photons updates them
 * (the call replaces that call in a step; both caller-owned and continued across calls). The
 * packets of cell (sec, ch) take slots in arrival order, starting at image[sec][ch] before the
 * call; a packet with slot < K stores
 *     d_words[sec][ch][slot]   the row word, by `layout`, with
 *                              us = (((jg fft_len) mod sample_rate) * 1000000) / sample_rate in int64
 *       MKID_ROW_WIDE       ch << 52 | peak << 40 | base << 28 | us   (the device packet with its
 *                           time field replaced; any C)
 *       MKID_ROW_REFERENCE  ch << 56 | peak << 44 | p1 << 32 | base << 20 | (us & 0xFFFFF),
 *                           p1 = clip(peak - base + 2048, 0, 4095): mkid_pack_reference's fields
 *                           (C <= 254)
 *     d_stamps[sec][ch][slot]  jg, the exact time tag and the key mkid_fill_photon_heights searches
 * and a packet with slot >= K is not stored and adds 1 to d_dropped int64[1] (the reference's
 * "first K kept"). Slots >= min(count, K) of a row are never written. d_words uint64 and d_stamps
 * int64 are [n_seconds][C][K], caller-owned. Each packet is passed once, with the call that
 * produced it, as for mkid_count_photons.
 *   - Device order (channel-major, stamp-ascending in a channel): a cell's packets are one
 *     contiguous run of the list, and row (sec, ch) holds that cell's packets of the whole stream
 *     in ascending stamp. Any chunking of a stream into calls, one-row calls included, gives the
 *     bits of one call over it.
 *   - Any other order: d_image, d_outside and d_dropped stay exact, and so does the set of (word,
 *     stamp) pairs of every row that did not overflow; but each maximal run of one cell in the
 *     list lands as a whole, and the runs of a cell in unspecified relative order (which packets
 *     of an overflowing row are the K kept is then unspecified too).
 * One integer atomic per run, no floating-point atomic; order comes from kernel boundaries. The
 * call's workspace (12 bytes per packet of n or cap) is the context's, grown on demand: allocate,
 * synchronise the stream once, move in; a call that does not grow it makes no synchronisation.
 * MKID_E_ARG before any launch: a null d_image, d_outside, d_words, d_stamps or d_dropped, a null
 * d_events with n > 0, a null d_count, a negative n, cap or j0 (or one so large that jg fft_len
 * leaves int64), n_seconds outside 1 .. 2^20, K outside 1 .. 65536, an unknown layout,
 * MKID_ROW_REFERENCE with C > 254, a sample_rate that is not a positive integer, or one above 2^43
 * (the product for us stays inside int64).
 *
 * mkid_fill_photon_heights: given the list and heights of a step's joined list (what
 * mkid_height_spectra is given; d_dt nullable, the second output of mkid_pulse_fit), for every
 * packet with ch < C that is not deferred (height finite, or jg < j_defer: the predicate of
 * mkid_height_spectra, so a packet is filled in exactly the step that bins it) jg is
 * binary-searched in d_stamps[sec][ch][0 .. min(image[sec][ch], K)). Found: the height (and dt,
 * with d_dt and d_row_dt) is copied into that slot of d_row_height (d_row_dt) bit for bit, NaN
 * included, and d_fill[0] += 1. Not found (sec >= n_seconds, or a packet its row dropped):
 * d_fill[1] += 1. Deferred packets and packets with ch >= C touch nothing. d_row_height float32
 * [n_seconds][C][K] and the nullable d_row_dt of the same shape are caller-owned and pre-filled by
 * the caller (with NaN); d_fill int64[2] is caller-owned and continued. Each row must be
 * stamp-ascending with distinct stamps: the device order of mkid_list_photons and a trigger with a
 * dead time give that. The result does not depend on the order of the list. No workspace.
 * MKID_E_ARG as for mkid_list_photons (n, cap, j0, n_seconds, K, sample_rate), and a null d_image,
 * d_stamps, d_row_height or d_fill, or null d_events or d_heights with n > 0.
 *
 * Common to the four device calls: device pointers only; asynchronous on the context stream; no
 * device-to-host copy; n == 0 is valid; the counted forms read min(*d_count, cap) packets. Not
 * timed (no MKID_K_ id).
 * mkid_list_photons_host / mkid_fill_photon_heights_host: the same rules on host memory through the
 * same definitions; no device, no context. The same MKID_E_ARG cases, and n_channels outside
 * 1 .. 4096 or fft_len < 1. */
#define MKID_ROW_WIDE 0
#define MKID_ROW_REFERENCE 1
int mkid_list_photons(mkid_ctx* ctx, const uint64_t* d_events, int64_t n, int64_t j0, int32_t n_seconds,
                      int32_t K, int32_t layout, int32_t* d_image, int64_t* d_outside, uint64_t* d_words,
                      int64_t* d_stamps, int64_t* d_dropped);
int mkid_list_photons_counted(mkid_ctx* ctx, const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                              int64_t j0, int32_t n_seconds, int32_t K, int32_t layout, int32_t* d_image,
                              int64_t* d_outside, uint64_t* d_words, int64_t* d_stamps, int64_t* d_dropped);
int mkid_fill_photon_heights(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights,
                             const float* d_dt /* nullable */, int64_t n, int64_t j0, int64_t j_defer,
                             int32_t n_seconds, int32_t K, const int32_t* d_image, const int64_t* d_stamps,
                             float* d_row_height, float* d_row_dt /* nullable */, int64_t* d_fill);
int mkid_fill_photon_heights_counted(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights,
                                     const float* d_dt, const int64_t* d_count, int64_t cap, int64_t j0,
                                     int64_t j_defer, int32_t n_seconds, int32_t K, const int32_t* d_image,
                                     const int64_t* d_stamps, float* d_row_height, float* d_row_dt,
                                     int64_t* d_fill);
int mkid_list_photons_host(const uint64_t* events, int64_t n, int64_t j0, int32_t fft_len, double sample_rate,
                           int32_t n_channels, int32_t n_seconds, int32_t K, int32_t layout, int32_t* image,
                           int64_t* outside, uint64_t* words, int64_t* stamps, int64_t* dropped);
int mkid_fill_photon_heights_host(const uint64_t* events, const float* heights, const float* dt /* nullable */,
                                  int64_t n, int64_t j0, int64_t j_defer, int32_t fft_len, double sample_rate,
                                  int32_t n_channels, int32_t n_seconds, int32_t K, const int32_t* image,
                                  const int64_t* stamps, float* row_height, float* row_dt /* nullable */,
                                  int64_t* fill);

/* The photon list as a streaming product of bounded memory: PacketMaster hands every finished
 * second to its writer and reuses the memory (PacketMaster.c:329-368, write_sec_data 978-1050).
 * Here the tables are a ring of n_slots second slots, [n_slots][C][K], a settled second is packed
 * into the reference's variable-length form on the device, and its slot is cleared for the second
 * n_slots later. The rules have one definition, csrc/obs_common.h (ring_cell, pack_host,
 * clear_host).
 *
 * mkid_list_photons_ring / mkid_fill_photon_heights_ring: the calls above with n_seconds replaced
 * by the window (sec0, n_slots, sec_end). A packet with ch < C and second sec belongs to slot
 * sec mod n_slots iff sec0 <= sec < min(sec0 + n_slots, sec_end); slot order, K, d_dropped, the
 * word by `layout` and the stamp are unchanged. d_outside is int64[4] here:
 *     [0] ch >= C            [1] sec >= sec_end (past the exposure)
 *     [2] sec < sec0 (its second was already drained)
 *     [3] sec0 + n_slots <= sec < sec_end (overrun: the ring is too short or was not drained)
 * and the fill counts a packet of any of the last three kinds in d_fill[1]. With sec0 = 0 and
 * n_slots = sec_end = n_seconds every output equals the plain call's bit for bit and
 * d_outside[2 .. 3] stay 0. The caller moves sec0 past a second only after mkid_clear_second of it.
 * MKID_E_ARG as for the plain calls, with, in place of n_seconds: n_slots outside 1 .. 2^20,
 * sec0 < 0, sec0 > sec_end, or sec_end so large that (sec_end + 1) sample_rate leaves int64.
 *
 * mkid_pack_second: reads slot s = sec mod n_slots and writes none of the tables. With
 * m_c = min(image[s][c] as uint32, K), the photons row c holds:
 *     d_counts[c]   int32 [C]      image[s][c], the raw count (PacketMaster's image row)
 *     d_offsets[c]  int64 [C + 1]  the exclusive prefix sum of m_c; d_offsets[C] is the total
 *     entry i < m_c of row c of d_words, d_stamps, d_row_height and d_row_dt goes to index
 *     d_offsets[c] + i of d_out_words, d_out_stamps, d_out_height and d_out_dt, bit for bit (NaN
 *     payloads included), when that index is < cap_out
 *     d_total       int64 [2]      {d_offsets[C], min(d_offsets[C], cap_out)}
 * Output entries at or beyond d_total[1] are never written. d_out_stamps may be NULL (then so may
 * d_stamps); d_out_dt may be NULL, and must be with a NULL d_row_dt; with cap_out = 0 the four
 * outputs may be NULL. It also serves the unbounded tables (n_slots = n_seconds). One workgroup
 * scans the C counts, then a wave copies each (channel, tile of 256 slots) that holds photons; no
 * atomics, no workspace.
 * mkid_clear_second: for every c the first m_c entries of row c of d_row_height (and of d_row_dt,
 * nullable) get the bit pattern 0x7FC00000, the NaN the tables are pre-filled with; then
 * image[s][c] = 0. Words, stamps and slots at or beyond m_c are not touched.
 * MKID_E_ARG before any launch: sec < 0, n_slots outside 1 .. 2^20, K outside 1 .. 65536, a
 * negative cap_out, a null d_image, d_words, d_row_height, d_counts, d_offsets or d_total, null
 * d_out_words or d_out_height with cap_out > 0, d_out_stamps without d_stamps, d_out_dt without
 * d_row_dt.
 *
 * Common to the six device calls: device pointers only; asynchronous on the context stream; no
 * device-to-host copy and no synchronisation (the list's workspace as above). Not timed.
 * The four _host twins: the same rules on host memory through the same definitions; the same
 * MKID_E_ARG cases, and n_channels outside 1 .. 4096 or fft_len < 1. */
int mkid_list_photons_ring(mkid_ctx* ctx, const uint64_t* d_events, int64_t n, int64_t j0, int64_t sec0,
                           int32_t n_slots, int64_t sec_end, int32_t K, int32_t layout, int32_t* d_image,
                           int64_t* d_outside, uint64_t* d_words, int64_t* d_stamps, int64_t* d_dropped);
int mkid_list_photons_ring_counted(mkid_ctx* ctx, const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                                   int64_t j0, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                   int32_t layout, int32_t* d_image, int64_t* d_outside, uint64_t* d_words,
                                   int64_t* d_stamps, int64_t* d_dropped);
int mkid_fill_photon_heights_ring(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights,
                                  const float* d_dt /* nullable */, int64_t n, int64_t j0, int64_t j_defer,
                                  int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K, const int32_t* d_image,
                                  const int64_t* d_stamps, float* d_row_height, float* d_row_dt /* nullable */,
                                  int64_t* d_fill);
int mkid_fill_photon_heights_ring_counted(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights,
                                          const float* d_dt, const int64_t* d_count, int64_t cap, int64_t j0,
                                          int64_t j_defer, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                          const int32_t* d_image, const int64_t* d_stamps, float* d_row_height,
                                          float* d_row_dt, int64_t* d_fill);
int mkid_pack_second(mkid_ctx* ctx, int64_t sec, int32_t n_slots, int32_t K, const int32_t* d_image,
                     const uint64_t* d_words, const int64_t* d_stamps, const float* d_row_height,
                     const float* d_row_dt /* nullable */, int64_t cap_out, int32_t* d_counts, int64_t* d_offsets,
                     uint64_t* d_out_words, int64_t* d_out_stamps /* nullable */, float* d_out_height,
                     float* d_out_dt /* nullable with d_row_dt */, int64_t* d_total);
int mkid_clear_second(mkid_ctx* ctx, int64_t sec, int32_t n_slots, int32_t K, int32_t* d_image, float* d_row_height,
                      float* d_row_dt /* nullable */);
int mkid_list_photons_ring_host(const uint64_t* events, int64_t n, int64_t j0, int32_t fft_len, double sample_rate,
                                int32_t n_channels, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                int32_t layout, int32_t* image, int64_t* outside, uint64_t* words, int64_t* stamps,
                                int64_t* dropped);
int mkid_fill_photon_heights_ring_host(const uint64_t* events, const float* heights, const float* dt /* nullable */,
                                       int64_t n, int64_t j0, int64_t j_defer, int32_t fft_len, double sample_rate,
                                       int32_t n_channels, int64_t sec0, int32_t n_slots, int64_t sec_end, int32_t K,
                                       const int32_t* image, const int64_t* stamps, float* row_height,
                                       float* row_dt /* nullable */, int64_t* fill);
int mkid_pack_second_host(int64_t sec, int32_t n_slots, int32_t K, int32_t n_channels, const int32_t* image,
                          const uint64_t* words, const int64_t* stamps, const float* row_height,
                          const float* row_dt /* nullable */, int64_t cap_out, int32_t* counts, int64_t* offsets,
                          uint64_t* out_words, int64_t* out_stamps /* nullable */, float* out_height,
                          float* out_dt /* nullable with row_dt */, int64_t* total);
int mkid_clear_second_host(int64_t sec, int32_t n_slots, int32_t K, int32_t n_channels, int32_t* image,
                           float* row_height, float* row_dt /* nullable */);

/* Energy calibration from laser spectra, and the energy cube. A pulse height is in the units of its
 * channel's filter output; the laser box (ArconsDashboard.py toggle_laser / do_cal) puts P <= 3 lines
 * of known energy into every channel's pulse-height spectrum, and their positions give the channel's
 * height -> energy polynomial and its resolving power. The quick-look (ArconsDashboard.py
 * image_Worker, :1282-1505) consumes ten energy or wavelength slices per pixel (data.bin). The rules
 * have one definition, csrc/wavecal_common.h; the kernels are csrc/k_wavecal.hip.
 *
 * mkid_spectrum_lines: every channel's lines found and fitted in one call. d_spectra int32
 * [nch][nbins + 3] is the table of mkid_height_spectra, of which only columns 1 .. nbins are read, a
 * count n[b] taken as (int64)(uint32); it is never written. d_lo, d_step float32 [nch]: bin b of a
 * channel starts at lo + b step. nbins 1 .. 16384; n_lines P 1 .. 3; energies (host memory, double
 * [P], eV): energies[p] belongs to the p-th chosen line in ascending bin order (give them descending
 * where heights are negative); smooth w 0 .. 64; min_sep >= 1 bins; min_peak any int64; fit_half g
 * 1 .. 64. Per channel, from its own row and these parameters alone:
 *   Integer part (exact: device, host twin and any restatement agree bit for bit).
 *     s[b] = sum_{k = -w .. w} (w + 1 - |k|) n[b + k] in int64, n = 0 outside 0 .. nbins - 1 and
 *     s = 0 outside too. Bin b is a candidate when s[b] >= min_peak, s[b] > s[b - 1] and
 *     s[b] >= s[b + 1] (a plateau's lowest bin). Lines are chosen greedily by descending s, ties to
 *     the lower bin, skipping a candidate with |b - b'| < min_sep of a chosen b', until P are chosen
 *     or no candidate is left; the chosen lines are then sorted by ascending bin. The fit window of
 *     line p at bin m is max(m - g, L) .. min(m + g, H), L = floor((m_prev + m) / 2) + 1 (0 for the
 *     first line), H = floor((m + m_next) / 2) (nbins - 1 for the last found line); only its bins
 *     with n >= 1 are used. mkid_line_fit: bin = m, peak_s = s[m], nfit = bins used, counts = sum of
 *     n over the window.
 *   Float64 part (Caruana's log-parabola with n^2 weights). Per used bin x = (double)(b - m),
 *     W = (double)n (double)n, y = log((double)n); with W x^k built as ((W x) x) .., the sums
 *     S_k = sum W x^k (k = 0 .. 4) and T_k = sum (W x^k) y (k = 0 .. 2) are accumulated in ascending
 *     b by one thread, every product and sum one IEEE operation, never fused. The normal system
 *     [S0 S1 S2; S1 S2 S3; S2 S3 S4] a = T is solved by the cofactor expansion written in
 *     wavecal_common.h solve3. With a2 < 0: mu_x = -a1 / (2 a2), sigma_x = sqrt(-1 / (2 a2)),
 *     amp = exp(a0 - a1^2 / (4 a2)); in height units mu = (double)lo + ((double)m + 0.5 + mu_x)
 *     (double)step and sigma = sigma_x |step|. A line's fit failed when nfit < 3, a2 >= 0 (or NaN),
 *     a value is not finite, or |mu_x| > g: mu, sigma and amp are then NaN. Device, host twin and
 *     a float64 restatement differ only through log (and exp, in amp).
 *   Calibration, only when all P lines were found and fitted: E(h) = c0 + c1 h + c2 h^2 through
 *     the points (mu_p, energies[p]): P = 1 c1 = E1 / mu1; P = 2 the line through both; P = 3 the
 *     parabola by Newton's divided differences expanded in the order written in wavecal_common.h
 *     calibrate. Resolving power R_p = E_p / (2.3548200450309493 |c1 + 2 c2 mu_p| sigma_p).
 *   status (mkid_energy_cal): MKID_CAL_FEW_LINES fewer than P lines found; MKID_CAL_FIT_FAILED << p
 *     the fit of found line p failed; MKID_CAL_BAD_SLOPE dE/dh = c1 + 2 c2 mu changes sign between
 *     the first and the last line, or is zero or not finite at a line (or c0 is not finite). With any
 *     bit set c[] and r[] are NaN; r[p] is NaN for p >= P as well. A line not found has bin = -1,
 *     nfit = counts = peak_s = 0 and NaN floats. n_found = lines found.
 *   Outputs: d_lines mkid_line_fit [nch][P]; d_cal mkid_energy_cal [nch]; d_cal_f float32 [nch][4] =
 *     (float)c0, (float)c1, (float)c2, and 1.0f (status 0) or 0.0f: the table mkid_energy_cube reads.
 * One workgroup per channel with the row staged in LDS (4 nbins bytes), s recomputed from it, the
 * selection P rounds of a workgroup arg-max without atomics, the fits on one lane per line. Device
 * pointers only (energies excepted); asynchronous on the context stream; no device-to-host copy, no
 * synchronisation, no workspace; nch >= 1 need not equal C. Not timed. MKID_E_ARG before any launch:
 * a null pointer, nch < 1, a parameter outside the ranges above, energies that are not finite and
 * positive or not distinct.
 * mkid_spectrum_lines_host: the same rules on host memory through the same definitions; no device,
 * no context. The same MKID_E_ARG cases.
 *
 * mkid_energy_cube: the list, j0, j_defer and d_heights are exactly those of mkid_height_spectra.
 * d_cal_f float32 [C][4] as above; mode MKID_CUBE_ENERGY or MKID_CUBE_WAVELENGTH; hc, vlo, vinv
 * float32; nb 1 .. 16384 bins; d_cube int32 [C][nb + 3], caller-owned, zeroed by the caller to start
 * and continued across calls; d_energy float32 [n], nullable. Per packet with ch < C:
 *     e = c0 + h (c1 + h c2), each operation rounded once in fp32; the NaN 0x7FC00000 where the
 *         channel's fourth entry is 0.0f, where h is not finite, or where the arithmetic gives NaN
 *     d_energy[p] = e (packets with ch >= C leave their entry untouched)
 *     a packet whose height is not finite and whose jg >= j_defer is skipped here (it comes again
 *         with the next call's list; j_defer = INT64_MAX skips none)
 *     otherwise v = e (energy mode) or hc / e rounded once in fp32 (wavelength mode), and
 *         cube[ch][column(v, vlo, vinv, nb)] += 1 with the column rule of mkid_height_spectra
 *         (t = v - vlo, u = t vinv): +-inf and NaN (no energy, e = 0 in wavelength mode) land in
 *         column nb + 2, values below vlo (a negative wavelength among them) in column 0.
 * The list is only read, so the call composes with mkid_height_spectra over the same list in either
 * order; every packet with ch < C ends in exactly one cube column over the stream, and a row's total
 * equals the spectra row's total. Run-length form as mkid_count_photons: two atomics per run of
 * equal cells in the device's order, correct for any order; only integers are accumulated, so the
 * cube does not depend on order, chunking or run. Device pointers only; asynchronous on the context
 * stream; no copy, no synchronisation, no workspace; n == 0 is valid; the counted form reads
 * min(*d_count, cap) packets. Not timed. MKID_E_ARG before any launch: a null d_cal_f or d_cube, null
 * d_events or d_heights with n > 0, a null d_count, a negative n, cap or j0, an unknown mode, nb
 * outside 1 .. 16384.
 * mkid_energy_cube_host: the same rules on host memory; the same MKID_E_ARG cases, and n_channels
 * outside 1 .. 4096. */
#define MKID_CAL_MAX_LINES 3
#define MKID_CAL_FEW_LINES 1
#define MKID_CAL_FIT_FAILED 2   /* << p for line p: 2, 4, 8 */
#define MKID_CAL_BAD_SLOPE 16
#define MKID_CUBE_ENERGY 0
#define MKID_CUBE_WAVELENGTH 1
typedef struct mkid_line_fit {
    int32_t bin, nfit;
    int64_t peak_s, counts;
    double mu, sigma, amp;
} mkid_line_fit;
typedef struct mkid_energy_cal {
    double c[3], r[3];
    int32_t n_found, status;
} mkid_energy_cal;
int mkid_spectrum_lines(mkid_ctx* ctx, const int32_t* d_spectra, const float* d_lo, const float* d_step, int32_t nch,
                        int32_t nbins, int32_t n_lines, const double* energies /* host */, int32_t smooth,
                        int32_t min_sep, int64_t min_peak, int32_t fit_half, mkid_line_fit* d_lines,
                        mkid_energy_cal* d_cal, float* d_cal_f);
int mkid_spectrum_lines_host(const int32_t* spectra, const float* lo, const float* step, int32_t nch, int32_t nbins,
                             int32_t n_lines, const double* energies, int32_t smooth, int32_t min_sep,
                             int64_t min_peak, int32_t fit_half, mkid_line_fit* lines, mkid_energy_cal* cal,
                             float* cal_f);
int mkid_energy_cube(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights, int64_t n, int64_t j0,
                     int64_t j_defer, const float* d_cal_f, int32_t mode, float hc, float vlo, float vinv, int32_t nb,
                     int32_t* d_cube, float* d_energy /* nullable */);
int mkid_energy_cube_counted(mkid_ctx* ctx, const uint64_t* d_events, const float* d_heights, const int64_t* d_count,
                             int64_t cap, int64_t j0, int64_t j_defer, const float* d_cal_f, int32_t mode, float hc,
                             float vlo, float vinv, int32_t nb, int32_t* d_cube, float* d_energy /* nullable */);
int mkid_energy_cube_host(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int64_t j_defer,
                          int32_t n_channels, const float* cal_f, int32_t mode, float hc, float vlo, float vinv,
                          int32_t nb, int32_t* cube, float* energy /* nullable */);

/* Resonator loop fits: every channel's swept IQ loop fitted with the ten-parameter model of the
 * reference's IQsweep.FitLoopMP (lib/iqsweep.py:141-291, RESDIFF :824-858) in one call, giving Q, f0,
 * the loop centre (p[8], p[9]), Qc, Qi and the dip depth per channel. Kept from the reference: the
 * model, the window, the guesses, the bounds, the start recipe, "the lowest chi^2 of S starts wins"
 * and the derived quantities. The optimiser is this library's own definition, not mpfit (finite
 * differences, an unseeded generator) and not FitLoopMP's slips (:231 raises, :211 re-slices the
 * windowed array). The rules have one definition, csrc/loopfit_common.h; the kernel is
 * csrc/k_loopfit.hip. All data are float64.
 *
 * mkid_fit_loops. d_freq, d_i, d_q [nch][fsteps]: a channel's frequencies in Hz and its I and Q with
 * the zero point already subtracted. d_isd, d_qsd [nch][fsteps], both or neither: weights wI = 1 /
 * isd, wQ = 1 / qsd (1 when null). d_draws [nch][S][5]: the random numbers of :236-244 for start s, g
 * (standard normal), u2, u3, u4 in [0, 1), u5 in [-1, 1); the caller supplies them, so the call is a
 * pure function of its arguments. d_qguess [nch], nullable: a Q from elsewhere (mkid_fit_mags' d_qout).
 * fsteps 12 .. 1024, n_starts S 1 .. 16, max_iter >= 1, ftol > 0. Per channel, integer division:
 *   Window (bit-identical on device, host twin and any restatement: +, -, x, sqrt, comparisons).
 *     v[i] = sqrt((I[i] - I[i+1])^2 + (Q[i] - Q[i+1])^2), i = 0 .. nv - 1, nv = fsteps - 2 (the last
 *     difference is dropped, as the reference does). The smoothed velocity is smooth() of :919-971:
 *     with top = min(10, nv - 1) the padded signal is s = [2 v[0] - v[top - t] (t = 0 .. top - 2), v,
 *     2 v[nv-1] - v[nv-1-t] (t = 0 .. 8)] and sv[i] = sum_{j = 0 .. 9} wn[j] s[i + 13 - j], added in
 *     ascending j from 0.0, i = 0 .. top + nv - 11; wn = hanning(10) / sum is made by the host entry
 *     (w[j] = 0.5 + 0.5 cos(pi (2 j - 9) / 9), the sum ascending) and handed to the kernel. cidx =
 *     the first index of the maximum of sv (found with > from sv[0]); low = max(cidx - fsteps / 4,
 *     0), high = min(cidx + fsteps / 4, fsteps), n = high - low points low .. high - 1.
 *   Guesses over the window, by one thread in ascending order: Iceng = (max I - min I) / 2 + min I,
 *     Qceng alike; gI = max I - min I and gQ alike over the whole window (the reference's :211
 *     re-slice is not kept); ang = atan2(Q[cidx] - Qceng, I[cidx] - Iceng), then ang - pi / 2 when
 *     ang >= 0, else ang + pi / 2.
 *   Bounds: Q [5e3, 1e6]; f0 [min x, max x]; aleak [1e-4, 1e2]; ph1 [1, 4e4]; da [-5e3, 5e3]; ang1
 *     +-1.1 pi; Igain gI -+ 0.5 gI; Qgain [gQ - 0.5 gQ, gQ + 0.5 gI] (:215 as written); Ioff Iceng -+
 *     0.5 |Iceng|; Qoff Qceng -+ 0.5 |Qceng|. A parameter with lo == hi is held fixed.
 *   Start s: Q = max(q_s + 20000 g, 5000) with q_s = d_qguess[c], else 10000 s; aleak = 1.1e-4 + 90
 *     u2; ph1 = 1 + 3e4 u3; da = 9000 u4 - 4500; ang1 = ang for s <= 5, else pi u5; f0 = (sum of x,
 *     ascending) / n; gains and offsets the guesses; every value clipped into its bounds.
 *   Model at x: dx = (x - f0) / f0, t = 2 Q dx, den = 1 + t^2, ph = dx ph1,
 *     re = (da dx + (t^2 / den - 0.5)) + aleak (1 - cos ph), im = t / den - aleak sin ph,
 *     Ix = re Igain, Qx = im Qgain, mI = (Ix cos ang1 + Qx sin ang1) + Ioff,
 *     mQ = (Qx cos ang1 - Ix sin ang1) + Qoff. Residuals rI = (I - mI) wI, rQ = (Q - mQ) wQ; chi^2 =
 *     sum r^2; J = w d(model)/dp analytic, written once in loopfit_common.h point_terms.
 *   Sums: the 55 entries of A = J^T J (lower triangle), the 10 of g = J^T r and chi^2 are 64 lane
 *     partials, lane l taking points l, l + 64, .. in ascending order, I half then Q half of each
 *     point; they combine by the butterfly p[l] = p[l] + p[l ^ m], m = 32, 16, .., 1. Every product
 *     and sum is one IEEE operation, never fused.
 *   Solver per start: lambda = 1e-3; D = diag A. The free set is the parameters with hi > lo and D >
 *     0; (A + lambda diag D) delta = g on the free set by the Cholesky written in lm_common.h
 *     step; a pivot that is not positive and finite: lambda x= 10 and retry. trial = clip(p + delta).
 *     Accept when chi^2(trial) is finite and smaller: lambda = max(lambda / 10, 1e-12), and stop when
 *     (chi^2 - chi^2(trial)) / chi^2 <= ftol. Otherwise lambda x= 10. Stop when lambda > 1e12, when
 *     the free set is empty, or when the start has made max_iter model evaluations (the first, at
 *     the start itself, included). A start whose first chi^2 is not finite ends there.
 *   Result: the start with the lowest finite chi^2, ties to the lower s. rad = |p6 + p7| / 4, diam = 2
 *     rad / (sqrt(p8^2 + p9^2) + rad), qc = p0 / diam, qi = p0 / (1 - diam), dipdb = 20 log10(1 -
 *     diam). evals = the best start's model evaluations. status bits: MKID_LOOP_NONFINITE a value of
 *     x, I, Q, wI or wQ in the window is not finite; MKID_LOOP_FLAT gI or gQ is 0; MKID_LOOP_NO_FIT no
 *     start reached a finite chi^2; MKID_LOOP_MAX_ITER the best start stopped on max_iter. With any
 *     of the first three every float is NaN, best_start = -1 and evals = 0. cidx, low, high and n are
 *     always set. d_chisq_all [nch][S], nullable: every start's final chi^2 (NaN for a channel with
 *     one of the first two bits).
 * Device, host twin and a float64 restatement differ only through sin, cos, atan2 and log10. One
 * workgroup of 256 threads per channel, the window staged in LDS once, one wave per start, the
 * butterfly by __shfl_xor, the Cholesky on one lane, the best start chosen through LDS without
 * atomics. Device pointers only; asynchronous on the context stream; no copy, no synchronisation, no
 * workspace. Not timed. MKID_E_ARG before any launch: a null pointer (d_qguess and d_chisq_all
 * excepted), only one of d_isd and d_qsd, a parameter outside the ranges above.
 * mkid_fit_loops_host: the same rules on host memory through the same definitions; no device, no
 * context. The same MKID_E_ARG cases. */
#define MKID_LOOP_NPAR 10
#define MKID_LOOP_NONFINITE 1
#define MKID_LOOP_FLAT 2
#define MKID_LOOP_NO_FIT 4
#define MKID_LOOP_MAX_ITER 8
typedef struct mkid_loop_fit {
    double p[MKID_LOOP_NPAR];   /* Q, f0, aleak, ph1, da, ang1, Igain, Qgain, Ioff, Qoff */
    double chisq, qc, qi, dipdb;
    int32_t cidx, low, high, n, best_start, evals, status, pad;
} mkid_loop_fit;
int mkid_fit_loops(mkid_ctx* ctx, const double* d_freq, const double* d_i, const double* d_q,
                   const double* d_isd /* nullable with d_qsd */, const double* d_qsd, const double* d_draws,
                   const double* d_qguess /* nullable */, int32_t nch, int32_t fsteps, int32_t n_starts,
                   int32_t max_iter, double ftol, mkid_loop_fit* d_fits, double* d_chisq_all /* nullable */);
int mkid_fit_loops_host(const double* freq, const double* i, const double* q, const double* isd, const double* qsd,
                        const double* draws, const double* qguess, int32_t nch, int32_t fsteps, int32_t n_starts,
                        int32_t max_iter, double ftol, mkid_loop_fit* fits, double* chisq_all);

/* Resonator magnitude fits: every channel's swept |S21| fitted with the six-parameter model of the
 * reference's IQsweep.FitMagMP (lib/iqsweep.py:293-356, MAGDIFF :913-917) in one call, giving Q and f0
 * from the magnitude alone, the parameters Pdf() plots as mopt / magfit, and the Q that seeds the
 * loop fit's starts (:227-231): d_qout is a valid d_qguess of mkid_fit_loops on the same stream. Kept
 * from the reference: the model, the normalisation, the error 1e-5, the bounds, the start recipe and
 * "the lowest chi^2 wins". The optimiser is mkid_fit_loops' own, with one definition for both fits
 * (csrc/lm_common.h step and run_start at N parameters). The rules have one definition,
 * csrc/magfit_common.h; the kernel is csrc/k_magfit.hip. All data are float64.
 *
 * mkid_fit_mags. d_freq, d_i, d_q [nch][fsteps]: a channel's frequencies in Hz and its I and Q with
 * the zero point already subtracted. d_draws [nch][S]: the standard normal g of :335 for start s; the
 * caller supplies it, so the call is a pure function of its arguments. fsteps 12 .. 1024, n_starts S
 * 1 .. 16, max_iter >= 1, ftol > 0. Per channel, over the whole sweep (there is no window):
 *   Data: mag[i] = sqrt(I[i] I[i] + Q[i] Q[i]); norm = the maximum of mag, found with > from mag[0]
 *     (a NaN never wins; a NaN at mag[0] stays); y[i] = mag[i] / norm; w = 1 / 1e-5 for every point.
 *     cidx = mkid_fit_loops' cidx, the first index of the maximum of the smoothed IQ velocity, by the
 *     same functions (the reference's vmaxidx); the fit does not use it.
 *   Bounds: Q [5e3, 1e6]; f0 [min x, max x]; carrier [1e-4, 1e2]; depth [0.01, 10]; slope [-5e3, 5e3];
 *     curve [-1e8, 1e8]. A parameter with lo == hi is held fixed.
 *   Start s: Q = max(10000 s + 5000 g, 5000), g = d_draws[c][s]; f0 = (sum of x, ascending) / fsteps;
 *     carrier 1.0, depth 0.7, slope 0.1, curve -10; every value clipped into its bounds.
 *   Model at x: dx = (x - f0) / f0, t = (2 Q) dx, den = 1 + t t, r = sqrt(den), a = |t| / r,
 *     m = (((a - 1) depth + carrier) + slope dx) + (curve dx) dx. Residual res = (y - m) w; chi^2 = sum
 *     res^2. No sin, cos or atan2: +, -, x, /, sqrt, |.| and comparisons only.
 *   Jacobian: sg = (t > 0) - (t < 0), 0 at the cusp t = 0; k = sg / (den r); ddx = -x / (f0 f0);
 *     dk = depth k; J = [w (dk (2 dx)), w (ddx (((dk (2 Q)) + slope) + (2 curve) dx)), w, w (a - 1),
 *     w dx, w (dx dx)], every product and sum in the order of the brackets.
 *   Sums: the 21 entries of A = J^T J (lower triangle), the 6 of g = J^T res and chi^2 are 64 lane
 *     partials, lane l taking points l, l + 64, .. in ascending order, per point chi^2 first, then g_i
 *     and A_ij (j <= i) by ascending i, j; they combine by the butterfly p[l] = p[l] + p[l ^ m], m =
 *     32, 16, .., 1. Every product and sum is one IEEE operation, never fused.
 *   Solver per start, accept rule, stop rules and winner: those of mkid_fit_loops word for word, at
 *     six parameters (lambda = 1e-3, D = diag A, the free set hi > lo and D > 0, the Cholesky, trial =
 *     clip(p + delta), accept a finite smaller chi^2 with lambda = max(lambda / 10, 1e-12) and stop at
 *     a relative gain <= ftol, else lambda x= 10; stop at lambda > 1e12, an empty free set or max_iter
 *     model evaluations; the lowest finite chi^2 wins, ties to the lower s).
 *   Result: p, chisq, norm, cidx, best_start, evals = the best start's model evaluations. status bits,
 *     with mkid_fit_loops' values: MKID_LOOP_NONFINITE a value of x, I or Q anywhere in the sweep is
 *     not finite; MKID_LOOP_FLAT norm == 0; MKID_LOOP_NO_FIT no start reached a finite chi^2;
 *     MKID_LOOP_MAX_ITER the best start stopped on max_iter. With any of the first three every float
 *     but norm is NaN, best_start = -1 and evals = 0. cidx and norm are always set.
 *   d_qout [nch], nullable: p[0] of a fitted channel, 50000.0 (FitLoopMP's own default Q, :193) for a
 *     channel with one of the first three bits, so that the array is always a valid d_qguess.
 *   d_chisq_all [nch][S], nullable: every start's final chi^2 (NaN for a channel with one of the
 *     first two bits).
 * Device, host twin and a float64 restatement agree in every bit; the bits do not depend on the
 * launch shape. One workgroup per channel of min(S, 8) waves, the sweep's x and y staged in LDS once
 * (the velocity scratch uses the same rows first), norm by a parallel maximum, one wave per start,
 * the butterfly by __shfl_xor, the Cholesky on one lane, the best start chosen through LDS without
 * atomics. Device pointers only; asynchronous on the context stream; no copy, no synchronisation, no
 * workspace. Not timed. MKID_E_ARG before any launch: a null pointer (d_qout and d_chisq_all
 * excepted), a parameter outside the ranges above.
 * mkid_fit_mags_host: the same rules on host memory through the same definitions; no device, no
 * context. The same MKID_E_ARG cases. */
#define MKID_MAG_NPAR 6
typedef struct mkid_mag_fit {
    double p[MKID_MAG_NPAR];   /* Q, f0, carrier, depth, slope, curve */
    double chisq, norm;
    int32_t cidx, best_start, evals, status;
} mkid_mag_fit;
int mkid_fit_mags(mkid_ctx* ctx, const double* d_freq, const double* d_i, const double* d_q, const double* d_draws,
                  int32_t nch, int32_t fsteps, int32_t n_starts, int32_t max_iter, double ftol, mkid_mag_fit* d_fits,
                  double* d_qout /* nullable */, double* d_chisq_all /* nullable */);
int mkid_fit_mags_host(const double* freq, const double* i, const double* q, const double* draws, int32_t nch,
                       int32_t fsteps, int32_t n_starts, int32_t max_iter, double ftol, mkid_mag_fit* fits, double* qout,
                       double* chisq_all);

/* Pulse capture: the firmware-style capture block between the stream and the template analysis.
 * For every photon packet the phase window around its stamp is copied into a caller-owned,
 * per-channel record bank on the device, for all channels at once and across streamed calls (the
 * scale-up of contsnapshot's one-channel host cut, ROACH_Pulses.py:557-762; window saving of
 * pulse_triggering_v2.py:104-174). A channel's records [P][length] then feed mkid_make_template.
 * mkid_set_capture: 1 <= length <= 4096 rows per record, 0 <= pre < length rows before the stamp,
 * max_per_ch >= 1 records per channel (R); it (re)allocates the context's capture state and starts
 * a new stream segment.
 * mkid_capture_pulses: d_phase [rows][C] are global phase rows j0 .. j0 + rows - 1 (as for
 * mkid_pulse_heights), d_events the n wide packets of that call (channel-major, time-ascending in
 * a channel, each passed exactly once, with the call that produced it). Bank: d_records
 * [C][R][length] float32, d_stamps [C][R] int64, d_info [C][2] int32 {ready, dropped}; the caller
 * zeroes d_info to start a bank, and a bank with ready > 0 is continued.
 *   - A stream segment is a run of calls whose j0 each equal the previous j0 + rows, covering rows
 *     [j_first, j_end). A call that does not continue the previous one starts a new segment (the
 *     carried rows and pending packets are forgotten, the bank keeps what it has), as do
 *     mkid_reset_stream and mkid_set_capture.
 *   - Stamps are unwrapped as for mkid_pulse_heights: base = max(j0 - 2^27, 0),
 *     jg = base + ((ts - base) mod 2^28).
 *   - A packet of channel c < C is eligible when s = jg - pre >= j_first (and >= j0 - the rows
 *     carried, max(length - 1, pre + 1): true of any stamp >= j0 - 1); channels >= C are ignored.
 *   - It completes in the call where s + length <= j_end first holds; until then it waits in a
 *     device-side pending list, so a window may span any number of calls. Windows still open when
 *     the stream ends are not recorded.
 *   - Completions of a channel are in stamp order. The first R are recorded: d_records[c][k][:] =
 *     phase[s : s + length, c], bit-identical, d_stamps[c][k] = jg, ready = records held. Later
 *     ones only add to dropped, as do packets beyond the pending list's room of
 *     (length - pre) / max(cfg.dead_time, 1) + 2 per channel, which the device trigger's own
 *     packets never exceed.
 *   - Any chunking of a segment, 1-row calls included, gives the result of one call over it.
 * rows == 0 and n == 0 are valid. Device pointers only; asynchronous on the context stream; the
 * counted form reads min(*d_count, cap) packets (d_count = &d_counts[1] of the process call: no
 * host round trip). MKID_E_STATE before mkid_set_capture. Timed as MKID_K_CAPTURE. */
int mkid_set_capture(mkid_ctx* ctx, int32_t length, int32_t pre, int32_t max_per_ch);
int mkid_capture_pulses(mkid_ctx* ctx, const float* d_phase, int64_t rows, int64_t j0,
                        const uint64_t* d_events, int64_t n, float* d_records, int64_t* d_stamps,
                        int32_t* d_info);
int mkid_capture_pulses_counted(mkid_ctx* ctx, const float* d_phase, int64_t rows, int64_t j0,
                                const uint64_t* d_events, const int64_t* d_count, int64_t cap,
                                float* d_records, int64_t* d_stamps, int32_t* d_info);

/* Every channel's template and pulse filter from a record bank in one call: the bank that
 * mkid_capture_pulses filled (or any bank of that layout) becomes the table that
 * mkid_set_pulse_filter takes, and optionally every channel's template and noise PSD.
 *   - Device pointers only; asynchronous on the context stream. Once the workspace exists the call
 *     makes no device-to-host copy and no stream synchronisation (growing the workspace allocates,
 *     synchronises once and moves the new buffer in). I1m/Q1m, pm/pdev, count1, count, pstart and
 *     flag are produced and consumed on the device.
 *   - IQ mode (d_Q != NULL): rows [0, ready_c) of d_I[c], d_Q[c] ([Cb][R][2000] float32) go through
 *     exactly mkid_make_template and then mkid_optimal_filter(pre, ncoeff): template, noise, every
 *     info field and coeff = (float) of the float64 weights are bit-identical to those two calls on
 *     that channel's set, the reference's double re-reference of the first 1000 pulses and the
 *     pass-1 cap of 1000 pulses included. This holds because mkid_make_template launches the same
 *     kernels on a one-channel bank (R = ready = npulses) and the filter stage is one device function
 *     for both calls; a channel's result does not depend on its slot, R or the group (below).
 *   - Phase mode (d_Q == NULL): d_I holds phase records (rad); the same pipeline runs on
 *     I = cosf(sign phi), Q = sinf(sign phi), formed as the records are loaded (no I/Q copy of the
 *     bank is made).
 *   - ready_c = d_ready[c * ready_stride] clamped to 0..R (ready_stride 2 reads the ready column of a
 *     capture d_info, 1 a plain list). A channel is worked on iff ready_c >= max(min_records, 1).
 *   - d_result[c].status: 0 used; 1 below min_records; 2 no pulse passed pass 1; 3 none passed pass
 *     2. Where status != 0 the channel's rows of d_coeff, d_templates and d_noise keep the bits they
 *     had (the caller pre-fills its fallback), flag = pstart = -1 and count = 0; count1, pm and pdev
 *     are what pass 1 found (status 2, 3) or 0 (status 1).
 *   - The bank and d_ready are never written; rows at or beyond ready_c and the other columns of
 *     d_ready are never read.
 *   - A channel's outputs depend on its own records and pre / ncoeff / sign only: not on its index,
 *     its neighbours, Cb, R or group.
 *   - The workspace is bounded by a fixed byte budget (256 MiB, unless one channel alone needs
 *     more), not by Cb R: channels are worked on in groups of `group` (0: as many as the budget
 *     holds; a larger request is cut to that).
 *   - MKID_E_ARG before any launch: a null required pointer, length != 2000, Cb < 1, R < 1, pre
 *     outside 10..2000, ncoeff outside 1..800, ready_stride < 1, group < 0, and in phase mode a
 *     sign that is zero or not finite. Not timed (no MKID_K_ id). */
typedef struct mkid_bank_cfg {
    int32_t n_channels;    /* Cb: channels of the bank (need not equal the context's C)      */
    int32_t max_per_ch;    /* R: record stride of the bank                                   */
    int32_t length;        /* rows per record; must be 2000 (MKID_E_ARG otherwise)           */
    int32_t min_records;   /* a channel is worked on iff ready >= max(min_records, 1)        */
    int32_t pre, ncoeff;   /* as mkid_optimal_filter: 10 <= pre <= 2000, 1 <= ncoeff <= 800  */
    int32_t ready_stride;  /* int32 stride of d_ready: 2 for a capture d_info, 1 for a plain list */
    int32_t group;         /* channels worked on per pass; 0 = as many as the workspace budget holds */
    float   sign;          /* phase mode only: I = cos(sign*phi), Q = sin(sign*phi)          */
} mkid_bank_cfg;
typedef struct mkid_bank_result {   /* one per channel, on the device */
    double count, count1, pm, pdev;
    int32_t flag, pstart;
    int32_t status;        /* 0 used; 1 below min_records; 2 no pulse passed pass 1; 3 none passed pass 2 */
    int32_t ready;         /* the record count used (d_ready clamped to 0..R) */
} mkid_bank_result;
int mkid_bank_filters(mkid_ctx* ctx, const float* d_I, const float* d_Q, const int32_t* d_ready,
                      const mkid_bank_cfg* cfg, double* d_templates, double* d_noise, float* d_coeff,
                      mkid_bank_result* d_result);

/* Every channel's trigger threshold from a Fix16_13 phase block in one call: the reference's rule
 * (loadThresholds / loadSingleThreshold, ROACH_Pulses.py:211-299; mkids_sdr_amd.codecs.
 * threshold_from_phase under numpy 2) for columns 0..nch-1 of d_raw [rows][ld] int16 (the layout of
 * mkid_replay_trigger; e.g. mkid_last_raw_phase of a quiet call). The result goes to
 * mkid_set_thresholds. Per channel, over its rows samples x:
 *   range      lo = min x, hi = max x as doubles; lo == hi: lo -= 0.5, hi += 0.5
 *   edges      step = (hi - lo) / 100; e[i] = i step + lo (i = 0..99; product and sum each rounded,
 *              never fused), e[100] = hi: np.histogram(x, bins=100)'s np.linspace
 *   bin        of x: the largest i <= 99 with e[i] <= x; count[i] samples, exact integers
 *   fractions  n[i] = (double)(float)count[i] / (double)rows  (np.array(n, dtype='float32') /
 *              np.sum(n): float32 over an int64 scalar is a float64 division)
 *   sums       tot[i] = np.sum(n[:i]), i = 0..100, in numpy's pairwise order below 128 elements:
 *              sequential from 0 below 8 elements, else 8 accumulators over the multiple-of-8
 *              prefix, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order
 *   threshold  med = e[first argmin |tot - 0.5|], p05 = e[first argmin |tot - 0.05|],
 *              thr = max((int)(-nsigma |med - p05|), -25736), the cast truncating toward zero
 * Counts are integers and every float64 step is one IEEE operation in a fixed order, so d_thr, med
 * and p05 are bit-identical to the host rule, to mkid_phase_thresholds_host, and from run to run.
 *   - mkid_phase_thresholds: device pointers only, asynchronous on the context stream; nch need not
 *     equal the context's C; the block is never written; d_thr [nch] and d_stats [nch] (nullable)
 *     are written for channels 0..nch-1 only. Once the workspace exists (min/max [nch] and counts
 *     [nch][100], owned by the context, grown on demand: allocate, synchronise once, move in) the
 *     call makes no device-to-host copy and no synchronisation. MKID_E_ARG before any launch: a null
 *     required pointer, rows < 1 or > 2^31 - 1, nch < 1 or > ld, nsigma negative or not finite.
 *     Not timed (no MKID_K_ id).
 *   - mkid_phase_thresholds_host: the same rule on host memory, through the same definitions
 *     (csrc/thr_common.h); needs no device and no context. The same MKID_E_ARG cases.
 *   - mkid_phase_thresholds_block_rows: the rows per workgroup row block the device call uses for a
 *     block of that shape on the context's device; aligned16 says whether d_raw is 16-byte aligned
 *     (an unaligned block, like an ld that is no multiple of 8, runs one channel per thread, which
 *     can change the strip count and with it the length). The count pass adds one partial table per
 *     row block and channel strip; tests put blocks around this length. */
typedef struct mkid_thr_stats { double med, p05; int32_t lo, hi; } mkid_thr_stats;
int mkid_phase_thresholds(mkid_ctx* ctx, const int16_t* d_raw, int64_t rows, int64_t ld, int32_t nch,
                          double nsigma, int32_t* d_thr /* [nch] */, mkid_thr_stats* d_stats /* nullable */);
int mkid_phase_thresholds_host(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, double nsigma,
                               int32_t* thr, mkid_thr_stats* stats /* nullable */);
int mkid_phase_thresholds_block_rows(const mkid_ctx* ctx, int64_t rows, int64_t ld, int32_t nch,
                                     int32_t aligned16, int64_t* block_rows);

/* Every channel's phase-noise spectrum from a Fix16_13 phase block in one call: the reference's
 * longsnapshot rule (ROACH_Pulses.py:521-543; mkids_sdr_amd.codecs.noise_spectrum) for columns
 * 0..nch-1 of d_raw [rows][ld] int16 (the layout of mkid_replay_trigger and mkid_phase_thresholds;
 * e.g. mkid_last_raw_phase of a quiet call). Only the arithmetic width differs from the reference.
 *   n = rows / n_averages (integer division); rows at or beyond n n_averages are never read
 *   piece a of channel c: x_a[j] = scale raw[(a n + j) ld + c], j < n
 *   spec[c][k] = (1 / n_averages) sum_a 20 log10(|X_a[k]| / norm1 / 1e-6), X_a = DFT_n(x_a),
 *   all n bins in np.fft.fft order; the factor scale / norm1 / 1e-6 is one float64 constant added
 *   after the logarithm. |X| == 0 gives -inf (as numpy), and so does the mean over the pieces then;
 *   finite input never gives NaN.
 * A channel's n outputs depend only on its own column, rows, n_averages, scale and norm1: not on its
 * index, nch, ld, the block's alignment, its neighbours or any grouping, and they are the same bits
 * from run to run (the pieces are added in a fixed order, without floating-point atomics). Two
 * pieces of one channel travel as the real and imaginary part of one complex transform; an odd
 * n_averages leaves the last piece unpaired. Every n in 1..MKID_NOISE_MAX_N is supported, primes
 * included: a mixed-radix transform over n's prime factors, a piece held in LDS as complex float32
 * (MKID_NOISE_MAX_N x 8 B = 128 KiB), at a cost of n x (sum of the prime factors) per piece.
 *   - mkid_phase_noise_spectra: device pointers only, asynchronous on the context stream; nch need
 *     not equal the context's C; the block is never written. The tables for an n (twiddles, radix
 *     tables, index maps: under 200 KiB, no workspace that grows with rows or nch) are owned by the
 *     context and made when a call brings a new n: allocate, upload, synchronise once, move in. A
 *     call with the n of the call before makes no device-to-host copy and no synchronisation.
 *     MKID_E_ARG before any launch, d_spec untouched: a null pointer, rows < 1 or > 2^31 - 1,
 *     nch < 1 or > ld, n_averages < 1 or > rows, n > MKID_NOISE_MAX_N, scale or norm1 not finite
 *     or <= 0. Not timed (no MKID_K_ id).
 *   - mkid_phase_noise_spectra_host: the same rule in float64 on host memory through the same
 *     definitions (csrc/noise_common.h, the plan of csrc/mkid_plan.h); needs no device and no
 *     context. The same MKID_E_ARG cases. */
#define MKID_NOISE_MAX_N 16384
int mkid_phase_noise_spectra(mkid_ctx* ctx, const int16_t* d_raw, int64_t rows, int64_t ld, int32_t nch,
                             int32_t n_averages, double scale, double norm1, double* d_spec /* [nch][n] */);
int mkid_phase_noise_spectra_host(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch,
                                  int32_t n_averages, double scale, double norm1, double* spec);

/* Welch power spectral densities of two real float64 series per channel in one call:
 * matplotlib.mlab.psd's defaults (Hanning window, no detrending, one-sided, density scaling,
 * noverlap = nfft / 2), which is how IQsweep.AnalyzeNoise (lib/iqsweep.py:792-801) calls it. For
 * channel c, series a = d_a[c ld + j] and b = d_b[c ld + j] (d_b null: all zeros), j < n:
 *   window     w[j] = 0.5 - 0.5 cos(2 pi j / (nfft - 1)), S2 = sum_j w[j]^2 added in ascending j in
 *              float64 with Kahan's compensation (from s = c = 0.0: y = w^2 - c, t = s + y,
 *              c = (t - s) - y, s = t; the plain sum is 2.4e-14 off at nfft = 262144, which scales
 *              every bin); made once per nfft by the host entry and handed to the kernels as a table
 *   segments   nseg = (n - nfft / 2) / (nfft / 2) (integer division); segment s covers samples
 *              s nfft / 2 .. s nfft / 2 + nfft - 1; samples beyond the last segment are never read
 *   transform  z[j] = (a[j] w[j], b[j] w[j]), Z = DFT_nfft(z) (np.fft.fft's sign). With Z1 = Z[k] and
 *              Z2 = Z[(nfft - k) mod nfft], |A[k]|^2 = ((Z1.re + Z2.re)^2 + (Z1.im - Z2.im)^2) / 4 and
 *              |B[k]|^2 = ((Z1.re - Z2.re)^2 + (Z1.im + Z2.im)^2) / 4, k = 0 .. nfft / 2
 *   sums       the segments are added in strips of MKID_WELCH_STRIP consecutive segments: a strip's
 *              powers in ascending segment order from 0.0, then the strips in ascending order from
 *              0.0; no floating-point atomics
 *   density    P[k] = (acc[k] / nseg) / (fs S2), times 2 for 0 < k < nfft / 2
 * Everything is float64, and every product and sum is one rounded IEEE operation, never fused. The
 * transform is decimation in frequency, in place, in passes of radix 8 while the remaining length
 * allows, then one of radix 4 or 2; a pass on blocks of L elements multiplies output t of the
 * butterfly at offset j by W_L^{j t} (skipped for j = 0), read from the nfft-entry table W_nfft^i =
 * (cos, -sin)(2 pi i / nfft) that the host entry makes in float64.
 *   nfft <= MKID_WELCH_LDS_MAX_N: one workgroup holds a segment in LDS (complex float64, 64 KiB).
 *   nfft larger: a four-step transform nfft = n1 n2 with n1 = 2^floor(log2(nfft) / 2), n2 = nfft / n1
 *              (8192 = 64 x 128, 32768 = 128 x 256, 262144 = 512 x 512), a function of nfft alone:
 *              sample j = n2 j1 + j2, bin k = k1 + n1 k2. The n2 column transforms of length n1 (over
 *              j1), the twiddle W_nfft^{j2 k1} (skipped where j2 k1 = 0), then the n1 row transforms of
 *              length n2 (over j2), through a workspace in global memory. Bin nfft - k lies in row
 *              (n1 - k1) mod n1, so the powers are taken from pairs of rows.
 * Kernel and host twin share one definition of all of this (csrc/welch_common.h), so they give the
 * same bits, and a channel's outputs depend only on its own samples, n, nfft and fs: not on nch,
 * ld, alignment, group or its neighbours. All-zero input gives exactly 0.0 in every bin.
 *   - mkid_welch_psd: device pointers only, asynchronous on the context stream. d_pa, d_pb (nullable)
 *     are [nch][nfft / 2 + 1]. The workspace (strip sums, and the four-step transform's segments) is
 *     owned by the context and bounded by a fixed byte budget (256 MiB, unless one channel alone
 *     needs more), not by nch n: channels are worked on in groups of `group` (0: as many as the
 *     budget holds; a larger request is cut to that). It is grown on demand (allocate, synchronise
 *     once, move in), and the tables are kept per nfft: a repeated call makes no device-to-host
 *     copy and no synchronisation. MKID_E_ARG before any launch, the outputs untouched: a null
 *     required pointer, nfft no power of two or outside 8 .. MKID_WELCH_MAX_N, n < nfft or
 *     n > 2^31 - 1, ld < n, nch < 1, group < 0, fs not finite or <= 0. Not timed (no MKID_K_ id).
 *   - mkid_welch_psd_host: the same rule on host memory through the same definitions; needs no
 *     device and no context. The same MKID_E_ARG cases. */
#define MKID_WELCH_STRIP 32
#define MKID_WELCH_LDS_MAX_N 4096
#define MKID_WELCH_MAX_N 262144
int mkid_welch_psd(mkid_ctx* ctx, const double* d_a, const double* d_b /* nullable */, int64_t n, int64_t ld,
                   int32_t nch, int32_t nfft, double fs, int32_t group, double* d_pa,
                   double* d_pb /* nullable */);
int mkid_welch_psd_host(const double* a, const double* b /* nullable */, int64_t n, int64_t ld, int32_t nch,
                        int32_t nfft, double fs, int32_t group, double* pa, double* pb /* nullable */);

/* IQsweep.AnalyzeNoise (lib/iqsweep.py:770-822) for every channel in one call: a long int16 IQ noise
 * record per channel, d_i, d_q [nch][ld], is moved to the fitted loop centre, rotated and normalised;
 * Welch spectra of its phase and amplitude at two resolutions are stitched into one spectrum, and
 * the frequency noise at f_eval is read off a line through a few of its bins. Per channel, with the
 * float64 zero point I0, Q0 (d_i0, d_q0), the fitted centre Icen, Qcen (d_icen, d_qcen: p[8], p[9]
 * of mkid_fit_loops) and the fitted Q (d_qfit: p[0]):
 *   means      SI, SQ the exact int64 sums of the first n samples;
 *              mI = ((((double)SI / (double)n) gain) / full_scale - I0) - Icen, mQ alike (np.mean's
 *              pairwise sum replaced by an exact one); resang = atan2(mQ, mI), c = cos(resang),
 *              s = sin(resang), rad = mI c + mQ s
 *   sample     Ia = ((((double)x gain) / full_scale) - I0) - Icen, Qa alike;
 *              nI = (Ia c + Qa s) / rad, nQ = (Qa c - Ia s) / rad;
 *              phase = atan2(nQ, nI), amp = sqrt(nI nI + nQ nQ)
 *   spectra    mkid_welch_psd's rule on (phase, amp) at nfft_low and at nfft_high, fs = samprate; the
 *              transforms' loader forms phase and amp as it loads: no float64 copy of the record
 *   stitch     r = nfft_low / nfft_high; pn[0 : r k_join] = low[0 : r k_join], pn[r k_join :] =
 *              high[k_join : nfft_high / 2] (the Nyquist bin is left out, as :805 does);
 *              nout = r k_join + nfft_high / 2 - k_join (2552 for the reference's values); an alike.
 *              Stitched bin b has frequency b (samprate / nfft_low) below r k_join and
 *              (b - r k_join + k_join) (samprate / nfft_high) from there (mkid_iq_noise_freqs)
 *   fn1k       the line through stitched bins fit_first .. fit_first + fit_count - 1 of pn in closed
 *              form: xm, ym the means (sums in ascending order over the count), slope =
 *              sum (x - xm)(y - ym) / sum (x - xm)^2, v = ym + slope (f_eval - xm);
 *              fn1k = v / (16.0 (Q Q))
 * Status bits: MKID_IQN_NONFINITE an offset (I0, Q0, Icen, Qcen) is not finite; MKID_IQN_BAD_RAD rad
 * is zero or not finite: pn, an and fn1k are NaN; MKID_IQN_BAD_Q the fitted Q is zero or not finite:
 * fn1k alone is NaN. Device and host twin differ only through atan2, sin and cos; sum_i, sum_q,
 * nseg_low, nseg_high and status are equal bit for bit.
 *   - mkid_iq_noise: device pointers only, asynchronous on the context stream; workspace, tables and
 *     grouping as mkid_welch_psd (cfg->group). d_pn, d_an [nch][nout], d_result [nch]. MKID_E_ARG
 *     before any launch, the outputs untouched: a null pointer, nch < 1, ld < n, n < nfft_low or
 *     n > 2^31 - 1, nfft_high no power of two or outside 8 .. MKID_WELCH_LDS_MAX_N, nfft_low no
 *     power of two, <= nfft_high or > MKID_WELCH_MAX_N, k_join < 1, k_join >= nfft_high / 2,
 *     r k_join > nfft_low / 2, fit_count < 2, the fit range outside [0, nout), group < 0, samprate
 *     not finite or <= 0, f_eval not finite, gain or full_scale not finite or zero.
 *   - mkid_iq_noise_host: the same rule on host memory through the same definitions.
 *   - mkid_iq_noise_freqs: the nout stitched frequencies on the host; MKID_E_ARG as for the cfg. */
#define MKID_IQN_NONFINITE 1
#define MKID_IQN_BAD_RAD 2
#define MKID_IQN_BAD_Q 4
typedef struct mkid_iqnoise_cfg {
    int32_t nfft_low, nfft_high;    /* the reference: 262144, 4096                              */
    int32_t k_join;                 /* high-resolution bins replaced by low-resolution ones: 8  */
    int32_t fit_first, fit_count;   /* stitched bins of the fn1k line: 521, 5                   */
    int32_t group;                  /* channels per pass; 0 = as many as the budget holds       */
    double samprate, f_eval;        /* 200000.0, 1000.0                                         */
    double gain, full_scale;        /* x gain / full_scale: 0.2, 32767.0                        */
} mkid_iqnoise_cfg;
typedef struct mkid_iqnoise_result {   /* one per channel */
    double mean_i, mean_q, resang, rad, fn1k;
    int64_t sum_i, sum_q;
    int32_t nseg_low, nseg_high, status, pad;
} mkid_iqnoise_result;
int mkid_iq_noise(mkid_ctx* ctx, const int16_t* d_i, const int16_t* d_q, int64_t n, int64_t ld, int32_t nch,
                  const double* d_i0, const double* d_q0, const double* d_icen, const double* d_qcen,
                  const double* d_qfit, const mkid_iqnoise_cfg* cfg, double* d_pn, double* d_an,
                  mkid_iqnoise_result* d_result);
int mkid_iq_noise_host(const int16_t* i, const int16_t* q, int64_t n, int64_t ld, int32_t nch, const double* i0,
                       const double* q0, const double* icen, const double* qcen, const double* qfit,
                       const mkid_iqnoise_cfg* cfg, double* pn, double* an, mkid_iqnoise_result* result);
int mkid_iq_noise_freqs(const mkid_iqnoise_cfg* cfg, double* freqs /* [nout] */);

/* Kernel timing with HIP events on the context stream (for bench roofline numbers). */
#define MKID_K_CHANNELIZE 0
#define MKID_K_FIR_PHASE 1
#define MKID_K_TRIGGER 2
#define MKID_K_COMPACT 3
#define MKID_K_FRONT 4        /* fused K1-K6 (replaces CHANNELIZE + FIR_PHASE when used) */
#define MKID_K_COPY 5         /* mkid_stream_copy (measured HBM roof)                     */
#define MKID_K_HEIGHTS 6      /* mkid_pulse_heights                                       */
#define MKID_K_CAPTURE 7      /* mkid_capture_pulses                                      */
#define MKID_K_COUNT 8
/* mkid_set_timing: enable 0 off, any other value times every kernel (the round-1..3 meaning).
 * mkid_set_timing_mask: an OR of MKID_TIMING_ONLY(k) times only those kernels (0 = off). Each timed
 * launch records two events on the stream, and an event record costs a few microseconds of
 * stream time (rocprofv3 traces: 5-6 us gaps around timed kernels), so a throughput run times
 * only the kernel it reports. Both reset the accumulated times. */
#define MKID_TIMING_ONLY(k) (1 << (k))
int mkid_set_timing(mkid_ctx* ctx, int32_t enable);
int mkid_set_timing_mask(mkid_ctx* ctx, uint32_t kernel_mask);
int mkid_get_timing(mkid_ctx* ctx, int32_t kernel, double* total_ms, int64_t* launches);
const char* mkid_kernel_name(int32_t kernel);

/* Diagnostic, not on the hot path: HBM stream copy d_dst = d_src (bytes a multiple of 16, both
 * 16-byte aligned), device pointers, asynchronous on the context stream, timed as MKID_K_COPY.
 * bench.py reads the chip's achievable bandwidth from it in the same run. */
int mkid_stream_copy(mkid_ctx* ctx, void* d_dst, const void* d_src, int64_t bytes);

/* Synthetic ADC source for tests/bench (device; NOT part of the hot path):
 *   out[n] = base[(n0+n) mod 2^16] + AWGN(sigma) + sum_p amp_c e^{i theta_c(t)} (e^{i delta_p(t)} - 1)
 * base = conj(DAC tone comb) as int16 [2^16][2] (the loop-back spectrum inversion implied by
 * ROACH_Setup.py:485-487 vs 511-517); theta_c(t) = 2 pi (freq_index_c t mod 2^16)/2^16 + phase0_c;
 * delta_p(tau) = -amp_rad (1 - e^{-tau/tau_rise}) e^{-tau/tau_fall} for 0 <= tau < window (ADC
 * samples; shape after ReadoutControls/lib/pulses.py:470-472). pulses sorted by start. */
typedef struct mkid_synth_tone { float amp; float phase0; int32_t freq_index; int32_t pad; } mkid_synth_tone;
typedef struct mkid_pulse { int64_t start; int32_t tone; float amp_rad; } mkid_pulse;
int mkid_synth_adc(mkid_ctx* ctx, int16_t* d_out, int64_t nsamples, int64_t n0,
                   const int16_t* d_base_iq, const mkid_synth_tone* d_tones,
                   const mkid_pulse* d_pulses, int64_t npulses, float tau_rise, float tau_fall,
                   int32_t window, float noise_sigma, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* MKIDGPU_H */
