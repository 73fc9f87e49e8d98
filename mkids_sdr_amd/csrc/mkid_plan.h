// Host-side planning of libmkidgpu.so, free of HIP so that it builds and runs on the CPU under
// AddressSanitizer / UndefinedBehaviorSanitizer (make -C mkids_sdr_amd/csrc asan; tools/plan_fuzz.cpp):
// workspace sizing at context creation, the per-call trigger segmentation and its slot-table
// geometry, the k_front3 select-slot order, the K1 tap quantisation, the merge of per-chunk packet
// lists, the reference packet re-encode, the validity bookkeeping of a carried history, the
// grouping and workspace layout of mkid_bank_filters, the launch geometry and workspace of
// mkid_phase_thresholds and the radix list, tables and index maps of mkid_phase_noise_spectra. The host
// files mkid_api.hip, mkid_stream.hip and mkid_calib.hip are the only product callers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mkidgpu.h"
#include "noise_common.h"

namespace mkid {
namespace plan {

constexpr int kFirTaps = 26;   // ROACH_Pulses.py:61
constexpr int kPfbTaps = 4;

// Speculative trigger segmentation (k_trigger.hip): segments of at least kSegL phase samples,
// each speculating from kSegW samples of warm-up (a multiple of the 26-sample matched-filter ring).
// The EMA baseline (alpha 41/512) forgets its start in ~10^2 samples on noisy phase. The warm-up is
// pure overhead when the speculation holds and the fix-up re-runs a segment when it does not
// (exact either way): on the bench stream 520 -> 260 samples is -6 % trigger time with no re-run,
// 130 re-runs 427 segments per step and gains nothing (profiles/r04/r04_j_kbench_trig_warmup.json).
// The floor kSegL only binds when the channels are few (256 at config 2: 2^28 samples give 2048
// rows per channel-segment at one wave per SIMD); 2048 -> 1024 is -41 % k_trig_spec there, 512
// no better, and config 3 / 5 segments are longer anyway (profiles/r04/r04_o_kbench_c2.json).
constexpr int64_t kSegL = 1024;
constexpr int64_t kSegW = 260;
// SVF baseline (Chamberlin 2-pole, Kf 82 / Kq 93623 Fix18_16): two integer trajectories started
// from different states coincide only after ~10^4 samples (median 1.5e4, 99th percentile 2.9e4, max
// 3.9e4 over 1024 simulated noisy channels; on the bench stream a 49k-sample warm-up misses 0.3 %
// of segments, 98k about 1 in 30000). Since round 6 the misses are re-run in
// parallel (k_trig_refix), so the warm-up is the half length: 49 140 samples with segments at one
// per SIMD lane (mkid_api.hip) measured 84-85 GS/s at config 3 against 65 for 98 280 at one per two
// lanes (profiles/r06/r06{f,g}_svf_*). Lengths are multiples of 26 so that every warm-up start keeps
// the filter ring aligned; segments are at least kSvfLmin long.
constexpr int64_t kSvfW = 26 * 1890;
constexpr int64_t kSvfLmin = 26 * 158;
static_assert(kSegW % kFirTaps == 0 && kSegL >= kSegW + kFirTaps - 1, "segment geometry");
static_assert(kSvfW % kFirTaps == 0, "SVF warm-up geometry");

// Packets a channel can produce in L phase rows: an event needs >= dead + 3 samples (trigger, peak,
// dead time, re-arm), plus the partial cycles at both ends.
int64_t seg_capacity(int64_t L, int dead);
// segment length for J rows: >= kSegL, and (C/64) * ceil(J/L) waves <= the resident wave slots
int64_t seg_length(int64_t J, int C, int64_t wave_slots);

// What a context was sized for (mkid_create): every later call is planned within it.
struct Workspace {
    int64_t max_chunk = 0;    // samples per call (cfg.max_chunk)
    int64_t Kmax = 0, Jmax = 0;   // FFT frames and phase rows of a call of max_chunk samples
    int64_t capc = 0;         // per-channel packet capacity of a whole call
    int64_t trig_slots = 0, svf_lanes = 0, svf_w = kSvfW;
    int64_t nseg_max = 0;     // segments per call
    int64_t slot_cap = 0;     // packet slots of the [C][nseg][capseg] table
    int64_t scratch_cap = 0;  // per-channel fix-up scratch
};
// cfg already validated (N = 2C, max_chunk a multiple of N, dead_time >= 0)
const char* size_workspace(const mkid_cfg& cfg, int64_t trig_slots, int64_t svf_lanes, int64_t svf_w,
                           Workspace& ws);

// Trigger geometry of one call of J phase rows: nseg segments of L rows (the last one shorter), each
// speculating from W rows of warm-up into capseg packet slots of the call's [C][nseg][capseg] table.
struct TrigPlan {
    int64_t J;
    int32_t L, W, nseg, capseg;
};
// The plan of a call of n samples (n a positive multiple of N, n <= max_chunk). Returns nullptr, or
// the error text when the call or its plan exceeds the workspace.
const char* plan_call(const Workspace& ws, int C, int N, int mode, int dead, int64_t n, TrigPlan& p);

// Which rows of a history buffer of H rows are valid: the last `rows`, and they precede a call that
// starts at global row j0 only if they end there (pulse heights and capture, mkid_calib.hip).
struct Carry {
    int64_t H = 0, end = -1, rows = 0;   // end: global row after the last carried one (-1: none)
    int64_t before(int64_t j0) const { return end == j0 ? rows : 0; }
    int64_t offset(int64_t j0) const { return H - before(j0); }   // first valid row of the buffer
    void advance(int64_t j0, int64_t n) { rows = std::min(H, before(j0) + n), end = j0 + n; }   // n rows rolled in
    void drop() { end = -1, rows = 0; }
};

// Workspace of mkid_bank_filters: the channels of a bank are worked on `group` at a time, and the
// group's tables (BankArgs, mkid_internal.h) are carved from one buffer of `bytes` bytes at the
// byte offsets below, each a multiple of kBankAlign. group = max(1, min(Cb, kBankMaxGroup, the
// channels `budget` holds, want if want > 0)): bytes <= budget whenever one channel fits, whatever
// Cb and R are; groups c0 = 0, group, 2 group, ... of min(group, Cb - c0) channels cover the bank.
constexpr int64_t kBankBudget = 256ll << 20;
constexpr int64_t kBankAlign = 256;
constexpr int64_t kBankMaxGroup = 65535;   // the group is a grid's y extent
struct BankWs {
    int64_t group = 0, bytes = 0, channel_bytes = 0;
    int64_t rows = 0, nrows = 0, peaks = 0, scratch = 0, tP = 0, tPf = 0, noise = 0, stats = 0, work = 0,
            coeff = 0, refmed = 0, accept = 0, appended = 0, status = 0, nready = 0;
};
BankWs plan_bank(int64_t Cb, int64_t R, int64_t budget, int64_t want = 0);

// mkid_phase_thresholds (k_thresholds.hip): a workgroup of kThrThreads threads takes a strip of
// kThrStrip channels x a block of B rows; a thread holds `vec` adjacent channels of a row (8: one
// 16-byte load, when the block is 16-byte aligned and ld a multiple of 8; else 1). Channels
// [0, nch_vec) run vec-wide, the tail [nch_vec, nch) one channel per thread. B is a multiple of
// kThrRowStep in kThrMinB..kThrMaxB that gives about two workgroups per compute unit where the
// block is large enough; the jobs (strip x row block) of either launch are walked by a grid of at
// most kThrMaxGrid workgroups. Workspace: lo [nch] int32, hi [nch] int32, counts [nch][100] uint32
// at the byte offsets below.
constexpr int kThrStrip = 64;
constexpr int kThrThreads = 256;
constexpr int64_t kThrRowStep = 32, kThrMinB = 128, kThrMaxB = 1024;
constexpr int64_t kThrMaxGrid = 1 << 20;
constexpr int kThrFinishCh = 16;          // channels a finish workgroup takes
constexpr int64_t kThrMaxInitGrid = 4096; // the init kernel strides over [nch][100]
struct ThrPlan {
    int32_t vec = 1, nch_vec = 0;
    int64_t B = 0, row_blocks = 0;
    int64_t strips_vec = 0, strips_tail = 0;   // strips of the two launches
    int64_t grid_vec = 0, grid_tail = 0;       // their grids (0: no launch)
    int64_t grid_init = 0, grid_finish = 0;    // workgroups of the init and the finish kernel
    int64_t off_lo = 0, off_hi = 0, off_counts = 0, bytes = 0;
};
// rows >= 1, 1 <= nch <= ld, ncu >= 1 (the entry point checks)
ThrPlan plan_thresholds(int64_t rows, int64_t ld, int32_t nch, bool aligned16, int ncu);

// mkid_phase_noise_spectra (k_noise.hip, noise_common.h): the transform of length n as in-place
// decimation-in-frequency passes, one per radix. The radices are n's prime factors with the twos
// taken in pairs (radix 4, then one 2 if their count is odd), in descending order: a large radix
// runs while M = L / r is still large, so that the lanes of a wave share the output index t and
// with it the radix-table entry they read. wn [n] is W_n^i and wr the passes' W_r^i tables one after
// the other (Pass::tw_off), in float64; bin_of_pos[p] is the bin that position p holds after the
// last pass and partner[p] the position of bin (n - bin_of_pos[p]) mod n. The device image of the
// tables (noise_pack_tables) is wn and wr as float32 pairs, then the two index tables, at the byte
// offsets below, `bytes` in all. A workgroup of `threads` threads takes a channel; every thread
// holds per_thread positions in registers (an output and a float64 sum each), threads * per_thread
// >= n: 256 x 16 up to n = 4096, 1024 x 16 above. lds_bytes: the piece as
// float32 pairs, kNoiseStageR radix-table entries and four partial words per wave.
constexpr int kNoiseThreadsSmall = 256, kNoisePerSmall = 16;
constexpr int kNoiseThreadsLarge = 1024, kNoisePerLarge = 16;
constexpr int kNoiseStageR = 1024;         // radix tables up to this length are staged in LDS
constexpr int64_t kNoiseMaxGrid = 1 << 20;
constexpr int64_t kNoiseXcdSpan = 256;     // the grid is a multiple of 8 XCDs x 32 channels of a 64-byte line
struct NoisePlan {
    int32_t n = 0;
    std::vector<noise::Pass> passes;
    std::vector<noise::Cx<double>> wn, wr;
    std::vector<uint16_t> bin_of_pos, partner;
    int32_t threads = 0, per_thread = 0;
    int64_t lds_bytes = 0;
    int64_t off_wn = 0, off_wr = 0, off_bin = 0, off_partner = 0, bytes = 0;
};
// 1 <= n <= MKID_NOISE_MAX_N (the entry point checks); false otherwise
bool plan_noise(int32_t n, NoisePlan& p);
// the device image of p's tables into out [p.bytes]
void noise_pack_tables(const NoisePlan& p, char* out);
// blocks the launch walks for nch channels (a multiple of kNoiseXcdSpan) and the channel of block
// b: blocks b and b + 8 tend to share an XCD, so the 32 channels of a 64-byte line of the block go
// to blocks 8 apart. A permutation of 0 .. blocks-1; channels >= nch are skipped. Speed only.
inline int64_t noise_blocks(int64_t nch) { return (nch + kNoiseXcdSpan - 1) / kNoiseXcdSpan * kNoiseXcdSpan; }
NOISE_HD int64_t noise_channel_of_block(int64_t b) {
    const int64_t i = b >> 3, xcd = b & 7;
    return (((i >> 5) << 3) + xcd) * 32 + (i & 31);
}

// mkid_pulse_fit (k_heights_fit.hip): one wave per packet, its LDS region of wave_floats floats
// holding, at the float offsets below, the window's W = ncoeff + 2 L rows, the channel's ncoeff
// coefficients, the wave's 64 partial sums and the nl = 2 L + 1 lag values. Lanes 0 .. G nl - 1 work,
// G = 64 / nl: lane g nl + d adds the taps i = g, g + G, g + 2 G, ... of lag d - L, reading
// coefficient i and window row i + d (<= ncoeff - 1 + 2 L = W - 1). A workgroup holds `waves`
// regions, at most kFitWaves and as many as kFitLdsBytes hold; the grid is capped at eight waves per
// SIMD of every compute unit and strides over the packets.
constexpr int kFitWaves = 4;
constexpr int64_t kFitLdsBytes = 64 * 1024;
struct FitPlan {
    int32_t W = 0, nl = 0, G = 0;
    int32_t off_w = 0, off_cf = 0, off_part = 0, off_h = 0, wave_floats = 0;
    int32_t waves = 0;
    int64_t lds_bytes = 0, grid_cap = 0;
    int64_t blocks(int64_t n) const { return std::min((n + waves - 1) / waves, grid_cap); }
};
// 1 <= ncoeff <= 4096, 0 <= L <= 31, ncu >= 1 (the entry points check)
FitPlan plan_fit(int32_t ncoeff, int32_t L, int ncu);

// k_front3 select-slot order (mkid_api.hip / include/mkidgpu.h mkid_slot_order): out[slot] = channel
void slot_order(const std::vector<int32_t>& bins, int C, std::vector<int16_t>& out);

// K1 taps as the device applies them: h_q = rint(h 2^S) int16, returns S
int quantize_pfb(const float* h, int T, int N, std::vector<int16_t>& hq);

// K7 re-arm level of a channel (mkid_set_rearm; oracle/trigger.py rearm_levels): the level moves
// from the threshold toward 0 (the baseline) by q8 / 256: thr - floor(thr q8 / 256), q8 in 0..256
int32_t rearm_level(int32_t thr, int32_t q8);

// per-chunk channel-major packet lists concatenated -> one channel-major list (stable in time)
void merge_channel_major(uint64_t* ev, int64_t n);

// wide device packet -> reference 64-bit packet; -1 if a channel does not fit the 8-bit field
int pack_reference(const uint64_t* wide, int64_t n, uint64_t* out);

}  // namespace plan
}  // namespace mkid
