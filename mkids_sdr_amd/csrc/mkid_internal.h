// Internal declarations shared by the HIP translation units of libmkidgpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <vector>

#include "mkidgpu.h"
#include "pkt_common.h"

namespace mkid {

constexpr int kPfbTaps = 4;    // T: PFB taps per branch (build decision)
constexpr int kFirTaps = 26;   // ROACH_Pulses.py:61
constexpr int kLpfHist = kFirTaps - 2;  // z frames carried for the decimating IQ low-pass
constexpr int kRawHist = kFirTaps - 1;  // raw phase samples carried for the matched filter
// Start-of-stream trigger hold-off (phase samples): after a reset the trigger is DEAD with no
// baseline while the PFB / low-pass / matched-filter histories fill (build decision, DESIGN.md §2;
// oracle/trigger.c HOLDOFF)
constexpr int kHoldOff = 64;

// Per-channel trigger state. Byte layout identical to oracle/trigger.c trig_state.
struct TrigState {
    int32_t B, binit, st, cnt, f1, f2, pad0, pad1;
    int64_t low, band;
};
static_assert(sizeof(TrigState) == 48, "TrigState layout");

struct LpfTaps { float g[kFirTaps]; };

// IQ snapshot sample: the low-pass output in ADC-count units, rounded and saturated to int16
__device__ __forceinline__ int16_t iq16(float v) {
    const float r = rintf(v);
    return (int16_t)(r < -32768.f ? -32768.f : (r > 32767.f ? 32767.f : r));
}

struct ChanArgs {
    const uint32_t* x;      // chunk, int16 I/Q packed per 32-bit word
    const uint32_t* xhist;  // T*N - M previous samples
    const float* pfb;       // T*N prototype
    const int32_t* bins;    // C
    const float2* lo;       // [P][C], conj(LUT)/2^15
    float2* z;              // [K][C]
    int64_t K;              // frames in this chunk
    int64_t k0;             // global index of the chunk's first frame
    int32_t P;              // LO period (power of two)
    int64_t frames_per_block;  // set by the launcher
};

// Centred low-pass (K5-K6 with the IQ-loop centre c subtracted BEFORE the accumulation, DESIGN.md
// §4): the kernels accumulate y' = sum_i g_i (z_i - c') with c' = c / G (G = sum_i g_i) and output
// phase = atan2(y' + r), r = G c' - c (host, float64). The partial sums then stay at the loop's
// radius instead of the tone's |y|, so the fp32 rounding of the accumulation no longer grows with
// |c| / radius. y = y' + (r + c) where the raw IQ is needed (IQ tap: `tap_off`; avgIQ: the host).
struct Centring {
    const float2* ncen;     // [C] -c' (the DDC's fused add)
    const float2* cor;      // [C] r
    float2 tap_off;         // r + c of the IQ-tap channel
};

struct LpfArgs {
    const float2* z;        // [K][C]
    const float2* zhist;    // [24][C]
    Centring cen;
    float* phase;           // [J][C] or nullptr
    int16_t* raw;           // [J][C]
    long long* ysum;        // [C][2] per-channel sum of y' (avgIQ), fixed point 2^-kYsumFrac, or nullptr
    int64_t J;
    int32_t C;
    LpfTaps taps;
    int16_t* iqtap;         // [J][2] int16 low-pass output of channel iq_ch (IQ snapshot) or nullptr
    int32_t iq_ch;
};

// avgIQ accumulator (firmware K9, avgIQ_bram): per-thread float partial sums are rounded to
// fixed point (2^-8) and added with integer atomics, so the sums do not depend on the order in
// which workgroups finish (float atomics would make the loop calibration run-to-run different)
constexpr int kYsumFrac = 8;
__device__ __forceinline__ void ysum_add(long long* ysum, int c, float sx, float sy) {
    atomicAdd(reinterpret_cast<unsigned long long*>(ysum) + 2 * c,
              (unsigned long long)llrintf(sx * (float)(1 << kYsumFrac)));
    atomicAdd(reinterpret_cast<unsigned long long*>(ysum) + 2 * c + 1,
              (unsigned long long)llrintf(sy * (float)(1 << kYsumFrac)));
}

struct FrontArgs {
    const uint32_t* x;      // chunk, int16 I/Q packed per 32-bit word
    const uint32_t* xhist;  // front_hist_samples(N) previous samples
    const uint2* pfbq;      // [N] int16 taps {h0|h1<<16, h2|h3<<16} of point p (scale 2^S in lo)
    const int32_t* bins;    // C
    const float2* lo;       // [P][C], conj(LUT)/2^15
    Centring cen;
    float* phase;           // [K/2][C] or nullptr
    int16_t* raw;           // [K/2][C]
    long long* ysum;        // [C][2] sums of y', fixed point 2^-kYsumFrac, or nullptr (accumulator off)
    int64_t K;              // frames in this chunk (even)
    int64_t k0;             // global index of the chunk's first frame
    int64_t frames_per_block;  // set by the launcher
    int64_t avail;          // samples readable before x; the host always passes 0 (a call is one
                            // launch: everything before x comes from xhist)
    int32_t P;              // LO period (power of two)
    int32_t ncu;           // compute units of the device (grid sizing: per-CU multipliers)
    LpfTaps taps;
    int16_t* iqtap;         // [K/2][2] int16 low-pass output of channel iq_ch (IQ snapshot) or nullptr
    int32_t iq_ch;
    int32_t pad;
    const int16_t* slot_ch; // [C] k_front3 (N = 2048): channel of select slot st + 512 q (nullptr: identity)
};

// Result of one segment's parallel SVF re-run (k_trig_refix, round 6): status and, for a re-run,
// the true packets before the merge detection (in TrigSpecArgs::refix_pk at the segment's slot
// entry), the speculative packets the re-run dropped, and the true end state when it did not merge.
enum { RF_OK = 0, RF_MERGED = 1, RF_UNMERGED = 2 };
struct RefixRes {
    int32_t status, nt, ndrop, pad;
    TrigState T;
};
static_assert(sizeof(RefixRes) == 64, "RefixRes layout");

struct TrigSpecArgs {
    const int16_t* raw;     // [J][C] Fix16_13 phase
    const int16_t* rhist;   // [25][C] previous call's last raw samples
    const int16_t* fir;     // [C][26] matched-filter taps (int12)
    const int32_t* thr;     // [C]
    const int32_t* rearm;   // [C] re-arm levels (mkid_set_rearm; = thr without hysteresis)
    const TrigState* st_in; // [C] carried state (segment 0 starts from it)
    TrigState* st_out;      // [C] carried state after this call (may alias st_in)
    TrigState* s_spec;      // [C][nseg] speculative state at each segment start (k_trigger.hip seg_state)
    TrigState* s_end;       // [C][nseg] state at each segment end
    uint64_t* slots;        // [C][nseg][capseg] packets (entry c*nseg + s)
    int32_t* counts;        // [C][nseg]
    uint64_t* scratch;      // [C][capseg] fix-up scratch
    int32_t* reruns;        // [C] segments re-run by the fix-up (diagnostic, nullable)
    int64_t J;
    int64_t j0;             // global index of the chunk's first phase sample
    int32_t C, nseg, L, W, capseg;
    int32_t mode, alpha, kf, kq, base_thr, dead;
    // Always (nseg, 0): the slot entry is seg_stride c + seg_base + s. They date from calls cut into
    // pieces that shared one table; reading nseg instead changes the register allocation of
    // k_trig_spec (VGPRs 85 -> 86 and 126 -> 128, scratch 48 -> 64 bytes), so removing them waits
    // for an A/B of its own
    int32_t seg_stride, seg_base;
    // The SVF path's tables (mkid_ctx.h SvfTables; an SVF launch needs all three, other modes none).
    // filt: [J][C] matched-filter output (int16) of the filter pre-pass (k_mf_rows), so that the SVF
    // walk, bound by one wave's instruction stream, skips the 26-tap filter. refix / refix_pk: every
    // failed segment is re-run in parallel (k_trig_refix) assuming its predecessor's speculative end
    // state, into [C][nseg] results and a [C][nseg][capseg] packet table; k_trig_fix_svf
    // then confirms the assumptions channel by channel
    int16_t* filt = nullptr;
    RefixRes* refix = nullptr;
    uint64_t* refix_pk = nullptr;
};

struct HeightArgs {
    const float* phase;      // [rows][C] rad, global phase rows j0 .. j0 + rows - 1
    const uint64_t* events;  // [n] wide packets
    const float* coeff;      // [C][ncoeff] per-channel optimal filter
    float* heights;          // [n] out (NaN: window outside the rows or unknown channel)
    int64_t rows, j0, n;    // n: packets (or the bound on *d_n)
    int32_t C, ncoeff, pre;
    const int64_t* d_n;     // nullable: device packet count (pkt::count(d_n, n) packets are processed)
    // carried phase history: rows j0 - hrows .. j0 - 1 ([hrows][C]), read for windows that start
    // before the call's first row (hrows = 0: none)
    const float* hist;
    int64_t hrows;
    int32_t ncu;            // compute units of the device (grid cap)
    int32_t pad;
};

// mkid_pulse_fit (k_heights_fit.hip): HeightArgs' stream, packets, filter and carried rows, the
// search and the four outputs; the LDS geometry comes from the call's plan (mkid_plan.h FitPlan)
struct FitArgs {
    const float* phase;      // [rows][C] rad, global phase rows j0 .. j0 + rows - 1
    const float* hist;       // [hrows][C] carried rows j0 - hrows .. j0 - 1 (hrows = 0: none)
    const uint64_t* events;  // [n] wide packets
    const float* coeff;      // [C][ncoeff]
    const int64_t* d_n;      // nullable: device packet count (pkt::count(d_n, n) packets are processed)
    float* heights;          // [n] fitted height (NaN: window outside the rows or unknown channel)
    float* dt;               // [n] nullable: vertex position in rows relative to the stamp
    int32_t* lag;            // [n] nullable: chosen lag (INT32_MIN where the height is NaN)
    float* h0;               // [n] nullable: the value at lag 0
    int64_t rows, j0, n, hrows;
    int32_t C, ncoeff, pre, L, s;
    int32_t W, nl, G, off_cf, off_part, off_h, wave_floats;
};
namespace plan {
struct FitPlan;
}
hipError_t launch_pulse_fit(FitArgs a, const plan::FitPlan& p, hipStream_t s);

// mkid_count_photons (k_observe.hip): the count image and the two `outside` counters
struct ObsCountArgs {
    const uint64_t* events;  // [n] wide packets
    const int64_t* d_n;      // nullable: device packet count (pkt::count(d_n, n) packets are read)
    int32_t* image;          // [n_seconds][C]
    int64_t* outside;        // [2]
    int64_t n, j0, N, fs;    // fs: samples per second (an integer, obs_common.h fs_ok)
    int32_t C, n_seconds, ncu, pad;
};
hipError_t launch_count_photons(const ObsCountArgs& a, hipStream_t s);

// mkid_height_spectra (k_observe.hip). A call's grid and LDS table come from plan_spectra: the
// list's cut into slices (pkt_common.h slices, where kObsMaxBlocks and kObsSlice are), and an LDS
// table of as many channel rows as fit kObsLdsBytes, kObsMaxRows at the most (a slice of the
// device's order spans few channels, and the table is zeroed and flushed in full), none in the
// plain form.
constexpr int kObsLdsBytes = 32768;
constexpr int kObsMaxRows = 16;
struct ObsPlan {
    pkt::Slices cut;
    int32_t lds_rows, lds_bytes;
};
ObsPlan plan_spectra(int64_t n, int32_t nbins, bool lds);
struct ObsSpectraArgs {
    const uint64_t* events;  // [n] wide packets
    const float* heights;    // [n]
    const int64_t* d_n;      // nullable: device packet count (pkt::count(d_n, n) packets are read)
    const float* lo;         // [C] lower edge of bin 0
    const float* inv;        // [C] 1 / bin width
    int32_t* spectra;        // [C][nbins + 3]
    uint64_t* deferred;      // nullable: [cap_def] packets that wait for their height
    int64_t* ndef;           // [2] {qualified, written} (with deferred)
    int32_t* wg_count;       // [kObsMaxBlocks] deferred packets of each workgroup's slice (with deferred)
    int64_t* wg_off;         // [kObsMaxBlocks] where each workgroup's deferred packets start
    int64_t n, j0, j_defer, cap_def, slice;
    int32_t C, nbins, lds_rows, pad;
};
hipError_t launch_height_spectra(const ObsSpectraArgs& a, const ObsPlan& p, hipStream_t s);
hipError_t launch_concat_packets(const uint64_t* a, const int64_t* d_na, int64_t cap_a, const uint64_t* b,
                                 const int64_t* d_nb, int64_t cap_b, uint64_t* out, int64_t cap_out, int64_t* nout,
                                 int32_t ncu, hipStream_t s);

// mkid_list_photons and mkid_fill_photon_heights (k_photons.hip) and their ring forms: the tables
// are [n_slots][C][K] and the cell is obs::ring_cell's over the window (sec0, sec_end, n_slots); the
// plain forms pass the whole window obs::whole(n_seconds). The list call runs over slices cut as the
// spectra's (pkt::slices) and keeps, per packet, the index of the first packet of its run, and per
// run (at its head's index) the cell's count before the run: photon_ws_bytes(n) of workspace,
// carved as below.
struct PhotonArgs {
    const uint64_t* events;  // [n] wide packets
    const int64_t* d_n;      // nullable: device packet count (pkt::count(d_n, n) packets are read)
    int32_t* image;          // [n_slots][C]
    int64_t* outside;        // [4]; the whole window reaches only [0] and [1]
    uint64_t* words;         // [n_slots][C][K]
    int64_t* stamps;         // [n_slots][C][K]
    int64_t* dropped;        // [1]
    int64_t* head;           // workspace [n]: index of the first packet of packet i's run
    int64_t* carry;          // workspace [kObsMaxBlocks]: last run head of a slice, then of the slices before it
    uint32_t* base;          // workspace [n]: at a run head's index, the cell's count before the run
    int64_t n, j0, N, fs, slice;
    int32_t C, n_slots, K, layout;
    int64_t sec0, sec_end;   // the window's seconds (obs_common.h Window)
};
inline size_t photon_ws_bytes(int64_t n) { return (size_t)n * 12 + (size_t)kObsMaxBlocks * 8; }
inline void photon_ws_carve(PhotonArgs& a, char* ws) {
    a.head = reinterpret_cast<int64_t*>(ws);
    a.carry = a.head + a.n;
    a.base = reinterpret_cast<uint32_t*>(a.carry + kObsMaxBlocks);
}
hipError_t launch_list_photons(const PhotonArgs& a, hipStream_t s);
struct PhotonFillArgs {
    const uint64_t* events;  // [n] wide packets
    const float* heights;    // [n]
    const float* dt;         // nullable [n]
    const int64_t* d_n;      // nullable: device packet count
    const int32_t* image;    // [n_slots][C]
    const int64_t* stamps;   // [n_slots][C][K]
    float* row_height;       // [n_slots][C][K]
    float* row_dt;           // nullable, the same shape
    int64_t* fill;           // [2] {found, not found}
    int64_t n, j0, j_defer, N, fs;
    int32_t C, n_slots, K, ncu;
    int64_t sec0, sec_end;
};
hipError_t launch_fill_photon_heights(const PhotonFillArgs& a, hipStream_t s);

// mkid_pack_second and mkid_clear_second (k_pack.hip): slot sec mod n_slots of the [n_slots][C][K]
// tables. A wave takes one (channel, tile of kPackTile slots) of the copy and of the clear.
constexpr int kPackTile = 256;
struct PackArgs {
    const int32_t* image;      // [n_slots][C]
    const uint64_t* words;     // [n_slots][C][K]
    const int64_t* stamps;     // nullable without out_stamps
    const float* row_height;
    const float* row_dt;       // nullable without out_dt
    int32_t* counts;           // [C]
    int64_t* offsets;          // [C + 1]
    uint64_t* out_words;       // [cap_out]
    int64_t* out_stamps;       // nullable
    float* out_height;
    float* out_dt;             // nullable
    int64_t* total;            // [2] {entries of the second, entries written}
    int64_t row0, cap_out;     // row0 = (sec mod n_slots) C
    int32_t C, K;
};
hipError_t launch_pack_second(const PackArgs& a, hipStream_t s);
struct ClearArgs {
    int32_t* image;
    float* row_height;
    float* row_dt;             // nullable
    int64_t row0;
    int32_t C, K;
};
hipError_t launch_clear_second(const ClearArgs& a, hipStream_t s);

// Pulse capture (k_capture.hip; the contract is in its header comment)
struct CaptureArgs {
    const float* phase;      // [rows][C] rad, global phase rows j0 .. j0 + rows - 1
    const float* hist;       // [hrows][C] carried rows j0 - hrows .. j0 - 1 (hrows = 0: none)
    const uint64_t* events;  // [n] wide packets, channel-major, time-ascending within a channel
    const int64_t* d_n;      // nullable: device packet count (pkt::count(d_n, n) packets are read)
    float* records;          // [C][R][L] caller's bank
    int64_t* stamps;         // [C][R] unwrapped stamp of each record
    int32_t* info;           // [C][2] {ready, dropped}
    const int64_t* pend_in;  // [C][PC] unwrapped stamps of the windows still open, per channel
    const int32_t* pend_n_in;  // [C]
    int64_t* pend_out;       // the list after this call (the other half of the double buffer)
    int32_t* pend_n_out;
    int32_t* work;           // [C][2] this call's records of a channel: {first slot, count}
    int64_t rows, j0, n, hrows;
    int32_t C, L, pre, R, PC, pad;
};

// launchers (return hipError_t of the launch)
hipError_t launch_capture(const CaptureArgs& a, hipStream_t s);
hipError_t launch_pulse_heights(const HeightArgs& a, hipStream_t s);
hipError_t launch_channelize(int N, const ChanArgs& a, hipStream_t s);
hipError_t launch_lpf_phase(const LpfArgs& a, hipStream_t s);
hipError_t launch_trigger(const TrigSpecArgs& a, hipStream_t s);
// resident wave slots of the speculative trigger kernel on a device (occupancy x CUs)
int64_t trigger_wave_slots(int device);

hipError_t launch_hist_roll(void* dst, const void* old_hist, const void* fresh, int64_t hist_rows,
                            int64_t fresh_rows, int64_t row_bytes, hipStream_t s);
// one history-roll job (k_hist_roll's arguments), for the rolls carried by the compaction launch
struct RollJob {
    void* dst;
    const void* old_hist;
    const void* fresh;
    int64_t hist_rows, fresh_rows, row_bytes;
};
// K8 compaction; roll1 / roll2 (or null) run as extra blocks of its gather launch
hipError_t launch_compact(const uint64_t* slots, const int32_t* counts, int64_t n_ent,
                          int32_t capseg, uint64_t* out, int64_t cap, int64_t* d_counts,
                          int64_t* scan_ws, const RollJob* roll1, const RollJob* roll2, hipStream_t s);
hipError_t launch_stream_copy(void* dst, const void* src, int64_t bytes, hipStream_t s);
hipError_t launch_synth(int16_t* out, int64_t n, int64_t n0, const int16_t* base,
                        const mkid_synth_tone* tones, const mkid_pulse* pulses, int64_t npulses,
                        float tr, float tf, int32_t window, float sigma, uint32_t seed,
                        hipStream_t s);

hipError_t launch_replay(const int16_t* raw, int64_t n, int64_t ld, int32_t nch, int32_t mode, int32_t length,
                         int64_t start, int64_t need, int64_t skip, int32_t wrap, double thr, uint32_t* flags,
                         double* means, int32_t* hits, int32_t cap, int32_t* counts, hipStream_t s);

hipError_t launch_optimal_filter(const double* tpl, const double* noise, int pre, int ncoeff, double* coeff,
                                 double* work, hipStream_t s);

// mkid_bank_filters and mkid_make_template (k_template.hip): one group of g channels, c0 .. c0 + g - 1,
// of the caller's bank. The workspace tables hold one slot per channel of the group (plan::BankWs
// gives their sizes).
struct BankArgs {
    const float* I;          // [Cb][R][2000] records: I, or phase (rad) where Q is null
    const float* Q;
    const int32_t* ready;    // [Cb * ready_stride]
    double* out_tpl;         // [Cb][2000], nullable
    double* out_noise;       // [Cb][800], nullable
    float* out_coeff;        // [Cb][ncoeff]; null: no filter is made (pre, ncoeff unused)
    mkid_bank_result* result;  // [Cb]
    double* rows;            // [g][R][2000]
    double* nrows;           // [g][R][800]
    double* peaks;           // [g][R]
    double* scratch;         // [g][2 R + 8]
    double* tP;              // [g][2000] pass-1 templates
    double* tPf;             // [g][2000]
    double* noise;           // [g][800]
    double* stats;           // [g][8] {pm, pdev, peaks, count1, count}
    double* work;            // [g][3][800]
    double* coeff;           // [g][800] float64 weights
    float* refmed;           // [g][2] I1m, Q1m
    int32_t* accept;         // [g][R]
    int32_t* appended;       // [g][R]
    int32_t* status;         // [g]
    int32_t* nready;         // [g] ready clamped to 0..R
    int32_t c0, g, R, ready_stride, min_records, pre, ncoeff;
    float sign;
};
hipError_t launch_bank_filters(const BankArgs& a, hipStream_t s);

// mkid_phase_thresholds (k_thresholds.hip): init, range pass, count pass and finish on stream s; `p`
// is the call's plan (mkid_plan.h ThrPlan), ws its workspace of p.bytes bytes
namespace plan {
struct ThrPlan;
}
hipError_t launch_thresholds(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, double nsigma,
                             const plan::ThrPlan& p, char* ws, int32_t* thr, mkid_thr_stats* stats, hipStream_t s);

// mkid_phase_noise_spectra (k_noise.hip): one launch on stream s; `p` is the plan of n (its passes,
// geometry and table offsets), tab the device image of its tables; spec = acc * mul + add
namespace plan {
struct NoisePlan;
}
hipError_t launch_noise(const int16_t* raw, int64_t ld, int32_t nch, int32_t n_averages, double mul, double add,
                        const plan::NoisePlan& p, const char* tab, double* spec, hipStream_t s);

// mkid_spectrum_lines and mkid_energy_cube (k_wavecal.hip; the rules are wavecal_common.h). The
// calibration runs one workgroup per channel with the row in dynamic LDS (4 nbins bytes); the cube
// is a grid-stride pass as k_obs_count's.
struct WcalLinesArgs {
    const int32_t* spectra;  // [nch][nbins + 3]
    const float* lo;         // [nch]
    const float* step;       // [nch]
    mkid_line_fit* lines;    // [nch][P]
    mkid_energy_cal* cal;    // [nch]
    float* cal_f;            // [nch][4]
    int64_t min_peak;
    double E[MKID_CAL_MAX_LINES];
    int32_t nbins, P, w, min_sep, g, pad;
};
hipError_t launch_spectrum_lines(const WcalLinesArgs& a, int32_t nch, hipStream_t s);
struct WcalCubeArgs {
    const uint64_t* events;  // [n] wide packets
    const float* heights;    // [n]
    const int64_t* d_n;      // nullable: device packet count (pkt::count(d_n, n) packets are read)
    const float* cal_f;      // [C][4]
    int32_t* cube;           // [C][nb + 3]
    float* energy;           // nullable [n]
    int64_t n, j0, j_defer;
    int32_t C, nb, mode, ncu;
    float hc, vlo, vinv, pad;
};
hipError_t launch_energy_cube(const WcalCubeArgs& a, hipStream_t s);

// mkid_fit_loops (k_loopfit.hip; the rules are loopfit_common.h): one workgroup per channel, the
// window in static LDS, one wave per start.
struct LoopfitArgs {
    const double* freq;    // [nch][fsteps]
    const double* i;       // [nch][fsteps]
    const double* q;       // [nch][fsteps]
    const double* isd;     // nullable with qsd
    const double* qsd;
    const double* draws;   // [nch][S][5]
    const double* qguess;  // nullable [nch]
    mkid_loop_fit* fits;   // [nch]
    double* chisq_all;     // nullable [nch][S]
    double wn[10];         // hanning(10) / sum, made on the host
    double ftol;
    int32_t fsteps, S, max_iter, pad;
};
hipError_t launch_fit_loops(const LoopfitArgs& a, int32_t nch, hipStream_t s);

// mkid_fit_mags (k_magfit.hip; the rules are magfit_common.h): one workgroup per channel, the
// sweep's x and normalised magnitude in static LDS, one wave per start.
struct MagfitArgs {
    const double* freq;    // [nch][fsteps]
    const double* i;       // [nch][fsteps]
    const double* q;       // [nch][fsteps]
    const double* draws;   // [nch][S]
    mkid_mag_fit* fits;    // [nch]
    double* qout;          // nullable [nch]
    double* chisq_all;     // nullable [nch][S]
    double wn[10];         // hanning(10) / sum, made on the host
    double ftol;
    int32_t fsteps, S, max_iter, pad;
};
hipError_t launch_fit_mags(const MagfitArgs& a, int32_t nch, hipStream_t s);

// mkid_welch_psd and mkid_iq_noise (k_welch.hip; the rules are welch_common.h). One group of g
// channels c0 .. c0 + g - 1 at one nfft: the strip sums of every channel and strip go to `part`
// [g][nstrips][2][nfft / 2 + 1] (nfft <= MKID_WELCH_LDS_MAX_N: one workgroup per channel and strip,
// one launch; larger: per segment of a strip a column launch and a row launch through `y`
// [g][nstrips][nfft] complex), then one launch adds the strips and writes the densities of bins
// k_lo .. k_hi - 1 to out_a / out_b [c ldo + off + k - k_lo]. The samples are float64 rows (a, b) or,
// with xi set, the phase and amplitude of an int16 IQ record (welch::IqLoader over res and the offsets).
struct WelchArgs {
    const double* a;        // [nch][ld]
    const double* b;        // nullable
    const int16_t* xi;      // [nch][ld]; null: the float64 rows
    const int16_t* xq;
    const double *i0, *q0, *icen, *qcen;   // [nch]
    const mkid_iqnoise_result* res;        // [nch]
    mkid_iqnoise_cfg cfg;
    const double* w;        // [nfft]
    const double* tw;       // [nfft][2]
    double* part;
    double* y;
    double* out_a;
    double* out_b;          // nullable
    int64_t ld, ldo, off, nseg, nstrips;
    double den;             // fs S2
    int32_t nfft, c0, g, k_lo, k_hi, pad;
};
hipError_t launch_welch_group(const WelchArgs& a, hipStream_t s);
// mkid_iq_noise's first and last launch: the exact sums and each channel's constants into res; then
// fn1k, and NaN over the spectra of a channel whose rad is unusable
struct IqNoiseArgs {
    const int16_t* xi;
    const int16_t* xq;
    const double *i0, *q0, *icen, *qcen, *qfit;
    mkid_iqnoise_result* res;
    double* pn;
    double* an;
    mkid_iqnoise_cfg cfg;
    int64_t n, ld;
    int32_t nch, pad;
};
hipError_t launch_iq_means(const IqNoiseArgs& a, hipStream_t s);
hipError_t launch_iq_fn1k(const IqNoiseArgs& a, hipStream_t s);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device), thread-safe: the
// attribute is per device, and several contexts (devices, host threads) may launch concurrently.
// `mask` is one static per kernel instantiation; the call is idempotent, so a race only repeats it.
inline hipError_t ensure_lds_attr(std::atomic<uint64_t>& mask, const void* fn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (mask.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) mask.fetch_or(bit, std::memory_order_acq_rel);
    return e;
}

bool channelize_supported(int N);
// fused PFB..phase front ends: k_front (N = 128 / 256), k_front3 (512 / 1024 / 2048, wave-
// specialised), k_front5 (4096, wave-specialised); fused_supported / launch_fused dispatch by N
bool fused_supported(int N);
hipError_t launch_fused(int N, const FrontArgs& a, hipStream_t s);
// N = 512 / 1024 / 2048: k_front3.hip is built once per N and instantiates that one
template <int N>
hipError_t launch_front3(const FrontArgs& a, hipStream_t s);
hipError_t launch_front5(const FrontArgs& a, hipStream_t s);         // N = 4096 (k_front5.hip)
int64_t front_hist_samples(int N);  // ADC history the fused kernel reads before a chunk

}  // namespace mkid
