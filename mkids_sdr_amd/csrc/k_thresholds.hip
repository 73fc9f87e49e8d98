// mkid_phase_thresholds: the reference's threshold rule (loadThresholds, ROACH_Pulses.py:211-299) for
// every channel of a Fix16_13 phase block [rows][ld] at once. thr_common.h holds the rule; this file
// holds its four stages, all on the caller's stream:
//   k_thr_init    lo = INT32_MAX, hi = INT32_MIN, counts = 0
//   k_thr_range   per-channel min / max: registers down a row block, LDS across a workgroup's row
//                 slots, one integer atomic per channel and workgroup
//   k_thr_count   100-bin histogram per channel: a workgroup builds the cut tables of its strip of 64
//                 channels in LDS (fp64, 99 per channel), bins its row block with integer work only
//                 (a float estimate corrected against the cut table) into LDS tables, and adds those
//                 into the global counts with integer atomics
//   k_thr_finish  fractions, numpy's 101 prefix sums, the two argmins and the threshold
// Integer atomics only: the counts, and so every output bit, do not depend on the schedule.
// Geometry (plan::ThrPlan): a workgroup is COLS column threads x RSLOTS row slots; a column thread
// holds V adjacent channels of a row (V = 8: one 16-byte load). Jobs = strips x row blocks, walked by
// the grid. The block is only read.
#include "mkid_internal.h"
#include "mkid_plan.h"
#include "thr_common.h"

namespace mkid {

using namespace thr;

namespace {

constexpr int kStrip = plan::kThrStrip;
constexpr int kThreads = plan::kThrThreads;
constexpr int kPitch = kBins + 1;   // odd: the lanes of a wave, on different channels, spread over the banks
static_assert(kPitch % 2 == 1, "LDS row pitch");

__global__ void __launch_bounds__(256) k_thr_init(int32_t* lo, int32_t* hi, uint32_t* counts, int64_t nch) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < nch; i += stride) lo[i] = INT32_MAX, hi[i] = INT32_MIN;
    for (int64_t i = t0; i < nch * kBins; i += stride) counts[i] = 0;
}

// V samples of one row: channels c .. c + V - 1
template <int V>
struct RowVec;
template <>
struct RowVec<8> {
    uint4 v;
    __device__ void load(const int16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
    __device__ int32_t get(int k) const {
        const uint32_t w = k < 2 ? v.x : (k < 4 ? v.y : (k < 6 ? v.z : v.w));
        return (int32_t)(int16_t)(k & 1 ? w >> 16 : w & 0xffffu);
    }
};
template <>
struct RowVec<1> {
    int16_t v;
    __device__ void load(const int16_t* p) { v = *p; }
    __device__ int32_t get(int) const { return v; }
};

// The job geometry shared by the range and the count pass: job -> (strip, row block); the thread's
// first channel and whether it holds channels at all.
template <int V>
struct Job {
    static constexpr int COLS = kStrip / V, RSLOTS = kThreads / COLS;
    int64_t r0, r1;     // rows of the block
    int64_t c0;         // first channel of the strip
    int32_t col, rslot; // this thread's place
    int32_t nloc;       // channels of the strip that exist (1..64)
    bool active;        // the thread's V channels exist (whole: cend - cbeg is a multiple of V)
    __device__ Job(int64_t job, int64_t strips, int64_t cbeg, int64_t cend, int64_t B, int64_t rows) {
        const int64_t rb = job / strips, st = job - rb * strips;
        r0 = rb * B;
        r1 = r0 + B < rows ? r0 + B : rows;
        c0 = cbeg + st * kStrip;
        col = (int32_t)threadIdx.x % COLS;
        rslot = (int32_t)threadIdx.x / COLS;
        const int64_t left = cend - c0;
        nloc = (int32_t)(left < kStrip ? left : kStrip);
        active = col * V < nloc;
    }
};

template <int V>
__global__ void __launch_bounds__(256)
k_thr_range(const int16_t* __restrict__ raw, int64_t rows, int64_t ld, int64_t cbeg, int64_t cend, int64_t B,
            int64_t strips, int64_t jobs, int32_t* __restrict__ g_lo, int32_t* __restrict__ g_hi) {
    __shared__ int32_t s_lo[kStrip], s_hi[kStrip];
    for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const Job<V> j(job, strips, cbeg, cend, B, rows);
        if (threadIdx.x < kStrip) s_lo[threadIdx.x] = INT32_MAX, s_hi[threadIdx.x] = INT32_MIN;
        __syncthreads();
        if (j.active) {
            int32_t mn[V], mx[V];
#pragma unroll
            for (int k = 0; k < V; ++k) mn[k] = INT32_MAX, mx[k] = INT32_MIN;
            const int16_t* p = raw + j.c0 + j.col * V;
            for (int64_t r = j.r0 + j.rslot; r < j.r1; r += Job<V>::RSLOTS) {
                RowVec<V> x;
                x.load(p + r * ld);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int32_t s = x.get(k);
                    mn[k] = s < mn[k] ? s : mn[k];
                    mx[k] = s > mx[k] ? s : mx[k];
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                atomicMin(&s_lo[j.col * V + k], mn[k]);
                atomicMax(&s_hi[j.col * V + k], mx[k]);
            }
        }
        __syncthreads();
        if ((int32_t)threadIdx.x < j.nloc) {
            atomicMin(&g_lo[j.c0 + threadIdx.x], s_lo[threadIdx.x]);
            atomicMax(&g_hi[j.c0 + threadIdx.x], s_hi[threadIdx.x]);
        }
        __syncthreads();   // the tables are reset by the next job
    }
}

template <int V>
__global__ void __launch_bounds__(256)
k_thr_count(const int16_t* __restrict__ raw, int64_t rows, int64_t ld, int64_t cbeg, int64_t cend, int64_t B,
            int64_t strips, int64_t jobs, const int32_t* __restrict__ g_lo, const int32_t* __restrict__ g_hi,
            uint32_t* __restrict__ g_counts) {
    __shared__ int32_t s_cut[kStrip * kPitch];    // [ch][0..100]: INT32_MIN, cut 1..99, INT32_MAX
    __shared__ uint32_t s_cnt[kStrip * kPitch];   // [ch][0..99]
    __shared__ Range s_rng[kStrip];
    __shared__ int32_t s_lo[kStrip];
    __shared__ float s_inv[kStrip], s_off[kStrip];   // the bin estimate (x - lo) inv + off
    for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
        const Job<V> j(job, strips, cbeg, cend, B, rows);
        // the strip's tables: cut points in fp64 from lo / hi, once per channel and workgroup
        if ((int32_t)threadIdx.x < j.nloc) {
            const int32_t lo = g_lo[j.c0 + threadIdx.x], hi = g_hi[j.c0 + threadIdx.x];
            s_rng[threadIdx.x] = make_range(lo, hi);
            s_lo[threadIdx.x] = lo;
            // a constant channel's samples all sit at the middle of its unit-wide range
            s_inv[threadIdx.x] = hi > lo ? (float)kBins / (float)(hi - lo) : 0.f;
            s_off[threadIdx.x] = hi > lo ? 0.f : (float)(kBins / 2);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < kStrip * kPitch; e += kThreads) {
            const int ch = e / kPitch, i = e - ch * kPitch;
            s_cnt[e] = 0;
            int32_t c = i == 0 ? INT32_MIN : INT32_MAX;
            if (ch < j.nloc && i > 0 && i < kBins) c = cut(s_rng[ch], i);
            s_cut[e] = c;
        }
        __syncthreads();
        if (j.active) {
            const int16_t* p = raw + j.c0 + j.col * V;
            const int cl = j.col * V;
            int32_t lo[V];
            float inv[V], off[V];
#pragma unroll
            for (int k = 0; k < V; ++k) lo[k] = s_lo[cl + k], inv[k] = s_inv[cl + k], off[k] = s_off[cl + k];
            for (int64_t r = j.r0 + j.rslot; r < j.r1; r += Job<V>::RSLOTS) {
                RowVec<V> x;
                x.load(p + r * ld);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int32_t s = x.get(k);
                    int b = (int)((float)(s - lo[k]) * inv[k] + off[k]);
                    b = b < 0 ? 0 : (b > kBins - 1 ? kBins - 1 : b);
                    b = bin_of(s, &s_cut[(cl + k) * kPitch], b);
                    atomicAdd(&s_cnt[(cl + k) * kPitch + b], 1u);
                }
            }
        }
        __syncthreads();
        // [nloc][100] of the strip is contiguous in the global table: 256 contiguous bytes per wave
        for (int e = threadIdx.x; e < j.nloc * kBins; e += kThreads) {
            const int ch = e / kBins, i = e - ch * kBins;
            const uint32_t n = s_cnt[ch * kPitch + i];
            if (n) atomicAdd(&g_counts[j.c0 * kBins + e], n);
        }
        __syncthreads();   // the tables are rebuilt by the next job
    }
}

// One workgroup finishes kFinCh channels; kFinParts threads share a channel's 101 prefix sums
// (edges part, part + kFinParts, ...), and the first of them merges their picks in index order.
constexpr int kFinCh = plan::kThrFinishCh, kFinParts = 256 / kFinCh;
static_assert(kFinCh * kFinParts == 256, "finish geometry");

struct FracRow {
    const double* n;
    __device__ double operator()(int i) const { return n[i]; }
};

__global__ void __launch_bounds__(256)
k_thr_finish(const int32_t* __restrict__ g_lo, const int32_t* __restrict__ g_hi,
             const uint32_t* __restrict__ g_counts, int64_t rows, int64_t nch, double nsigma,
             int32_t* __restrict__ thr, mkid_thr_stats* __restrict__ stats) {
    __shared__ double s_n[kFinCh * kPitch];
    __shared__ Pick s_pick[kFinCh * kFinParts];
    const int64_t c0 = (int64_t)blockIdx.x * kFinCh;
    const int nloc = (int)(nch - c0 < kFinCh ? nch - c0 : kFinCh);
    for (int e = threadIdx.x; e < nloc * kBins; e += 256) {
        const int ch = e / kBins, i = e - ch * kBins;
        s_n[ch * kPitch + i] = fraction(g_counts[c0 * kBins + e], rows);
    }
    __syncthreads();
    const int ch = threadIdx.x / kFinParts, part = threadIdx.x % kFinParts;
    if (ch < nloc) s_pick[threadIdx.x] = pick_scan(FracRow{&s_n[ch * kPitch]}, part, kFinParts);
    __syncthreads();
    if (ch < nloc && part == 0) {
        Pick p = s_pick[threadIdx.x];
        for (int q = 1; q < kFinParts; ++q) pick_merge(p, s_pick[threadIdx.x + q]);
        mkid_thr_stats st;
        thr[c0 + ch] = finish(g_lo[c0 + ch], g_hi[c0 + ch], p, nsigma, &st);
        if (stats) stats[c0 + ch] = st;
    }
}

template <int V>
hipError_t launch_pass(const int16_t* raw, int64_t rows, int64_t ld, int64_t cbeg, int64_t cend,
                       const plan::ThrPlan& p, int64_t strips, int64_t grid, int32_t* lo, int32_t* hi,
                       uint32_t* counts, bool count, hipStream_t s) {
    if (grid <= 0) return hipSuccess;
    const int64_t jobs = strips * p.row_blocks;
    if (count)
        k_thr_count<V><<<dim3((unsigned)grid), dim3(kThreads), 0, s>>>(raw, rows, ld, cbeg, cend, p.B, strips, jobs,
                                                                       lo, hi, counts);
    else
        k_thr_range<V><<<dim3((unsigned)grid), dim3(kThreads), 0, s>>>(raw, rows, ld, cbeg, cend, p.B, strips, jobs,
                                                                       lo, hi);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_thresholds(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, double nsigma,
                             const plan::ThrPlan& p, char* ws, int32_t* thr, mkid_thr_stats* stats, hipStream_t s) {
    int32_t* lo = (int32_t*)(ws + p.off_lo);
    int32_t* hi = (int32_t*)(ws + p.off_hi);
    uint32_t* counts = (uint32_t*)(ws + p.off_counts);
    k_thr_init<<<dim3((unsigned)p.grid_init), dim3(256), 0, s>>>(lo, hi, counts, nch);
    hipError_t e = hipGetLastError();
    for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
        if (p.vec == 8)
            e = launch_pass<8>(raw, rows, ld, 0, p.nch_vec, p, p.strips_vec, p.grid_vec, lo, hi, counts, pass, s);
        if (e == hipSuccess)
            e = launch_pass<1>(raw, rows, ld, p.nch_vec, nch, p, p.strips_tail, p.grid_tail, lo, hi, counts, pass, s);
    }
    if (e != hipSuccess) return e;
    k_thr_finish<<<dim3((unsigned)p.grid_finish), dim3(256), 0, s>>>(lo, hi, counts, rows, nch, nsigma, thr, stats);
    return hipGetLastError();
}

}  // namespace mkid
