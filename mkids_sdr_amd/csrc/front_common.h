// The stages the fused front ends share (k_front.hip, k_front3.hip, k_front5.hip), one definition
// each: run geometry and grid sizing, the ADC hop loader, the ring-plane store, the exact int16 PFB
// dot product, the PFB + in-wave 512-point sub-FFT, the packed low-pass step, the Fix16_13
// quantiser (also k_lpf_phase.hip), the IQ-tap word and the timing-build stamp macro. The kernels
// keep what differs between them: geometry, wave roles, scheduling fences, bin select and stores.
#pragma once
#include "fft_common.h"
#include "mkid_internal.h"

// MKID_XP_STAMPS (timing experiments only, tools/stamps.py / stamps4.py): lane 0 of every wave of
// the first 4 workgroups records s_memtime at point slot_ (0..15) of iterations first_ .. first_ + 7
// into the phase buffer (which then holds no phases); it_ is the kernel's iteration counter.
#ifdef MKID_XP_STAMPS
#define FRONT_STAMP(it_, first_, slot_)                                                           \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        const uint64_t tm_ = __builtin_amdgcn_s_memtime();                                        \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (blockIdx.x < 4 && (it_) >= (first_) && (it_) < (first_) + 8 && (threadIdx.x & 63) == 0) \
            reinterpret_cast<uint64_t*>(a.phase)[((blockIdx.x * 16 + (threadIdx.x >> 6)) * 8 +   \
                                                  ((it_) - (first_))) * 16 + (slot_)] = tm_;       \
    } while (0)
#else
#define FRONT_STAMP(it_, first_, slot_) ((void)0)
#endif

namespace mkid {
namespace {

// ---- run geometry ----
// ADC samples a fused kernel reads before a chunk (hop = M samples): the PFB's 2T - 1 earlier hops
// and the kLpfHist warm-up frames that rebuild the low-pass history
constexpr int64_t front_hist(int M) { return (int64_t)(2 * kPfbTaps - 1 + kLpfHist) * M; }

// The run of frames [k_b, k_e) a workgroup owns; it computes from k_start (warm-up, no output)
struct FrontRun {
    int64_t k_b, k_e, k_start;
    int nrun;
    __device__ __forceinline__ explicit FrontRun(const FrontArgs& a) {
        k_b = (int64_t)blockIdx.x * a.frames_per_block;
        k_e = k_b + a.frames_per_block;
        if (k_e > a.K) k_e = a.K;
        k_start = k_b - kLpfHist;
        nrun = (int)(k_e - k_b);
    }
    __device__ __forceinline__ bool empty() const { return k_b >= k_e; }
};

// Host: frames per run for about `runs` runs over the chunk, at least 64 (the 24-frame warm-up is
// amortised) and at most max_frames, rounded up to `multiple`; sets a.frames_per_block and
// returns the grid size
inline int64_t front_grid(FrontArgs& a, int64_t runs, int64_t max_frames, int64_t multiple) {
    int64_t fpb = a.K / runs;
    fpb = fpb < 64 ? 64 : (fpb > max_frames ? max_frames : fpb);
    fpb = (fpb + multiple - 1) / multiple * multiple;
    a.frames_per_block = fpb;
    return (a.K + fpb - 1) / fpb;
}

// ---- hop loader ----
// W 16-byte words (4 W samples) at sample tid * 4 W of the hops starting at first_hop: non-temporal
// loads from the chunk (every ADC byte is read once), the call's history (the last front_hist
// samples of the previous call) before it, zeros past the chunk's end
template <int W>
struct Hop {
    uint4 v[W];
};
template <int M, int W>
__device__ __forceinline__ Hop<W> front_load(const FrontArgs& a, int64_t first_hop, int tid) {
    Hop<W> h;
    const int64_t s0 = first_hop * M + (int64_t)tid * (4 * W);
    if (s0 >= a.K * M) {
#pragma unroll
        for (int w = 0; w < W; ++w) h.v[w] = make_uint4(0, 0, 0, 0);
    } else if (s0 >= -a.avail) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 p[W];
#pragma unroll
        for (int w = 0; w < W; ++w) p[w] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.x + s0 + 4 * w));
#pragma unroll
        for (int w = 0; w < W; ++w) h.v[w] = make_uint4(p[w].x, p[w].y, p[w].z, p[w].w);
    } else {
        const uint32_t* x = a.xhist + (s0 + a.avail + front_hist(M));
#pragma unroll
        for (int w = 0; w < W; ++w) h.v[w] = *reinterpret_cast<const uint4*>(x + 4 * w);
    }
    return h;
}

// front_load<M, 1> as one unconditional load (no branch around it, so that the compiler's wait for
// it can count the loads issued after it): the address is selected, and a load past the chunk's
// end reads the chunk's first word and is zeroed by the caller where it is used (past)
struct Load4 {
    uint4 v;
    bool past;
};
template <int M>
__device__ __forceinline__ Load4 front_load4_nb(const FrontArgs& a, int64_t first_hop, int tid) {
    const int64_t s0 = first_hop * M + (int64_t)tid * 4;
    const bool past = s0 >= a.K * M;
    const uint32_t* p = s0 >= -a.avail ? a.x + (past ? 0 : s0) : a.xhist + (s0 + a.avail + front_hist(M));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return Load4{make_uint4(v.x, v.y, v.z, v.w), past};
}

// ---- ring planes (k_front3, k_front5) ----
// Paired plane index: plane index i = 64 j + l (j = 0..3) at 128 (j >> 1) + 2 l + (j & 1), so a
// lane's PFB points j and j + 1 are one ds_read_b64 (conflict-free: 32 lanes x 2 dwords)
__device__ __forceinline__ int ring3_idx(int i) { return 128 * (i >> 7) + 2 * (i & 63) + ((i >> 6) & 1); }

// A hop of M = 256 NW samples is NW planes of 256: sample o lives in plane o mod NW at
// ring3_idx(o / NW). Stores the 4 W consecutive samples of h at o (a multiple of 4 W; NW divides
// 4 W): ds_write_b32 with at most 2-way bank conflicts, which cost no extra cycles for
// ds_write_b32 (MI355X_MICROARCH.md §LDS). Plane indices o / NW + d, d < 4, stay within one group
// of 64, so they sit 2 d after the first.
template <int NW, int W>
__device__ __forceinline__ void ring_put(uint32_t* hop, int o, const Hop<W>& h) {
    static_assert((4 * W) % NW == 0, "ring layout");
    uint32_t* p = hop + ring3_idx(o / NW);
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t x[4] = {h.v[w].x, h.v[w].y, h.v[w].z, h.v[w].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) p[((4 * w + i) % NW) * 256 + 2 * ((4 * w + i) / NW)] = x[i];
    }
}

// ---- PFB ----
typedef short fshort2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ fshort2_t as_s2(uint32_t v) { return __builtin_bit_cast(fshort2_t, v); }
// First dot product of a chain, h.lo * x.lo + h.hi * x.hi exact in int32: the VOP3P form with an
// inline-constant zero accumulator (the compiler otherwise picks v_dot2c_i32_i16 behind a v_mov of 0)
__device__ __forceinline__ int32_t dot2_first(uint32_t h, uint32_t x) {
    int32_t d;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(h), "v"(x));
    return d;
}

// One PFB point: u = sum_tau h_tau x_tau for the T = 4 packed int16 I/Q words x (low halves I,
// high halves Q) and the point's taps h = {h0 | h1 << 16, h2 | h3 << 16}, exact, as float (I, Q)
__device__ __forceinline__ float2 pfb_dot(uint2 h, const uint32_t (&x)[kPfbTaps]) {
    static_assert(kPfbTaps == 4, "two int16 tap pairs per point");
    // the I (0x05040100) or Q (0x07060302) halves of two words: lo16 from the second, hi16 from the first
    constexpr uint32_t kPermI = 0x05040100u, kPermQ = 0x07060302u;
    const uint32_t i01 = __builtin_amdgcn_perm(x[1], x[0], kPermI);
    const uint32_t q01 = __builtin_amdgcn_perm(x[1], x[0], kPermQ);
    const uint32_t i23 = __builtin_amdgcn_perm(x[3], x[2], kPermI);
    const uint32_t q23 = __builtin_amdgcn_perm(x[3], x[2], kPermQ);
    int32_t ai = dot2_first(h.x, i01);
    ai = __builtin_amdgcn_sdot2(as_s2(h.y), as_s2(i23), ai, false);
    int32_t aq = dot2_first(h.x, q01);
    aq = __builtin_amdgcn_sdot2(as_s2(h.y), as_s2(q23), aq, false);
    return make_float2((float)ai, (float)aq);
}

// ---- in-wave 512-point sub-FFT (k_front3, k_front5) ----
// Y_w[k] of a 512-point sub-FFT at k ^ ((k >> 2) & 14) of its region: the stage-3 writes and the
// select's bin-indexed reads are both conflict-free or near it (tools/front_layouts.py)
__device__ __forceinline__ int yswz(int k) { return k ^ ((k >> 2) & 14); }

// T1 through the wave's own LDS region: element (lane 8 kl + la, register r) goes to (lane 8 r + la,
// register kl). Lane L writes register r at 72 r + L; lane L' reads register r' at 72 (L' >> 3) +
// 8 r' + (L' & 7). Both patterns are bank-conflict-free for ds_*_b64 (writes: 32 consecutive
// entries; reads: entries 8 (r + r') + la mod 32 distinct over a lane group, r = L' >> 3 < 4
// there), every offset an immediate. 8 writes + 8 reads replace 32 VALU cross-lane moves (DPP
// row_ror:8 + v_permlane16/32_swap), which cost more on VALU-issue-bound transform waves
// (-3.9 % k_front3 at N = 2048, round 3: DESIGN.md §5.2).
__device__ __forceinline__ void t1_lds(float2 (&v)[8], float2* reg, int L) {
#pragma unroll
    for (int r = 0; r < 8; ++r) reg[72 * r + L] = v[r];
    __builtin_amdgcn_wave_barrier();
    const float2* rd = reg + 72 * (L >> 3) + (L & 7);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = rd[8 * r];
    __builtin_amdgcn_wave_barrier();
}

// PFB + 512-point sub-FFT of one wave (lane L): the frame whose oldest hop sits in ring slot sb
// (RS slots of M words), the sub-FFT whose ring plane starts at word `plane` of each hop, taps tq
// of the lane's 8 points, stage twiddles w1 = W_512^{L k}, w2 = W_64^{(L & 7) k}. 2 T ds_read_b64
// pairs, 8 pfb_dots, three radix-8 stages through t1_lds and the 72-stride transpose in `reg`.
// Leaves stage 3's outputs in v: v[r] = Y[64 r + e], e = (L >> 3) + 8 (L & 7), which the caller
// stores at reg + yswz(64 r + e) = reg + (e ^ ((L & 7) << 1)) + 64 r.
template <int M, int RS>
__device__ __forceinline__ void pfb_fft512(const uint32_t* ring, int sb, int plane, const uint2 (&tq)[8],
                                           const float2 (&w1)[7], const float2 (&w2)[7], float2* reg, int L,
                                           float2 (&v)[8]) {
    constexpr int T = kPfbTaps;
    uint32_t xr[8][T];
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
        for (int tau = 0; tau < T; ++tau) {
            int sl = sb + 2 * tau + hi;
            sl -= sl >= RS ? RS : 0;
            const uint32_t* pl = ring + sl * M + plane + 2 * L;
            const uint2 p01 = *reinterpret_cast<const uint2*>(pl);
            const uint2 p23 = *reinterpret_cast<const uint2*>(pl + 128);
            xr[4 * hi + 0][tau] = p01.x;
            xr[4 * hi + 1][tau] = p01.y;
            xr[4 * hi + 2][tau] = p23.x;
            xr[4 * hi + 3][tau] = p23.y;
        }
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = pfb_dot(tq[r], xr[r]);
    const int la = L & 7, kl = L >> 3;
    dft<8>(v);
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul_pk(v[k], w1[k - 1]);
    t1_lds(v, reg, L);
    dft<8>(v);
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul_pk(v[k], w2[k - 1]);
    float2* t2w = reg + 72 * kl + la;
    const float2* t2r = reg + 72 * kl + 9 * la;
#pragma unroll
    for (int r = 0; r < 8; ++r) t2w[9 * r] = v[r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = t2r[r];
    dft<8>(v);
    __builtin_amdgcn_wave_barrier();
}

// ---- output tail ----
// Transposed decimating low-pass over 13 complex accumulators per channel and the uniform tap
// pairs gp[m] = tap_pair(g_2m, g_2m+1): an even frame 2j adds g_{2m+1} z to output j + m; an odd
// frame 2j + 1 adds g_{2m} z, completes output j (returned in y) and shifts:
// y_j = sum_i g_i z_{2j+1-i}. Taps outer, channels inner; a caller that wants one channel at a time
// uses the single-channel forms below.
template <int CPT>
__device__ __forceinline__ void lpf_even(const uint64_t (&gp)[13], const float2 (&z)[CPT], float2 (&acc)[CPT][13]) {
#pragma unroll
    for (int m = 0; m < 13; ++m)
#pragma unroll
        for (int q = 0; q < CPT; ++q) acc[q][m] = fma_tap<1>(gp[m], z[q], acc[q][m]);
}
template <int CPT>
__device__ __forceinline__ void lpf_odd(const uint64_t (&gp)[13], const float2 (&z)[CPT], float2 (&acc)[CPT][13],
                                        float2 (&y)[CPT]) {
#pragma unroll
    for (int q = 0; q < CPT; ++q) y[q] = fma_tap<0>(gp[0], z[q], acc[q][0]);
#pragma unroll
    for (int m = 0; m < 12; ++m)
#pragma unroll
        for (int q = 0; q < CPT; ++q) acc[q][m] = fma_tap<0>(gp[m + 1], z[q], acc[q][m + 1]);
#pragma unroll
    for (int q = 0; q < CPT; ++q) acc[q][12] = make_float2(0.f, 0.f);
}
__device__ __forceinline__ void lpf_even(const uint64_t (&gp)[13], float2 z, float2 (&acc)[13]) {
    lpf_even<1>(gp, reinterpret_cast<const float2(&)[1]>(z), reinterpret_cast<float2(&)[1][13]>(acc));
}
__device__ __forceinline__ float2 lpf_odd(const uint64_t (&gp)[13], float2 z, float2 (&acc)[13]) {
    float2 y[1];
    lpf_odd<1>(gp, reinterpret_cast<const float2(&)[1]>(z), reinterpret_cast<float2(&)[1][13]>(acc), y);
    return y[0];
}

// Fix16_13: raw = clamp(rint(phi 2^13), +-pi 2^13) (ROACH_Pulses.py:274-278)
__device__ __forceinline__ int16_t fix16_13(float ph) {
    constexpr int kPi13 = 25736;
    const int q = __float2int_rn(ph * 8192.0f);
    return (int16_t)(q < -kPi13 ? -kPi13 : (q > kPi13 ? kPi13 : q));
}

// IQ snapshot tap (conv_phase_snapIQ_bram): the (I, Q) int16 pair of the tap channel's centred
// low-pass output y', one 32-bit word of iqtap[row]
__device__ __forceinline__ uint32_t iq_tap_word(const Centring& cen, float2 y) {
    return (uint32_t)(uint16_t)iq16(y.x + cen.tap_off.x) | ((uint32_t)(uint16_t)iq16(y.y + cen.tap_off.y) << 16);
}

}  // namespace
}  // namespace mkid
