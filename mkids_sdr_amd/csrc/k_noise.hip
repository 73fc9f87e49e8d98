// mkid_phase_noise_spectra: every channel's phase-noise spectrum from a Fix16_13 block [rows][ld]
// (include/mkidgpu.h states the rule). One workgroup per channel. Per pair of
// pieces (a, a + 1) it
//   loads the two columns as z[j] = (x_a[j], x_{a+1}[j]), float32 pairs in LDS, takes the rounded
//   integer mean off each (noise_common.h round_mean; exact, only bin 0 changes and bin 0 is the
//   integer sum),
//   runs the in-place mixed-radix passes of the plan: every thread computes the outputs at its
//   positions tid + i T into registers (noise::pass_output: r LDS reads of the piece, r reads of
//   the pass's radix table staged in LDS, one n-table twiddle), barrier, writes them, barrier,
//   unpacks the two spectra at its positions (the partner position is tabulated) and adds
//   log2 |X|^2 of a, then of a + 1, to the position's float64 accumulator in a register.
// A thread owns the same positions for the whole channel, so the pieces are added in a fixed order
// by one thread and nothing is accumulated in memory. The end writes spec[c][bin_of_pos[p]].
//
// The column of a time-major block is a stride-2 ld walk: every 2-byte load touches a line of its
// own. Nothing is transposed; the 32 channels of a 64-byte line go to workgroups that start
// together on one XCD (plan::noise_channel_of_block) and share the line in that XCD's L2.
// LDS: a wave's positions are consecutive, so with M >= 64 its piece reads are consecutive 8-byte
// words (ds_read_b64, conflict-free) and its lanes share t, i.e. the radix-table word (broadcast).
// In the late passes (M < 64) lanes with equal (b, j) read the same word and the groups lie r M
// words apart: conflict-free for odd r M, two-way for the last radix-4 pass.
// More than 64 KiB of LDS per workgroup needs the dynamic-LDS attribute (ensure_lds_attr).
#include <hip/hip_runtime.h>

#include <atomic>

#include "mkid_internal.h"
#include "mkid_plan.h"
#include "noise_common.h"

namespace mkid {
namespace {

using noise::Cx;
using noise::Pass;
constexpr int kStageR = plan::kNoiseStageR;

struct NoiseArgs {
    const int16_t* raw;
    int64_t ld, nch, blocks;
    int32_t n, n_averages, npass;
    double mul, add;
    const Cx<float>* wn;
    const Cx<float>* wr;
    const uint16_t* bin_of_pos;
    const uint16_t* partner;
    double* spec;
    Pass pass[noise::kMaxPasses];
};

struct LdsCx {
    const Cx<float>* p;
    __device__ Cx<float> operator()(int32_t i) const { return p[i]; }
};
struct GlobalCx {
    const Cx<float>* p;
    __device__ Cx<float> operator()(int32_t i) const { return p[i]; }
};

template <int T, int kPer>
__global__ __launch_bounds__(T) void k_noise(const NoiseArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    Cx<float>* z = (Cx<float>*)s_dyn;          // [n]
    Cx<float>* s_wr = z + a.n;                  // [kStageR]
    int32_t* s_red = (int32_t*)(s_wr + kStageR);   // [waves][4]
    constexpr int nw = T >> 6;
    const int tid = threadIdx.x;
    const int32_t n = a.n;
    for (int64_t blk = blockIdx.x; blk < a.blocks; blk += gridDim.x) {
        const int64_t c = plan::noise_channel_of_block(blk);
        if (c >= a.nch) continue;   // the whole workgroup
        double acc[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) acc[i] = 0.0;
        for (int32_t pa = 0; pa < a.n_averages; pa += 2) {
            const bool paired = pa + 1 < a.n_averages;
            const int16_t* colA = a.raw + (int64_t)pa * n * a.ld + c;
            const int16_t* colB = colA + (int64_t)n * a.ld;
            const int32_t fa = colA[0], fb = paired ? colB[0] : 0;
            int32_t sa = 0, sb = 0, va = 0, vb = 0;   // sums, and OR of x ^ x[0] (0: a flat piece)
            int32_t j0 = tid;
            asm volatile("" : "+v"(j0));   // the row offsets are made here, not kept across the pairs
#pragma unroll 4
            for (int32_t j = j0; j < n; j += T) {
                const int32_t xa = colA[(int64_t)j * a.ld], xb = paired ? colB[(int64_t)j * a.ld] : 0;
                sa += xa, sb += xb;
                va |= xa ^ fa, vb |= xb ^ fb;
                z[j] = Cx<float>{(float)xa, (float)xb};
            }
            for (int o = 32; o > 0; o >>= 1) {
                sa += __shfl_xor(sa, o, 64), sb += __shfl_xor(sb, o, 64);
                va |= __shfl_xor(va, o, 64), vb |= __shfl_xor(vb, o, 64);
            }
            if ((tid & 63) == 0) {
                int32_t* r = s_red + 4 * (tid >> 6);
                r[0] = sa, r[1] = sb, r[2] = va, r[3] = vb;
            }
            __syncthreads();
            sa = 0, sb = 0, va = 0, vb = 0;
            for (int w = 0; w < nw; ++w) {
                const int32_t* r = s_red + 4 * w;
                sa += r[0], sb += r[1], va |= r[2], vb |= r[3];
            }
            // the same in every lane: kept in scalar registers over the passes
            sa = __builtin_amdgcn_readfirstlane(sa), sb = __builtin_amdgcn_readfirstlane(sb);
            va = __builtin_amdgcn_readfirstlane(va), vb = __builtin_amdgcn_readfirstlane(vb);
            const float oa = (float)noise::round_mean(sa, n), ob = (float)noise::round_mean(sb, n);
            for (int32_t j = tid; j < n; j += T) z[j].re -= oa, z[j].im -= ob;   // the thread's own elements
            __syncthreads();
            for (int32_t s = 0; s < a.npass; ++s) {
                const Pass ps = a.pass[s];
                const bool staged = ps.r <= kStageR;
                if (staged) {
                    for (int32_t q = tid; q < ps.r; q += T) s_wr[q] = a.wr[ps.tw_off + q];
                    __syncthreads();
                }
                Cx<float> y[kPer];
#pragma unroll
                for (int i = 0; i < kPer; ++i) {
                    int32_t p = tid + i * T;
                    // one output after the other: otherwise the index arithmetic of all kPer outputs
                    // is hoisted in front of the first and the 1024-thread kernel runs out of registers
                    if (i > 0) asm volatile("" : "+v"(p) : "v"(y[i - 1].re), "v"(y[i - 1].im));
                    if (p < n)
                        y[i] = staged ? noise::pass_output<float>(ps, p, LdsCx{z}, LdsCx{s_wr}, GlobalCx{a.wn})
                                      : noise::pass_output<float>(ps, p, LdsCx{z}, GlobalCx{a.wr + ps.tw_off},
                                                                  GlobalCx{a.wn});
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < kPer; ++i) {
                    const int32_t p = tid + i * T;
                    if (p < n) z[p] = y[i];
                }
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < kPer; ++i) {
                int32_t p = tid + i * T;
                if (i > 0) asm volatile("" : "+v"(p) : "v"(acc[i - 1]));   // as above
                if (p < n) {
                    float pw_a, pw_b;
                    noise::bin_power(a.bin_of_pos[p] == 0, z[p], z[a.partner[p]], sa, sb, va == 0, vb == 0, pw_a, pw_b);
                    acc[i] += (double)log2f(pw_a);
                    if (paired) acc[i] += (double)log2f(pw_b);
                }
            }
            __syncthreads();   // the next pair overwrites z and s_red
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            int32_t p = tid + i * T;
            asm volatile("" : "+v"(p));   // as above: keeps the kPer addresses out of the channel loop
            if (p < n) a.spec[c * n + a.bin_of_pos[p]] = noise::finish(acc[i], a.mul, a.add);
        }
    }
}

}  // namespace

hipError_t launch_noise(const int16_t* raw, int64_t ld, int32_t nch, int32_t n_averages, double mul, double add,
                        const plan::NoisePlan& p, const char* tab, double* spec, hipStream_t s) {
    static std::atomic<uint64_t> lds_small{0}, lds_large{0};
    const int max_lds = 8 * MKID_NOISE_MAX_N + 8 * kStageR + 16 * 16;
    const bool large = p.threads == plan::kNoiseThreadsLarge;
    if (!large && p.threads != plan::kNoiseThreadsSmall) return hipErrorInvalidValue;
    const void* fn = large ? (const void*)k_noise<plan::kNoiseThreadsLarge, plan::kNoisePerLarge>
                           : (const void*)k_noise<plan::kNoiseThreadsSmall, plan::kNoisePerSmall>;
    hipError_t e = ensure_lds_attr(large ? lds_large : lds_small, fn, max_lds);
    if (e != hipSuccess) return e;
    if (p.lds_bytes > max_lds || (int64_t)p.threads * p.per_thread < p.n || (int)p.passes.size() > noise::kMaxPasses)
        return hipErrorInvalidValue;
    NoiseArgs a{};
    a.raw = raw, a.ld = ld, a.nch = nch, a.blocks = plan::noise_blocks(nch);
    a.n = p.n, a.n_averages = n_averages, a.npass = (int32_t)p.passes.size();
    a.mul = mul, a.add = add;
    a.wn = (const Cx<float>*)(tab + p.off_wn), a.wr = (const Cx<float>*)(tab + p.off_wr);
    a.bin_of_pos = (const uint16_t*)(tab + p.off_bin), a.partner = (const uint16_t*)(tab + p.off_partner);
    a.spec = spec;
    for (int i = 0; i < a.npass; ++i) a.pass[i] = p.passes[(size_t)i];
    const int64_t grid = std::min(a.blocks, plan::kNoiseMaxGrid);
    if (large)
        k_noise<plan::kNoiseThreadsLarge, plan::kNoisePerLarge>
            <<<dim3((unsigned)grid), dim3(plan::kNoiseThreadsLarge), (size_t)p.lds_bytes, s>>>(a);
    else
        k_noise<plan::kNoiseThreadsSmall, plan::kNoisePerSmall>
            <<<dim3((unsigned)grid), dim3(plan::kNoiseThreadsSmall), (size_t)p.lds_bytes, s>>>(a);
    return hipGetLastError();
}

}  // namespace mkid
