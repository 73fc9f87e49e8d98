// The collectives of a wave and of a workgroup, one definition for every kernel that scans, ranks or
// reduces. Device code only. A workgroup is nw full waves of 64; op is any associative (a, b) -> a op b
// and id its identity over the values in use.
//   wave total  lane 63's inclusive value after a scan, any lane's value after a reduction, a rank's count;
//   before      the wave totals of the waves before mine, folded in ascending wave order from id;
//   total       all nw wave totals folded in ascending wave order, the same in every thread.
// The shuffle orders are part of the contract: a scan takes offsets 1, 2, .., 32 and a reduction
// 32, 16, .., 1, each step x = op(x, the other lane's x). Floating-point callers (k_heights; the sums
// of lm_common.h, which keeps its own copy of the loop) have their result's bits from that order.
// LDS: the caller declares ws[nw]. fold_waves has one barrier, after the store: a caller that writes
// ws again (a loop, a second fold) puts one __syncthreads() in between, any other caller pays none.
#pragma once
#include <hip/hip_runtime.h>

namespace mkid {
namespace wg {

struct Add { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
// b wins only where b > a: a NaN never wins
struct Max { template <class T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };
// Inclusive scan over the wave: lane l gets x_0 op .. op x_l.
template <class T, class Op>
__device__ __forceinline__ T wave_scan(T x, T id, Op op) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(x, off, 64);
        x = op(x, (int)(threadIdx.x & 63) >= off ? y : id);
    }
    return x;
}
// Butterfly reduction over the wave: every lane ends with the same bits.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T x, Op op) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = op(x, __shfl_xor(x, m, 64));
    return x;
}
// The lanes of the wave whose predicate holds: how many are below this lane, and how many there are.
struct Rank { int below, count; };
__device__ __forceinline__ Rank wave_rank(bool p) {
    const uint64_t m = __ballot(p);
    return Rank{(int)__popcll(m & (((uint64_t)1 << (threadIdx.x & 63)) - 1)), (int)__popcll(m)};
}
// The workgroup step: the wave's `owner` lane stores the wave total `mine`, one barrier, every thread folds.
template <class T, class Op>
__device__ __forceinline__ void fold_waves(bool owner, T mine, T* ws, int nw, T id, Op op, T& before, T& total) {
    const int w = threadIdx.x >> 6;
    if (owner) ws[w] = mine;
    __syncthreads();
    before = id, total = id;
    for (int i = 0; i < nw; ++i) {
        const T v = ws[i];
        before = op(before, i < w ? v : id);
        total = op(total, v);
    }
}
// Reduction over the workgroup, the same bits in every thread.
template <class T, class Op>
__device__ __forceinline__ T reduce(T x, T* ws, int nw, T id, Op op) {
    T before, total;
    fold_waves((threadIdx.x & 63) == 0, wave_reduce(x, op), ws, nw, id, op, before, total);
    return total;
}

}  // namespace wg
}  // namespace mkid
