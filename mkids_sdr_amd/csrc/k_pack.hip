// A settled second out of its slot, and the slot made free (include/mkidgpu.h mkid_pack_second,
// mkid_clear_second; the rules are obs_common.h pack_host, clear_host).
//
// The slot is rows row0 .. row0 + C - 1 of the [n_slots][C][K] tables, row0 = (sec mod n_slots) C,
// and row c holds m_c = row_fill(image[row0 + c], K) photons. The order between the steps comes
// from the kernel boundaries alone:
// k_pk_scan   one workgroup: counts[c] = the raw count, offsets = the exclusive prefix sum of m_c
//             (kPackPer consecutive channels a thread, wg::wave_scan, the fold here); thread 0: offsets[C], total.
// k_pk_copy   a wave per (channel, tile of kPackTile slots), a wave whose tile starts at or past
//             m_c leaving at once, so that one long row is spread over many waves and many short
//             rows cost a wave each. The lanes walk consecutive slots: the loads from the row and
//             the stores to offsets[c] + slot of the packed arrays are both contiguous. An entry at
//             or past cap_out is not written.
// k_pk_nan    mkid_clear_second, the same grid: the first m_c heights (and dt) get the NaN the
//             tables are pre-filled with.
// k_pk_zero   then image[row0 + c] = 0, after every wave of k_pk_nan has read its count.
// No atomics, no scratch, nothing read back by the host.
#include "mkid_internal.h"
#include "obs_common.h"
#include "wg_common.h"

namespace mkid {

constexpr int kPackThreads = 256;                     // k_pk_copy, k_pk_nan: kPackThreads / 64 waves
constexpr int kPackScanThreads = 1024, kPackPer = 4;  // 4096 channels at the most
static_assert(kPackScanThreads * kPackPer >= 4096, "the scan is one workgroup");

__global__ __launch_bounds__(kPackScanThreads) void k_pk_scan(PackArgs a) {
    __shared__ int64_t wsum[kPackScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t m[kPackPer], x = 0;
#pragma unroll
    for (int j = 0; j < kPackPer; ++j) {
        const int c = t * kPackPer + j;
        m[j] = 0;
        if (c < a.C) {
            const int32_t count = a.image[a.row0 + c];
            a.counts[c] = count;
            m[j] = obs::row_fill(count, a.K);
        }
        x += m[j];
    }
    const int64_t inc = wg::wave_scan(x, (int64_t)0, wg::Add{});
    if (lane == 63) wsum[w] = inc;   // wg::fold_waves' text: through it the kernel takes 62 VGPRs for 50
    __syncthreads();
    int64_t before = 0, total = 0;
    for (int i = 0; i < kPackScanThreads / 64; ++i) {
        const int64_t v = wsum[i];
        before += i < w ? v : 0;
        total += v;
    }
    int64_t off = before + inc - x;
#pragma unroll
    for (int j = 0; j < kPackPer; ++j) {
        const int c = t * kPackPer + j;
        if (c < a.C) a.offsets[c] = off;
        off += m[j];
    }
    if (t == 0) {
        a.offsets[a.C] = total;
        a.total[0] = total;
        a.total[1] = total < a.cap_out ? total : a.cap_out;
    }
}

// The wave's (channel, first slot of its tile), or false past the last tile of the last channel.
__device__ __forceinline__ bool pk_tile(int32_t C, int32_t K, int32_t& c, int32_t& start) {
    const int32_t tiles = (K + kPackTile - 1) / kPackTile;   // <= 256, and C tiles <= 2^20
    const int32_t work = (int32_t)blockIdx.x * (kPackThreads / 64) + (int32_t)(threadIdx.x >> 6);
    if (work >= C * tiles) return false;
    c = work / tiles;
    start = (work - c * tiles) * kPackTile;
    return true;
}

__global__ __launch_bounds__(kPackThreads) void k_pk_copy(PackArgs a) {
    int32_t c, start;
    if (!pk_tile(a.C, a.K, c, start)) return;
    const int64_t m = obs::row_fill(a.image[a.row0 + c], a.K);
    if (start >= m) return;
    const int64_t src = (a.row0 + c) * a.K, dst = a.offsets[c];
    const int64_t end = start + kPackTile < m ? start + kPackTile : m;
    for (int64_t i = start + (threadIdx.x & 63); i < end && dst + i < a.cap_out; i += 64) {
        a.out_words[dst + i] = a.words[src + i];
        if (a.out_stamps) a.out_stamps[dst + i] = a.stamps[src + i];
        obs::copy_bits(a.out_height + dst + i, a.row_height + src + i);
        if (a.out_dt) obs::copy_bits(a.out_dt + dst + i, a.row_dt + src + i);
    }
}

hipError_t launch_pack_second(const PackArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(kPackScanThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.cap_out == 0) return e;
    const int32_t work = a.C * ((a.K + kPackTile - 1) / kPackTile), per = kPackThreads / 64;
    hipLaunchKernelGGL(k_pk_copy, dim3((unsigned)((work + per - 1) / per)), dim3(kPackThreads), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(kPackThreads) void k_pk_nan(ClearArgs a) {
    int32_t c, start;
    if (!pk_tile(a.C, a.K, c, start)) return;
    const int64_t m = obs::row_fill(a.image[a.row0 + c], a.K);
    if (start >= m) return;
    const int64_t at = (a.row0 + c) * a.K;
    const int64_t end = start + kPackTile < m ? start + kPackTile : m;
    const float nan = __uint_as_float(obs::kNanBits);
    for (int64_t i = start + (threadIdx.x & 63); i < end; i += 64) {
        obs::copy_bits(a.row_height + at + i, &nan);
        if (a.row_dt) obs::copy_bits(a.row_dt + at + i, &nan);
    }
}

__global__ __launch_bounds__(kPackThreads) void k_pk_zero(int32_t* image, int64_t row0, int32_t C) {
    const int32_t c = (int32_t)(blockIdx.x * kPackThreads + threadIdx.x);
    if (c < C) image[row0 + c] = 0;
}

hipError_t launch_clear_second(const ClearArgs& a, hipStream_t s) {
    const int32_t work = a.C * ((a.K + kPackTile - 1) / kPackTile), per = kPackThreads / 64;
    hipLaunchKernelGGL(k_pk_nan, dim3((unsigned)((work + per - 1) / per)), dim3(kPackThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pk_zero, dim3((unsigned)((a.C + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, s,
                       a.image, a.row0, a.C);
    return hipGetLastError();
}

}  // namespace mkid
