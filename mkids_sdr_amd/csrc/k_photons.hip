// The per-pixel, per-second photon rows (include/mkidgpu.h mkid_list_photons,
// mkid_fill_photon_heights; the rules are obs_common.h).
//
// A run is a maximal stretch of the list whose packets share a cell (or an `outside` counter); in
// the device's order a cell's packets of a call are one run. Packet i goes to slot
// base + (i - head) of its cell's row: head, the index of the first packet of its run, and base,
// the cell's count before the run. The list is cut into slices (pkt::slices), workgroup b taking
// slice b tile by tile, and the order between the steps comes from the kernel boundaries alone:
// k_ph_heads  a packet is a run head when its left neighbour is of another cell (k_obs_count's
//             test). head[i] = the last head at or before i inside the slice (a max-scan of
//             head ? i : -1, per wave from a ballot, across the waves and tiles through LDS), -1
//             where the run began in an earlier slice; carry[b] = the slice's last head, or -1.
// k_ph_scan   one workgroup: carry[b] = the last head of the slices before b (the exclusive
//             max-scan of the carries; the k_obs_scan pattern).
// k_ph_base   head[i] < 0 takes carry[b]. The last packet of a run adds the run's length to the
//             image (or to an `outside` counter) and publishes the old value as base[head]: one
//             integer atomic per run.
// k_ph_rows   words / stamps[cell][base[head] + i - head] where that slot is < K, else the packet
//             is counted as dropped (one atomic per workgroup that dropped any).
// k_ph_fill   mkid_fill_photon_heights: thread per packet, a binary search of its stamp in its
//             cell's row, the height (and dt) copied into the slot found; the two counters of a
//             workgroup go out as one atomic each.
// No workgroup waits for another inside a kernel, and no floating-point atomic is used.
// The cell is obs::ring_cell's over the call's window: a slot's cells are distinct inside the window,
// so a cell's packets of a call are one run, and each of the four `outside` kinds is a run of its
// own. The plain forms (mkid_list_photons, mkid_fill_photon_heights) are the whole window. There
// ring_cell is obs::cell, and the three list kernels are built a second time with it (kWhole): the
// window's compares and its 64-bit modulo, two cells per packet, cost the list call 7 to 13 % at the
// operating shape; the fill, one cell and a binary search per packet, has one build.
#include "mkid_internal.h"
#include "obs_common.h"

namespace mkid {

constexpr int kPhThreads = 256;

// The cell of a decoded packet in the call's window (PhotonArgs and PhotonFillArgs name it alike);
// kWhole: the window is obs::whole(n_slots).
template <bool kWhole, class A>
__device__ __forceinline__ int64_t ph_cell(const A& a, const pkt::Stamp& st) {
    if (kWhole) return obs::cell(st, a.C, a.N, a.fs, a.n_slots);
    return obs::ring_cell(st, a.C, a.N, a.fs, obs::Window{a.sec0, a.sec_end, a.n_slots});
}

template <bool kWhole>
__global__ __launch_bounds__(kPhThreads) void k_ph_heads(PhotonArgs a) {
    __shared__ int64_t wlast[kPhThreads / 64];
    const int64_t n = pkt::count(a.d_n, a.n);
    int64_t b0, b1;
    pkt::bounds(blockIdx.x, a.slice, n, b0, b1);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t run = -1;   // the last head of the tiles walked so far
    for (int64_t t0 = b0; t0 < b1; t0 += kPhThreads) {   // workgroup-uniform trip count
        const int64_t i = t0 + threadIdx.x;
        const bool head = i < b1 && (i == 0 || ph_cell<kWhole>(a, pkt::decode(a.events[i - 1], a.j0)) !=
                                                   ph_cell<kWhole>(a, pkt::decode(a.events[i], a.j0)));
        const uint64_t m = __ballot(head);
        const int64_t w0 = t0 + w * 64;
        if (lane == 0) wlast[w] = m ? w0 + 63 - __clzll(m) : -1;
        __syncthreads();
        int64_t before = run, total = run;   // head indices ascend with the wave, so the last set one wins
#pragma unroll
        for (int k = 0; k < kPhThreads / 64; ++k) {
            const int64_t v = wlast[k];
            if (v >= 0) {
                if (k < w) before = v;
                total = v;
            }
        }
        const uint64_t mm = m & (lane == 63 ? ~(uint64_t)0 : (((uint64_t)2 << lane) - 1));
        if (i < b1) a.head[i] = mm ? w0 + 63 - __clzll(mm) : before;
        run = total;
        __syncthreads();   // wlast is rewritten by the next tile
    }
    if (threadIdx.x == 0) a.carry[blockIdx.x] = run;
}

__global__ __launch_bounds__(kObsMaxBlocks) void k_ph_scan(int64_t* carry, int32_t blocks) {
    __shared__ int64_t wmax[kObsMaxBlocks / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t inc = t < blocks ? carry[t] : -1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(inc, off, 64);
        if (lane >= off && y > inc) inc = y;
    }
    if (lane == 63) wmax[w] = inc;
    const int64_t left = __shfl_up(inc, 1, 64);
    __syncthreads();   // every carry is read, every wave's maximum written
    int64_t ex = lane ? left : -1;
    for (int i = 0; i < w; ++i) {
        const int64_t v = wmax[i];
        if (v > ex) ex = v;
    }
    if (t < blocks) carry[t] = ex;
}

template <bool kWhole>
__global__ __launch_bounds__(kPhThreads) void k_ph_base(PhotonArgs a) {
    const int64_t n = pkt::count(a.d_n, a.n);
    int64_t b0, b1;
    pkt::bounds(blockIdx.x, a.slice, n, b0, b1);
    const int64_t carry = a.carry[blockIdx.x];
    for (int64_t i = b0 + threadIdx.x; i < b1; i += kPhThreads) {
        int64_t h = a.head[i];
        if (h < 0) a.head[i] = h = carry;   // packet 0 is a head, so a slice after the first has one before it
        const int64_t k = ph_cell<kWhole>(a, pkt::decode(a.events[i], a.j0));
        if (i != n - 1 && ph_cell<kWhole>(a, pkt::decode(a.events[i + 1], a.j0)) == k) continue;
        const uint64_t len = (uint64_t)(i + 1 - h);
        if (k >= 0)
            a.base[h] = atomicAdd(reinterpret_cast<unsigned int*>(a.image) + k, (unsigned int)len);
        else
            atomicAdd(reinterpret_cast<unsigned long long*>(a.outside) + (-1 - k), (unsigned long long)len);
    }
}

template <bool kWhole>
__global__ __launch_bounds__(kPhThreads) void k_ph_rows(PhotonArgs a) {
    __shared__ unsigned int s_drop;
    const int64_t n = pkt::count(a.d_n, a.n);
    int64_t b0, b1;
    pkt::bounds(blockIdx.x, a.slice, n, b0, b1);
    if (threadIdx.x == 0) s_drop = 0;
    __syncthreads();
    unsigned int drop = 0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += kPhThreads) {
        const uint64_t word = a.events[i];
        const pkt::Stamp st = pkt::decode(word, a.j0);
        const int64_t k = ph_cell<kWhole>(a, st);
        if (k < 0) continue;
        const int64_t h = a.head[i];
        const uint32_t slot = a.base[h] + (uint32_t)(i - h);   // modulo 2^32, as the image counts
        if (slot < (uint32_t)a.K) {
            a.words[k * a.K + slot] = obs::row_word(word, obs::microsecond(st.jg, a.N, a.fs), a.layout);
            a.stamps[k * a.K + slot] = st.jg;
        } else {
            ++drop;
        }
    }
    if (drop) atomicAdd(&s_drop, drop);
    __syncthreads();
    if (threadIdx.x == 0 && s_drop)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.dropped), (unsigned long long)s_drop);
}

template <bool kWhole>
static hipError_t launch_list(const PhotonArgs& a, const pkt::Slices& p, hipStream_t s) {
    const dim3 grid((unsigned)p.blocks), wg(kPhThreads);
    hipLaunchKernelGGL(k_ph_heads<kWhole>, grid, wg, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ph_scan, dim3(1), dim3(kObsMaxBlocks), 0, s, a.carry, p.blocks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ph_base<kWhole>, grid, wg, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ph_rows<kWhole>, grid, wg, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_list_photons(const PhotonArgs& a0, hipStream_t s) {
    if (a0.n <= 0) return hipSuccess;
    const pkt::Slices p = pkt::slices(a0.n, kPhThreads);
    PhotonArgs a = a0;
    a.slice = p.slice;
    const bool whole = a.sec0 == 0 && a.sec_end == a.n_slots;   // obs::whole: every plain call
    return whole ? launch_list<true>(a, p, s) : launch_list<false>(a, p, s);
}

// ---- heights into the rows ---------------------------------------------------------------------
__global__ __launch_bounds__(kPhThreads) void k_ph_fill(PhotonFillArgs a) {
    __shared__ unsigned int s_fill[2];
    const int64_t n = pkt::count(a.d_n, a.n);
    if (threadIdx.x < 2) s_fill[threadIdx.x] = 0;
    __syncthreads();
    unsigned int found = 0, missed = 0;
    const int64_t stride = (int64_t)gridDim.x * kPhThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPhThreads + threadIdx.x; i < n; i += stride) {
        const pkt::Stamp st = pkt::decode(a.events[i], a.j0);
        if (st.ch >= a.C || obs::deferred(a.heights[i], st.jg, a.j_defer)) continue;
        const int64_t k = ph_cell<false>(a, st);
        const int64_t at = k < 0 ? -1 : obs::find_stamp(a.stamps + k * a.K, obs::row_fill(a.image[k], a.K), st.jg);
        if (at < 0) {
            ++missed;
            continue;
        }
        obs::copy_bits(a.row_height + k * a.K + at, a.heights + i);
        if (a.dt && a.row_dt) obs::copy_bits(a.row_dt + k * a.K + at, a.dt + i);
        ++found;
    }
    if (found) atomicAdd(&s_fill[0], found);
    if (missed) atomicAdd(&s_fill[1], missed);
    __syncthreads();
    if (threadIdx.x < 2 && s_fill[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(a.fill) + threadIdx.x, (unsigned long long)s_fill[threadIdx.x]);
}

hipError_t launch_fill_photon_heights(const PhotonFillArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int64_t blocks = pkt::grid_stride_blocks(a.n, kPhThreads, a.ncu, 8);
    hipLaunchKernelGGL(k_ph_fill, dim3((unsigned)blocks), dim3(kPhThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mkid
