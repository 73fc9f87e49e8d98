// The observing products after the heights (include/mkidgpu.h mkid_count_photons,
// mkid_height_spectra, mkid_concat_packets; the rules are obs_common.h).
//
// k_obs_count    image[sec][ch] and the two `outside` counters. The device's lists are channel-major
//                and time-ascending in a channel, so the packets of one cell are one contiguous run:
//                thread i decodes packet i and both neighbours; the first packet of a run adds -i to
//                the cell and the last adds i + 1 (one atomic of +1 where they are the same packet),
//                two integer atomics per run instead of one per packet. Sums are modulo 2^32 / 2^64,
//                so the order of the two adds does not matter, and any other list order only makes
//                the runs shorter. The neighbour past the last valid packet (a device-side count
//                below the capacity) is "none".
// k_obs_spectra  workgroup b takes packets [b slice, (b + 1) slice). With lds_rows > 0 it bins into
//                an LDS table of lds_rows channel rows of nbins + 3 counters, keyed by ch - ch_first
//                (ch_first: the channel of the slice's first packet), and adds the non-zero counters
//                to the spectra with global atomics; packets of other channels, and every packet when
//                lds_rows = 0 (the plain form, which is the shipped one: a launch option, the rule
//                is the same code; DESIGN.md §5.11 has the A/B), go to global atomics directly. It
//                also counts the slice's deferred packets.
// k_obs_scan     one workgroup: exclusive scan of the per-workgroup deferred counts on top of
//                ndef[1], then ndef = {+ qualified, min(+ written, cap_def)}.
// k_obs_scatter  workgroup b walks its slice again in list order, tile by tile, and writes its
//                deferred packets from its offset on: the list keeps the order of the input, with no
//                host step. Workgroups without deferred packets leave at once.
// k_obs_concat   out = a[0 .. min(*na, cap_a)) then b[0 .. min(*nb, cap_b)), cut at cap_out.
// Integer adds commute: image and spectra are the same bits from run to run.
#include "mkid_internal.h"
#include "obs_common.h"
#include "wg_common.h"

namespace mkid {

constexpr int kObsThreads = 256;

__global__ __launch_bounds__(kObsThreads) void k_obs_count(ObsCountArgs a) {
    const int64_t n = pkt::count(a.d_n, a.n);
    const int64_t stride = (int64_t)gridDim.x * kObsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kObsThreads + threadIdx.x; i < n; i += stride) {
        const int64_t k = obs::cell(pkt::decode(a.events[i], a.j0), a.C, a.N, a.fs, a.n_seconds);
        const bool first = i == 0 || obs::cell(pkt::decode(a.events[i - 1], a.j0), a.C, a.N, a.fs, a.n_seconds) != k;
        const bool last = i == n - 1 || obs::cell(pkt::decode(a.events[i + 1], a.j0), a.C, a.N, a.fs, a.n_seconds) != k;
        if (!first && !last) continue;
        const uint64_t d = pkt::run_delta(i, first, last);
        if (k >= 0)
            atomicAdd(reinterpret_cast<unsigned int*>(a.image) + k, (unsigned int)d);
        else
            atomicAdd(reinterpret_cast<unsigned long long*>(a.outside) + (k == obs::kNonPixel ? 0 : 1),
                      (unsigned long long)d);
    }
}

hipError_t launch_count_photons(const ObsCountArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int64_t blocks = pkt::grid_stride_blocks(a.n, kObsThreads, a.ncu, 8);
    hipLaunchKernelGGL(k_obs_count, dim3((unsigned)blocks), dim3(kObsThreads), 0, s, a);
    return hipGetLastError();
}

// ---- spectra and the deferred list -----------------------------------------------------------
ObsPlan plan_spectra(int64_t n, int32_t nbins, bool lds) {
    ObsPlan p{};
    p.cut = pkt::slices(n, kObsThreads);
    const int64_t row_bytes = (int64_t)(nbins + obs::kExtraCols) * 4;
    const int64_t fit = kObsLdsBytes / row_bytes;
    p.lds_rows = lds ? (int32_t)(fit < kObsMaxRows ? fit : kObsMaxRows) : 0;
    p.lds_bytes = (int32_t)(p.lds_rows * row_bytes);
    return p;
}

__global__ __launch_bounds__(kObsThreads) void k_obs_spectra(ObsSpectraArgs a) {
    extern __shared__ unsigned int obs_tab[];
    __shared__ int s_ndef;
    const int64_t n = pkt::count(a.d_n, a.n);
    int64_t b0, b1;
    pkt::bounds(blockIdx.x, a.slice, n, b0, b1);
    const int32_t cols = a.nbins + obs::kExtraCols;
    const int32_t tab_n = a.lds_rows * cols;
    if (threadIdx.x == 0) s_ndef = 0;
    for (int32_t i = threadIdx.x; i < tab_n; i += kObsThreads) obs_tab[i] = 0;
    __syncthreads();
    if (b0 < b1) {
        const int32_t ch_first = pkt::decode(a.events[b0], a.j0).ch;
        int mine = 0;
        for (int64_t i = b0 + threadIdx.x; i < b1; i += kObsThreads) {
            const pkt::Stamp st = pkt::decode(a.events[i], a.j0);
            if (st.ch >= a.C) continue;
            const float h = a.heights[i];
            if (a.deferred && obs::deferred(h, st.jg, a.j_defer)) {
                ++mine;
                continue;
            }
            const int32_t col = obs::column(h, a.lo[st.ch], a.inv[st.ch], a.nbins);
            const int32_t row = st.ch - ch_first;
            if (row >= 0 && row < a.lds_rows)
                atomicAdd(&obs_tab[row * cols + col], 1u);
            else
                atomicAdd(reinterpret_cast<unsigned int*>(a.spectra) + (int64_t)st.ch * cols + col, 1u);
        }
        if (mine) atomicAdd(&s_ndef, mine);
        __syncthreads();
        // rows past channel C - 1 stay zero: no packet maps to them
        for (int32_t i = threadIdx.x; i < tab_n; i += kObsThreads) {
            const unsigned int v = obs_tab[i];
            if (v) atomicAdd(reinterpret_cast<unsigned int*>(a.spectra) + (int64_t)ch_first * cols + i, v);
        }
    } else {
        __syncthreads();
    }
    if (a.deferred && threadIdx.x == 0) a.wg_count[blockIdx.x] = s_ndef;
}

__global__ __launch_bounds__(kObsMaxBlocks) void k_obs_scan(const int32_t* wg_count, int32_t blocks, int64_t* wg_off,
                                                            int64_t cap_def, int64_t* ndef) {
    __shared__ int64_t wsum[kObsMaxBlocks / 64];
    const int t = threadIdx.x;
    const int64_t x = t < blocks ? wg_count[t] : 0;
    int64_t before, total;
    const int64_t inc = wg::wave_scan(x, (int64_t)0, wg::Add{});
    wg::fold_waves((t & 63) == 63, inc, wsum, kObsMaxBlocks / 64, (int64_t)0, wg::Add{}, before, total);
    const int64_t base = ndef[1];
    __syncthreads();   // every thread has read ndef[1] before thread 0 replaces it
    if (t < blocks) wg_off[t] = base + before + inc - x;
    if (t == 0) {
        ndef[0] += total;
        const int64_t end = base + total;
        ndef[1] = end < cap_def ? end : (base > cap_def ? base : cap_def);
    }
}

__global__ __launch_bounds__(kObsThreads) void k_obs_scatter(ObsSpectraArgs a) {
    __shared__ int wtot[kObsThreads / 64];
    if (a.wg_count[blockIdx.x] == 0) return;   // workgroup-uniform
    const int64_t n = pkt::count(a.d_n, a.n);
    int64_t b0, b1;
    pkt::bounds(blockIdx.x, a.slice, n, b0, b1);
    int64_t o = a.wg_off[blockIdx.x];
    for (int64_t t0 = b0; t0 < b1; t0 += kObsThreads) {   // workgroup-uniform trip count
        const int64_t i = t0 + threadIdx.x;
        bool q = false;
        uint64_t word = 0;
        if (i < b1) {
            word = a.events[i];
            const pkt::Stamp st = pkt::decode(word, a.j0);
            q = st.ch < a.C && obs::deferred(a.heights[i], st.jg, a.j_defer);
        }
        const wg::Rank r = wg::wave_rank(q);   // then the rank in the workgroup: the waves' counts folded
        int before, total;
        wg::fold_waves((threadIdx.x & 63) == 0, r.count, wtot, kObsThreads / 64, 0, wg::Add{}, before,
                       total);
        const int64_t pos = o + before + r.below;
        if (q && pos >= 0 && pos < a.cap_def) a.deferred[pos] = word;
        o += total;
        __syncthreads();   // wtot is rewritten by the next tile
    }
}

hipError_t launch_height_spectra(const ObsSpectraArgs& a0, const ObsPlan& p, hipStream_t s) {
    if (a0.n <= 0) return hipSuccess;
    ObsSpectraArgs a = a0;
    a.slice = p.cut.slice, a.lds_rows = p.lds_rows;
    hipLaunchKernelGGL(k_obs_spectra, dim3((unsigned)p.cut.blocks), dim3(kObsThreads), (size_t)p.lds_bytes, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.deferred) return e;
    hipLaunchKernelGGL(k_obs_scan, dim3(1), dim3(kObsMaxBlocks), 0, s, a.wg_count, p.cut.blocks, a.wg_off, a.cap_def, a.ndef);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_obs_scatter, dim3((unsigned)p.cut.blocks), dim3(kObsThreads), 0, s, a);
    return hipGetLastError();
}

// ---- joining two counted lists ------------------------------------------------------------------
__global__ __launch_bounds__(kObsThreads) void k_obs_concat(const uint64_t* a, const int64_t* d_na, int64_t cap_a,
                                                            const uint64_t* b, const int64_t* d_nb, int64_t cap_b,
                                                            uint64_t* out, int64_t cap_out, int64_t* nout) {
    const int64_t na = pkt::count(d_na, cap_a), nb = pkt::count(d_nb, cap_b);
    const int64_t tot = na + nb, nw = tot < cap_out ? tot : cap_out;
    const int64_t stride = (int64_t)gridDim.x * kObsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kObsThreads + threadIdx.x; i < nw; i += stride)
        out[i] = i < na ? a[i] : b[i - na];
    if (blockIdx.x == 0 && threadIdx.x == 0) nout[0] = tot, nout[1] = nw;
}

hipError_t launch_concat_packets(const uint64_t* a, const int64_t* d_na, int64_t cap_a, const uint64_t* b,
                                 const int64_t* d_nb, int64_t cap_b, uint64_t* out, int64_t cap_out, int64_t* nout,
                                 int32_t ncu, hipStream_t s) {
    const int64_t most = cap_a + cap_b < cap_out ? cap_a + cap_b : cap_out;
    const int64_t need = pkt::grid_stride_blocks(most, kObsThreads, ncu, 8);
    const int64_t blocks = need < 1 ? 1 : need;   // the counts are written even where nothing is copied
    hipLaunchKernelGGL(k_obs_concat, dim3((unsigned)blocks), dim3(kObsThreads), 0, s, a, d_na, cap_a, b, d_nb, cap_b, out,
                       cap_out, nout);
    return hipGetLastError();
}

}  // namespace mkid
