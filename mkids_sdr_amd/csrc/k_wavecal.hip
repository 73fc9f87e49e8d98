// Energy calibration from laser spectra and the energy cube (include/mkidgpu.h mkid_spectrum_lines,
// mkid_energy_cube; the rules are wavecal_common.h).
//
// k_wcal_lines  one workgroup of 256 threads per channel. The channel's nbins counts are staged in
//               dynamic LDS (4 nbins bytes, 64 KiB at the most; above 64 KiB less the static tables
//               the launch needs the dynamic-LDS attribute). Lane map: thread t owns bins t, t + 256,
//               ..: a wave's 64 lanes read 64 consecutive words of the row at every step of the
//               smoothing sum (ds_read_b32, conflict-free), and s is recomputed from the row each
//               time: an int64 table of s beside the row would be 192 KiB, more than a CU has.
//               Selection: P rounds; in a round every thread takes the largest key (s 2^15 + 32767 -
//               b, wavecal_common.h candidate_key) of its candidates that no chosen line excludes, and
//               wg::reduce gives every thread their maximum, so the round's end is workgroup-uniform;
//               no atomics. Thread p < found then fits line p (one lane per line: float64 sums by ascending bin),
//               thread 0 makes the calibration from the fits in LDS, threads p < P store the lines.
// k_wcal_cube   grid-stride over the packets as k_obs_count: thread i computes the cell of packet i
//               and of both neighbours; the first packet of a run of equal cells adds -i and the
//               last i + 1 (one atomic of +1 where they are the same packet). A packet that touches
//               no cell (ch >= C, deferred) ends a run and adds nothing. Sums are modulo 2^32, so
//               any list order gives the same cube.
#include <hip/hip_runtime.h>

#include <atomic>

#include "mkid_internal.h"
#include "wavecal_common.h"
#include "wg_common.h"

namespace mkid {

constexpr int kWcalThreads = 256;
constexpr int kWcalWaves = kWcalThreads / 64;

__global__ __launch_bounds__(kWcalThreads) void k_wcal_lines(WcalLinesArgs a) {
    extern __shared__ int32_t wcal_row[];
    __shared__ unsigned long long wmax[kWcalWaves];   // the type the shuffles take
    __shared__ mkid_line_fit s_fit[wcal::kMaxLines];
    const int t = threadIdx.x;
    const int64_t ch = blockIdx.x;
    const int32_t nbins = a.nbins;
    const int32_t* src = a.spectra + ch * (nbins + obs::kExtraCols) + 1;
    for (int32_t b = t; b < nbins; b += kWcalThreads) wcal_row[b] = src[b];
    __syncthreads();
    int32_t chosen[wcal::kMaxLines] = {0, 0, 0};
    int32_t found = 0;
    for (int32_t r = 0; r < a.P; ++r) {   // workgroup-uniform trip count
        unsigned long long best = 0;
        for (int32_t b = t; b < nbins; b += kWcalThreads) {
            if (wcal::excluded(b, chosen, r, a.min_sep)) continue;
            const uint64_t k = wcal::candidate_key(wcal_row, nbins, a.w, a.min_peak, b);
            best = k > best ? k : best;
        }
        const unsigned long long top = wg::reduce(best, wmax, kWcalWaves, 0ull, wg::Max{});
        __syncthreads();   // wmax is rewritten by the next round
        if (!top) break;   // every thread holds the same maximum
        chosen[found++] = wcal::key_bin(top);
    }
    wcal::sort_bins(chosen, found);
    if (t < a.P) {
        if (t < found)
            wcal::fit_line(wcal_row, nbins, a.w, chosen[t], wcal::window(chosen, found, t, a.g, nbins), a.g, a.lo[ch],
                           a.step[ch], &s_fit[t]);
        else
            wcal::no_line(&s_fit[t]);
    }
    __syncthreads();
    if (t == 0) {
        wcal::Params pr{};
        pr.nbins = nbins, pr.P = a.P, pr.w = a.w, pr.min_sep = a.min_sep, pr.g = a.g, pr.min_peak = a.min_peak;
        for (int i = 0; i < wcal::kMaxLines; ++i) pr.E[i] = a.E[i];
        mkid_energy_cal cal;
        float cf[4];
        wcal::calibrate(pr, s_fit, found, &cal, cf);
        a.cal[ch] = cal;
        for (int i = 0; i < 4; ++i) a.cal_f[ch * 4 + i] = cf[i];
    }
    if (t < a.P) a.lines[ch * a.P + t] = s_fit[t];
}

hipError_t launch_spectrum_lines(const WcalLinesArgs& a, int32_t nch, hipStream_t s) {
    static std::atomic<uint64_t> lds_mask{0};
    const int max_lds = 4 * obs::kMaxBins;
    hipError_t e = ensure_lds_attr(lds_mask, (const void*)k_wcal_lines, max_lds);
    if (e != hipSuccess) return e;
    if (!obs::bins_ok(a.nbins) || nch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wcal_lines, dim3((unsigned)nch), dim3(kWcalThreads), (size_t)a.nbins * 4, s, a);
    return hipGetLastError();
}

// ---- the energy cube ----------------------------------------------------------------------------
__device__ __forceinline__ int64_t wcal_cell(const WcalCubeArgs& a, const wcal::CubeRule& r, int64_t i, float* e,
                                             bool* pixel) {
    return wcal::cube_cell(a.events[i], a.heights[i], a.cal_f, r, e, pixel);
}

__global__ __launch_bounds__(kWcalThreads) void k_wcal_cube(WcalCubeArgs a) {
    const int64_t n = pkt::count(a.d_n, a.n);
    const wcal::CubeRule r{a.j0, a.j_defer, a.C, a.nb, a.mode, a.hc, a.vlo, a.vinv};
    const int64_t stride = (int64_t)gridDim.x * kWcalThreads;
    for (int64_t i = (int64_t)blockIdx.x * kWcalThreads + threadIdx.x; i < n; i += stride) {
        float e = 0.f, en = 0.f;
        bool pixel = false, pn = false;
        const int64_t k = wcal_cell(a, r, i, &e, &pixel);
        if (pixel && a.energy) a.energy[i] = e;
        if (k < 0) continue;
        const bool first = i == 0 || wcal_cell(a, r, i - 1, &en, &pn) != k;
        const bool last = i == n - 1 || wcal_cell(a, r, i + 1, &en, &pn) != k;
        if (!first && !last) continue;
        atomicAdd(reinterpret_cast<unsigned int*>(a.cube) + k, (unsigned int)pkt::run_delta(i, first, last));
    }
}

hipError_t launch_energy_cube(const WcalCubeArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int64_t blocks = pkt::grid_stride_blocks(a.n, kWcalThreads, a.ncu, 8);
    hipLaunchKernelGGL(k_wcal_cube, dim3((unsigned)blocks), dim3(kWcalThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mkid
