// Resonator magnitude fits (include/mkidgpu.h mkid_fit_mags; the rules are magfit_common.h, the solver and the
// workgroup's driver lm_common.h).
//
// k_magfit  one workgroup per channel, min(S, 8) waves: one wave per start up to eight.
//   Index:   thread t computes velocities t, t + T, .. into LDS, then the smoothed velocities from
//            them; thread 0 scans for the first maximum (cidx). The two scratch rows are the rows the
//            sweep is staged in afterwards.
//   Data:    thread t takes points t, t + T, ..: x and the magnitude go to LDS (2 x 8 KiB at 1024
//            points), a value that is not finite raises a flag in LDS, and the largest magnitude is
//            wg::reduce's from 0 (magnitudes are >= 0 or NaN and a NaN never wins, so the maximum of the
//            others in any order is the serial scan's from mag[0], unless mag[0] itself is NaN, which is
//            then the result as it is there). Each thread then divides its own points by norm. Thread 0
//            makes the bounds and the start's f0.
//   Starts:  wave w takes starts w, w + W, .. one at a time. In an evaluation lane l takes points l,
//            l + 64, .. and keeps the 21 + 6 + 1 float64 partial sums in registers; the lanes combine
//            by __shfl_xor, m = 32 .. 1, so that every lane ends with the same bits. Lane 0 runs the
//            6 x 6 Cholesky and hands the trial and the verdict to the wave by __shfl, which keeps the
//            iteration wave-uniform. A start is one wave's work whatever the group's size, so the
//            result's bits do not depend on the launch shape.
//   Result:  lane 0 of each wave keeps its best start and writes it to LDS; after a barrier thread 0
//            takes the lowest chi^2 (ties to the lower start) and writes the channel's result and
//            d_qout. No atomics.
// Group size, from the compiler's register report (profiles/magfit/resource_usage.txt). The 56
// VGPRs of sums are not the whole of it: run_start holds two sets of sums, the unrolled Cholesky its
// factor, and the kernel wants about 262 registers a lane. Bounded to 256 threads it takes 256 VGPRs
// + 6 AGPRs, no scratch, one wave a SIMD (four waves a CU); bounded to 512 threads 256 VGPRs with 5
// spilled (24 B of scratch a lane) at two waves a SIMD (eight waves a CU); bounded to 1024 threads
// 128 VGPRs with 237 spilled (524 B a lane). Eight waves it is: twice the starts in flight of the
// four-wave group for five spilled registers, and ten starts in two rounds; 2048 channels x 10
// starts x 200 steps take 14.7 ms so and 19.5 ms with four-wave groups (profiles/magfit/).
#include <hip/hip_runtime.h>

#include "magfit_common.h"
#include "mkid_internal.h"
#include "wg_common.h"

namespace mkid {

#ifndef MKID_MFIT_WAVES
#define MKID_MFIT_WAVES 8   // an A/B build may take 4 or 16 (FLAGS_k_magfit=-DMKID_MFIT_WAVES=16)
#endif
constexpr int kMfitMaxWaves = MKID_MFIT_WAVES;
constexpr int kMfitMaxThreads = kMfitMaxWaves * 64;

__global__ __launch_bounds__(kMfitMaxThreads) void k_magfit(MagfitArgs a) {
    __shared__ double s_x[mfit::kMaxSteps], s_y[mfit::kMaxSteps];   // first the velocities and their smoothing
    __shared__ double s_wmax[kMfitMaxWaves];
    __shared__ int32_t s_cidx, s_bad;
    __shared__ mfit::Problem s_pr;
    __shared__ mfit::StartResult s_best[kMfitMaxWaves];
    __shared__ int32_t s_best_s[kMfitMaxWaves];
    const int t = threadIdx.x, T = blockDim.x, lane = t & 63, wv = t >> 6, W = T >> 6;
    const int64_t ch = blockIdx.x;
    const int32_t fsteps = a.fsteps, S = a.S;
    const int64_t o = ch * fsteps;
    const double *gI = a.i + o, *gQ = a.q + o;
    if (t == 0) s_bad = 0;
    const lfit::Window w0 = lfit::window_group(gI, gQ, fsteps, a.wn, t, T, s_x, s_y);
    if (t == 0) s_cidx = w0.cidx;
    __syncthreads();   // the scan is over: the rows are free
    const int32_t cidx = s_cidx;
    double mx = 0.0;
    bool bad = false;
    for (int32_t i = t; i < fsteps; i += T) {
        const double x = a.freq[o + i], I = gI[i], Q = gQ[i];
        const double mag = mfit::magnitude(I, Q);
        bad = bad || !(lm::fin(x) && lm::fin(I) && lm::fin(Q));
        s_x[i] = x, s_y[i] = mag;
        mx = mag > mx ? mag : mx;
    }
    if (bad) s_bad = 1;   // every writer stores the same value; wg::reduce has the barrier
    double norm = wg::reduce(mx, s_wmax, W, 0.0, wg::Max{});
    const double mag0 = s_y[0];
    if (mag0 != mag0) norm = mag0;
    const bool nonfinite = s_bad != 0;
    __syncthreads();   // everyone has read mag[0]
    for (int32_t i = t; i < fsteps; i += T) s_y[i] = lm::div(s_y[i], norm);
    if (t == 0) mfit::problem(s_x, fsteps, nonfinite, norm, &s_pr);
    __syncthreads();
    const int32_t status = s_pr.status;   // workgroup-uniform
    if (status != 0) {
        lm::no_fit(a.chisq_all, ch * S, S, t, T);
        if (t == 0) {
            const double qo = mfit::finish(cidx, norm, status, nullptr, -1, &a.fits[ch]);
            if (a.qout) a.qout[ch] = qo;
        }
        return;
    }
    mfit::StartResult r{};
    double best_chi = 0.0;   // the wave's best start itself waits in LDS, written by lane 0
    int32_t best_s = -1;
    const auto part = [=](const double* p, mfit::Sums* s) { mfit::lane_partial(p, s_x, s_y, fsteps, lane, s); };
    const lm::WaveEval<mfit::kNP, decltype(part)> ev{part};
    const lm::WaveSolve<mfit::kNP> sol{s_pr.lo, s_pr.hi, lane};
    for (int32_t s = wv; s < S; s += W) {   // wave-uniform; written here and in k_loopfit (lm_common.h)
        mfit::make_start(s_pr, s, a.draws[ch * S + s], r.p);
        lm::run_start(a.max_iter, a.ftol, ev, sol, &r);
        if (lane == 0 && a.chisq_all) a.chisq_all[ch * S + s] = r.chi;
        if (lm::better(r.chi, s, best_chi, best_s)) {
            best_chi = r.chi, best_s = s;
            if (lane == 0) s_best[wv] = r;
        }
    }
    if (lane == 0) s_best_s[wv] = best_s;
    __syncthreads();
    if (t == 0) {
        const int32_t pick = lm::pick_wave(s_best, s_best_s, W);
        const double qo =
            mfit::finish(cidx, norm, 0, pick < 0 ? nullptr : &s_best[pick], pick < 0 ? -1 : s_best_s[pick], &a.fits[ch]);
        if (a.qout) a.qout[ch] = qo;
    }
}

hipError_t launch_fit_mags(const MagfitArgs& a, int32_t nch, hipStream_t s) {
    if (nch < 1 || a.fsteps < mfit::kMinSteps || a.fsteps > mfit::kMaxSteps || a.S < 1 || a.S > mfit::kMaxStarts)
        return hipErrorInvalidValue;
    const int waves = a.S < kMfitMaxWaves ? a.S : kMfitMaxWaves;
    hipLaunchKernelGGL(k_magfit, dim3((unsigned)nch), dim3((unsigned)(waves * 64)), 0, s, a);
    return hipGetLastError();
}

}  // namespace mkid
