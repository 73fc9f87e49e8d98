// Resonator loop fits (include/mkidgpu.h mkid_fit_loops; the rules are loopfit_common.h, the solver and the
// workgroup's driver lm_common.h).
//
// k_loopfit  one workgroup of 256 threads per channel.
//   Window:  thread t computes velocities t, t + 256, .. into LDS, then the smoothed velocities from
//            them (ten terms each); thread 0 scans for the first maximum and publishes cidx, low,
//            high, n. The window's x, I, Q, wI, wQ (n <= 512 points, 20 KiB) are staged in LDS once
//            and every model evaluation reads them from there; thread 0 makes the guesses and bounds.
//   Starts:  wave w takes starts w, w + 4, .. one at a time. In an evaluation lane l takes points l,
//            l + 64, .. and keeps the 55 + 10 + 1 float64 partial sums in registers (a 256-thread
//            group leaves a lane 512 registers; a 1024-thread group would leave 128, fewer than the
//            132 the sums alone take); the lanes combine by __shfl_xor, m = 32 .. 1, so that every
//            lane ends with the same bits. Lane 0 runs the 10 x 10 Cholesky and hands the trial and
//            the verdict to the wave by __shfl, which keeps the iteration wave-uniform.
//   Result:  lane 0 of each wave keeps its best start and writes it to LDS; after a barrier thread 0
//            takes the lowest chi^2 (ties to the lower start) and writes the channel's result. No
//            atomics.
#include <hip/hip_runtime.h>

#include "loopfit_common.h"
#include "mkid_internal.h"

namespace mkid {

constexpr int kLfitThreads = 256;
constexpr int kLfitWaves = kLfitThreads / 64;

__global__ __launch_bounds__(kLfitThreads) void k_loopfit(LoopfitArgs a) {
    __shared__ double s_vel[lfit::kMaxSteps], s_sv[lfit::kMaxSteps];
    __shared__ double s_x[lfit::kMaxWindow], s_i[lfit::kMaxWindow], s_q[lfit::kMaxWindow], s_wi[lfit::kMaxWindow],
        s_wq[lfit::kMaxWindow];
    __shared__ lfit::Window s_win;
    __shared__ lfit::Problem s_pr;
    __shared__ lfit::StartResult s_best[kLfitWaves];
    __shared__ int32_t s_best_s[kLfitWaves];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t ch = blockIdx.x;
    const int32_t fsteps = a.fsteps, S = a.S;
    const int64_t o = ch * fsteps;
    const double *gI = a.i + o, *gQ = a.q + o;
    const lfit::Window w0 = lfit::window_group(gI, gQ, fsteps, a.wn, t, kLfitThreads, s_vel, s_sv);
    if (t == 0) s_win = w0;
    __syncthreads();
    const lfit::Window w = s_win;
    for (int32_t i = t; i < w.n; i += kLfitThreads) {
        s_x[i] = a.freq[o + w.low + i], s_i[i] = gI[w.low + i], s_q[i] = gQ[w.low + i];
        s_wi[i] = a.isd ? lm::div(1.0, a.isd[o + w.low + i]) : 1.0;
        s_wq[i] = a.qsd ? lm::div(1.0, a.qsd[o + w.low + i]) : 1.0;
    }
    __syncthreads();
    if (t == 0) lfit::guesses(s_x, s_i, s_q, s_wi, s_wq, w.n, w.cidx - w.low, &s_pr);
    __syncthreads();
    const int32_t status = s_pr.status;   // workgroup-uniform
    if (status != 0) {
        lm::no_fit(a.chisq_all, ch * S, S, t, kLfitThreads);
        if (t == 0) lfit::finish(w, status, nullptr, -1, &a.fits[ch]);
        return;
    }
    const bool have_q = a.qguess != nullptr;
    const double qg = have_q ? a.qguess[ch] : 0.0;
    lfit::StartResult r{};
    double best_chi = 0.0;   // the wave's best start itself waits in LDS, written by lane 0
    int32_t best_s = -1;
    // the partial holds pointers, as written: naming the arrays in it changes the register allocation
    const double *x = s_x, *yI = s_i, *yQ = s_q, *wI = s_wi, *wQ = s_wq;
    const int32_t n = w.n;
    const auto part = [=](const double* p, lfit::Sums* s) { lfit::lane_partial(p, x, yI, yQ, wI, wQ, n, lane, s); };
    const lm::WaveEval<lfit::kNP, decltype(part)> ev{part};
    const lm::WaveSolve<lfit::kNP> sol{s_pr.lo, s_pr.hi, lane};
    for (int32_t s = wv; s < S; s += kLfitWaves) {   // wave-uniform; written here and in k_magfit (lm_common.h)
        lfit::make_start(s_pr, s, a.draws + (ch * S + s) * 5, have_q, qg, r.p);
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
        const int32_t pick = lm::pick_wave(s_best, s_best_s, kLfitWaves);
        lfit::finish(w, 0, pick < 0 ? nullptr : &s_best[pick], pick < 0 ? -1 : s_best_s[pick], &a.fits[ch]);
    }
}

hipError_t launch_fit_loops(const LoopfitArgs& a, int32_t nch, hipStream_t s) {
    if (nch < 1 || a.fsteps < lfit::kMinSteps || a.fsteps > lfit::kMaxSteps || a.S < 1 || a.S > lfit::kMaxStarts)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_loopfit, dim3((unsigned)nch), dim3(kLfitThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mkid
