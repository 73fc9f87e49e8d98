// The solver of the resonator fits, one definition for every model fitted with it (the loop fit of
// loopfit_common.h at N = 10 parameters, the magnitude fit of magfit_common.h at N = 6), for the
// kernels and for the host twins: the one-operation helpers, the sums A = J^T J, g = J^T r and
// chi^2 with the butterfly over 64 lane partials, the damped normal equations with their Cholesky,
// the accept and stop rules of one start, "the lowest chi^2 of S starts wins", and the two drivers
// that run them: the host loops (no HIP, so that the CPU sanitizer build of tools/plan_fuzz.cpp
// runs them) and, under __HIPCC__, the wave's and the workgroup's share of the same work. A model
// brings its data, its bounds, make_start(s, p), a lane partial of the sums and its finish.
//
// Levenberg-Marquardt on analytic normal equations, Marquardt's diagonal scaling, projected onto
// the bounds: this repository's definition, include/mkidgpu.h mkid_fit_loops states it in full.
//
// Every float operation is rounded once and never fused with its neighbour (the helpers switch
// contraction off for their own statement, as wavecal_common.h's), and every sum has a written
// order, so that device, host twin and a float64 restatement differ only through the library
// functions a model calls.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LM_HD __host__ __device__ inline
#else
#define LM_HD inline
#endif
#if defined(__clang__)
#define LM_NO_FMA _Pragma("clang fp contract(off)")
#define LM_UNROLL _Pragma("unroll")
#else
#define LM_NO_FMA
#define LM_UNROLL
#endif

namespace mkid {
namespace lm {

constexpr int32_t kLanes = 64;
constexpr int32_t kMaxStarts = 16;
constexpr double kLam0 = 1e-3, kLamMin = 1e-12, kLamMax = 1e12;

// one IEEE operation each
LM_HD double add(double a, double b) { LM_NO_FMA return a + b; }
LM_HD double sub(double a, double b) { LM_NO_FMA return a - b; }
LM_HD double mul(double a, double b) { LM_NO_FMA return a * b; }
LM_HD double div(double a, double b) { LM_NO_FMA return a / b; }
LM_HD double nan64() { return __builtin_nan(""); }
LM_HD bool fin(double v) { return __builtin_isfinite(v); }
LM_HD double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the sums ---------------------------------------------------------------------------------------
// The sums of a fit with N parameters: the lower triangle of A = J^T J, entry (i, j <= i) at
// i (i + 1) / 2 + j, g = J^T r and chi^2.
template <int32_t N>
struct SumsT {
    double A[N * (N + 1) / 2], g[N], chi;
};
template <int32_t N>
LM_HD void zero(SumsT<N>* s) {
    LM_UNROLL
    for (int32_t i = 0; i < N * (N + 1) / 2; ++i) s->A[i] = 0.0;
    LM_UNROLL
    for (int32_t i = 0; i < N; ++i) s->g[i] = 0.0;
    s->chi = 0.0;
}

// one residual r with its row J of the Jacobian into the sums: chi, then g_i and A_ij (j <= i) by
// ascending i, j
template <int32_t N>
LM_HD void accumulate(SumsT<N>* s, const double* J, double r) {
    s->chi = add(s->chi, mul(r, r));
    LM_UNROLL
    for (int32_t i = 0; i < N; ++i) {
        s->g[i] = add(s->g[i], mul(J[i], r));
        LM_UNROLL
        for (int32_t j = 0; j <= i; ++j) s->A[i * (i + 1) / 2 + j] = add(s->A[i * (i + 1) / 2 + j], mul(J[i], J[j]));
    }
}

// ---- the step -------------------------------------------------------------------------------------
// trial = clip(p + delta), (A + lam diag D) delta = g on the free set (hi > lo and D = A_ii > 0). A
// parameter outside the free set has its row and column replaced by the identity's and g = 0, so
// that its delta is exactly 0 and the others are those of the reduced system. Cholesky, column by
// column, every inner sum by ascending k. false: a pivot that is not positive and finite. N: the
// number of parameters (p, lo, hi, trial [N]).
template <int32_t N>
LM_HD bool step(const SumsT<N>& c, double lam, const double* p, const double* lo, const double* hi, double* trial,
                int32_t* nfree) {
    double L[N * (N + 1) / 2], y[N];
    bool fr[N];
    int32_t nf = 0;
    LM_UNROLL
    for (int32_t i = 0; i < N; ++i) {
        fr[i] = hi[i] > lo[i] && c.A[i * (i + 1) / 2 + i] > 0.0;
        nf += fr[i] ? 1 : 0;
    }
    *nfree = nf;
    LM_UNROLL
    for (int32_t j = 0; j < N; ++j) {
        const double ajj = c.A[j * (j + 1) / 2 + j];
        double s = fr[j] ? add(ajj, mul(lam, ajj)) : 1.0;
        LM_UNROLL
        for (int32_t k = 0; k < j; ++k) s = sub(s, mul(L[j * (j + 1) / 2 + k], L[j * (j + 1) / 2 + k]));
        if (!(s > 0.0 && fin(s))) return false;
        const double d = sqrt(s);
        L[j * (j + 1) / 2 + j] = d;
        LM_UNROLL
        for (int32_t i = j + 1; i < N; ++i) {
            double t = fr[i] && fr[j] ? c.A[i * (i + 1) / 2 + j] : 0.0;
            LM_UNROLL
            for (int32_t k = 0; k < j; ++k) t = sub(t, mul(L[i * (i + 1) / 2 + k], L[j * (j + 1) / 2 + k]));
            L[i * (i + 1) / 2 + j] = div(t, d);
        }
    }
    LM_UNROLL
    for (int32_t i = 0; i < N; ++i) {   // L y = g
        double t = fr[i] ? c.g[i] : 0.0;
        LM_UNROLL
        for (int32_t k = 0; k < i; ++k) t = sub(t, mul(L[i * (i + 1) / 2 + k], y[k]));
        y[i] = div(t, L[i * (i + 1) / 2 + i]);
    }
    LM_UNROLL
    for (int32_t i = N - 1; i >= 0; --i) {   // L^T delta = y, delta kept in y
        double t = y[i];
        LM_UNROLL
        for (int32_t k = i + 1; k < N; ++k) t = sub(t, mul(L[k * (k + 1) / 2 + i], y[k]));
        y[i] = div(t, L[i * (i + 1) / 2 + i]);
    }
    LM_UNROLL
    for (int32_t i = 0; i < N; ++i) trial[i] = clip(add(p[i], y[i]), lo[i], hi[i]);
    return true;
}

// ---- one start --------------------------------------------------------------------------------------
template <int32_t N>
struct StartResultT {
    double p[N], chi;
    int32_t evals, hit_max;
};

// eval(p, &sums): the combined sums at p. solve(sums, lam, p, trial, &nfree): step() (the device has
// one lane run it and hands the result to the wave). r->p holds the start on entry.
template <int32_t N, class Eval, class Solve>
LM_HD void run_start(int32_t max_iter, double ftol, Eval&& eval, Solve&& solve, StartResultT<N>* r) {
    SumsT<N> cur, nxt;
    eval(r->p, &cur);
    r->chi = cur.chi, r->evals = 1, r->hit_max = 0;
    if (!fin(cur.chi)) return;
    double lam = kLam0;
    for (;;) {
        if (r->evals >= max_iter) {
            r->hit_max = 1;
            return;
        }
        double trial[N];
        int32_t nfree = 0;
        if (!solve(cur, lam, r->p, trial, &nfree)) {
            lam = mul(lam, 10.0);
            if (lam > kLamMax) return;
            continue;
        }
        if (nfree == 0) return;
        eval(trial, &nxt);
        r->evals += 1;
        if (fin(nxt.chi) && nxt.chi < r->chi) {
            const double rel = div(sub(r->chi, nxt.chi), r->chi);
            LM_UNROLL
            for (int32_t i = 0; i < N; ++i) r->p[i] = trial[i];
            r->chi = nxt.chi;
            cur = nxt;
            const double l = div(lam, 10.0);
            lam = l > kLamMin ? l : kLamMin;
            if (rel <= ftol) return;
        } else {
            lam = mul(lam, 10.0);
            if (lam > kLamMax) return;
        }
    }
}

// a start beats the best so far: a finite chi^2 that is lower, or equal from a lower start
LM_HD bool better(double chi, int32_t s, double best_chi, int32_t best_s) {
    if (!fin(chi)) return false;
    return best_s < 0 || chi < best_chi || (chi == best_chi && s < best_s);
}

// ---- the host driver --------------------------------------------------------------------------------
// the butterfly over the 64 lane partials: p[l] = p[l] + p[l ^ m] on every lane at once, m = 32 .. 1
template <int32_t N>
inline void butterfly_host(SumsT<N>* part) {
    for (int32_t m = kLanes / 2; m >= 1; m >>= 1) {
        for (int32_t l = 0; l < kLanes; ++l) {
            if (l & m) continue;
            SumsT<N>& a = part[l];
            SumsT<N>& b = part[l ^ m];
            for (int32_t i = 0; i < N * (N + 1) / 2; ++i) a.A[i] = b.A[i] = add(a.A[i], b.A[i]);
            for (int32_t i = 0; i < N; ++i) a.g[i] = b.g[i] = add(a.g[i], b.g[i]);
            a.chi = b.chi = add(a.chi, b.chi);
        }
    }
}

// The combined sums as the wave makes them: partial(p, lane, &sums) for the 64 lanes, the
// butterfly, lane 0's copy.
template <int32_t N, class Partial>
struct HostEval {
    Partial partial;
    void operator()(const double* p, SumsT<N>* out) const {
        SumsT<N> part[kLanes];
        for (int32_t l = 0; l < kLanes; ++l) partial(p, l, &part[l]);
        butterfly_host(part);
        *out = part[0];
    }
};
template <int32_t N, class Partial>
inline HostEval<N, Partial> host_eval(Partial partial) {
    return {partial};
}

// The S starts of one channel, make_start(s, p) writing start s: every start's chi^2 into chisq_all
// (when given), the winner into *best -> its start, -1 when no start ends with a finite chi^2. With
// a status other than 0 nothing is fitted and chisq_all is NaN.
template <int32_t N, class MakeStart, class Eval>
inline int32_t run_starts_host(int32_t status, int32_t S, int32_t max_iter, double ftol, MakeStart&& make_start,
                               Eval&& eval, const double* lo, const double* hi, StartResultT<N>* best,
                               double* chisq_all) {
    StartResultT<N> r{};
    int32_t best_s = -1;
    for (int32_t s = 0; s < S; ++s) {
        if (status != 0) {
            if (chisq_all) chisq_all[s] = nan64();
            continue;
        }
        make_start(s, r.p);
        run_start(
            max_iter, ftol, eval,
            [&](const SumsT<N>& c, double lam, const double* p, double* trial, int32_t* nfree) {
                return step(c, lam, p, lo, hi, trial, nfree);
            },
            &r);
        if (chisq_all) chisq_all[s] = r.chi;
        if (better(r.chi, s, best->chi, best_s)) *best = r, best_s = s;
    }
    return best_s;
}

// ---- the device driver ------------------------------------------------------------------------------
// One workgroup of W waves per channel, thread t = 64 wv + lane; wave wv takes starts wv, wv + W, ..
// one at a time. That loop (make_start, run_start with the two functors below, chisq_all, the
// wave's best start kept in LDS by lane 0) stays written in each kernel: behind a function of this
// header both kernels, which sit at the register ceiling, come out of the register allocator
// differently, and k_loopfit 0.6 % slower (profiles/lmsolver/).
#if defined(__HIPCC__)
// The combined sums of a wave: partial(p, &sums) is the lane's share, then the butterfly: the lanes
// combine by __shfl_xor, m = 32 .. 1, and every lane ends with the same bits. It is the contract of
// wg_common.h's wave_reduce, written out here: through it k_loopfit's instruction stream changes.
template <int32_t N, class Partial>
struct WaveEval {
    Partial partial;
    __device__ void operator()(const double* p, SumsT<N>* s) const {
        partial(p, s);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
            for (int i = 0; i < N * (N + 1) / 2; ++i) s->A[i] = add(s->A[i], __shfl_xor(s->A[i], m, 64));
#pragma unroll
            for (int i = 0; i < N; ++i) s->g[i] = add(s->g[i], __shfl_xor(s->g[i], m, 64));
            s->chi = add(s->chi, __shfl_xor(s->chi, m, 64));
        }
    }
};

// lane 0 runs step() and hands the trial and the verdict to the wave by __shfl, which keeps the
// iteration wave-uniform
template <int32_t N>
struct WaveSolve {
    const double *lo, *hi;
    int32_t lane;
    __device__ bool operator()(const SumsT<N>& c, double lam, const double* p, double* trial, int32_t* nfree) const {
        int ok = 0, nf = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) trial[i] = 0.0;
        if (lane == 0) ok = step(c, lam, p, lo, hi, trial, &nf) ? 1 : 0;
        ok = __shfl(ok, 0, 64), nf = __shfl(nf, 0, 64);
#pragma unroll
        for (int i = 0; i < N; ++i) trial[i] = __shfl(trial[i], 0, 64);
        *nfree = nf;
        return ok != 0;
    }
};

// a channel that is not fitted (status != 0): chisq_all (the call's array or null; row: the channel's
// first index in it) is NaN, by the T threads of the group
__device__ __forceinline__ void no_fit(double* chisq_all, int64_t row, int32_t S, int32_t t, int32_t T) {
    if (chisq_all)
        for (int32_t s = t; s < S; s += T) chisq_all[row + s] = nan64();
}

// s_best[wv], s_best_s[wv]: wave wv's best start and its index (-1: none), written by its lane 0.
// After a barrier, one thread: the wave whose best start wins (the lowest chi^2, ties to the lower
// start), -1 when no wave has one
template <int32_t N>
__device__ __forceinline__ int32_t pick_wave(const StartResultT<N>* s_best, const int32_t* s_best_s, int32_t W) {
    int32_t pick = -1;
    for (int i = 0; i < W; ++i)
        if (s_best_s[i] >= 0 &&
            better(s_best[i].chi, s_best_s[i], pick < 0 ? 0.0 : s_best[pick].chi, pick < 0 ? -1 : s_best_s[pick]))
            pick = i;
    return pick;
}
#endif

}  // namespace lm
}  // namespace mkid
