// Resonator loop fits (include/mkidgpu.h mkid_fit_loops states the rules), one definition for the
// kernel of k_loopfit.hip and for the host entry point mkid_fit_loops_host: the IQ-velocity window
// (the magnitude fit of magfit_common.h takes its velocity-maximum index from it), the guesses, the
// bounds, the starts, the ten-parameter loop model with its analytic Jacobian, its lane partial of
// the sums and the derived quantities. The solver and the drivers that run the starts, on the host
// and in the workgroup, are lm_common.h's at N = 10. No HIP is used but in the workgroup's window
// prologue: the host loops below are the whole of the host entry point, so that the CPU sanitizer
// build (tools/plan_fuzz.cpp) runs them.
//
// Kept from the reference's IQsweep.FitLoopMP (lib/iqsweep.py:141-291): the model RESDIFF
// (:824-858), the window about the fastest point of the loop, the guesses, the bounds, the recipe of
// the random starts, "the lowest chi^2 of S starts wins" and the derived quantities. The optimiser is
// NOT the reference's: mpfit differences the model numerically and draws its starts from an unseeded
// generator, and FitLoopMP itself raises at :231 and re-slices an already windowed array at :211.
//
// Every float operation is rounded once and never fused with its neighbour and every sum has a
// written order (lm_common.h), so that device, host twin and a float64 restatement differ only
// through sin, cos, atan2 (and log10 in dipdb).
#pragma once
#include "lm_common.h"
#include "mkidgpu.h"

namespace mkid {
namespace lfit {

using lm::add;
using lm::clip;
using lm::div;
using lm::fin;
using lm::kLanes;
using lm::kMaxStarts;
using lm::mul;
using lm::nan64;
using lm::sub;

constexpr int32_t kNP = MKID_LOOP_NPAR;   // 10 parameters
constexpr int32_t kMinSteps = 12, kMaxSteps = 1024, kMaxWindow = kMaxSteps / 2;
constexpr int32_t kWin = 10;              // hanning(10)
constexpr double kPi = 3.141592653589793;

using Sums = lm::SumsT<kNP>;
using StartResult = lm::StartResultT<kNP>;

inline bool args_ok(const double* freq, const double* i, const double* q, const double* isd, const double* qsd,
                    const double* draws, int32_t nch, int32_t fsteps, int32_t S, int32_t max_iter, double ftol,
                    const mkid_loop_fit* fits) {
    return freq && i && q && draws && fits && (isd == nullptr) == (qsd == nullptr) && nch >= 1 && fsteps >= kMinSteps &&
           fsteps <= kMaxSteps && S >= 1 && S <= kMaxStarts && max_iter >= 1 && ftol > 0.0;
}

// hanning(10) / sum by the host's cos: w[j] = 0.5 + 0.5 cos(pi (2 j - 9) / 9), the sum ascending.
inline void window_weights(double* wn) {
    double w[kWin], sum = 0.0;
    for (int32_t j = 0; j < kWin; ++j) {
        w[j] = add(0.5, mul(0.5, cos(div(mul(kPi, (double)(2 * j - 9)), 9.0))));
        sum = add(sum, w[j]);
    }
    for (int32_t j = 0; j < kWin; ++j) wn[j] = div(w[j], sum);
}

// ---- the window: +, -, x, sqrt and comparisons only ---------------------------------------------
LM_HD double velocity(const double* I, const double* Q, int32_t i) {
    const double dI = sub(I[i], I[i + 1]), dQ = sub(Q[i], Q[i + 1]);
    return sqrt(add(mul(dI, dI), mul(dQ, dQ)));
}

// smooth() of lib/iqsweep.py:919-971 on the nv = fsteps - 2 velocities: the padded signal
//   s = [2 v[0] - v[top - t] (t = 0 .. top - 2), v, 2 v[nv - 1] - v[nv - 1 - t] (t = 0 .. 8)],
// top = min(10, nv - 1) (numpy's slice v[10:1:-1]); out[i] = sum_{j = 0 .. 9} wn[j] s[i + 13 - j] in
// ascending j from 0.0, i = 0 .. smooth_len - 1 (the 'same' convolution cut to [9:-9]).
LM_HD int32_t smooth_len(int32_t nv) { return (nv - 1 < 10 ? nv - 1 : 10) - 1 + nv - 9; }
LM_HD double padded(const double* v, int32_t nv, int32_t t) {
    const int32_t top = nv - 1 < 10 ? nv - 1 : 10, left = top - 1;
    if (t < left) return sub(mul(2.0, v[0]), v[top - t]);
    if (t < left + nv) return v[t - left];
    return sub(mul(2.0, v[nv - 1]), v[nv - 1 - (t - left - nv)]);
}
LM_HD double smooth_at(const double* v, int32_t nv, const double* wn, int32_t i) {
    double acc = 0.0;
    for (int32_t j = 0; j < kWin; ++j) acc = add(acc, mul(wn[j], padded(v, nv, i + 13 - j)));
    return acc;
}

struct Window {
    int32_t cidx, low, high, n;
};
// cidx: the first index of the maximum, found with `>` from sv[0] (a NaN never wins a comparison)
LM_HD Window window(const double* sv, int32_t nsv, int32_t fsteps) {
    int32_t cidx = 0;
    double best = sv[0];
    for (int32_t i = 1; i < nsv; ++i)
        if (sv[i] > best) best = sv[i], cidx = i;
    const int32_t q = fsteps / 4;
    Window w;
    w.cidx = cidx, w.low = cidx - q > 0 ? cidx - q : 0, w.high = cidx + q < fsteps ? cidx + q : fsteps;
    w.n = w.high - w.low;
    return w;
}

// one channel's window on the host: the velocities, their smoothing, the scan
inline Window window_host(const double* I, const double* Q, int32_t fsteps, const double* wn) {
    double vel[kMaxSteps], sv[kMaxSteps];
    const int32_t nv = fsteps - 2, nsv = smooth_len(nv);
    for (int32_t i = 0; i < nv; ++i) vel[i] = velocity(I, Q, i);
    for (int32_t i = 0; i < nsv; ++i) sv[i] = smooth_at(vel, nv, wn, i);
    return window(sv, nsv, fsteps);
}

#if defined(__HIPCC__)
// The same by a workgroup of T threads: thread t computes velocities t, t + T, .. into the LDS row
// s_vel, then the smoothed velocities from them into s_sv; thread 0 scans for the first maximum.
// -> the window on thread 0 alone, which publishes what the kernel needs of it; the rows are free
// after the barrier that follows that.
__device__ __forceinline__ Window window_group(const double* gI, const double* gQ, int32_t fsteps, const double* wn,
                                               int32_t t, int32_t T, double* s_vel, double* s_sv) {
    const int32_t nv = fsteps - 2, nsv = smooth_len(nv);
    for (int32_t i = t; i < nv; i += T) s_vel[i] = velocity(gI, gQ, i);
    __syncthreads();
    for (int32_t i = t; i < nsv; i += T) s_sv[i] = smooth_at(s_vel, nv, wn, i);
    __syncthreads();
    return t == 0 ? window(s_sv, nsv, fsteps) : Window{};
}
#endif

// ---- guesses, bounds, starts --------------------------------------------------------------------
struct Problem {
    double lo[kNP], hi[kNP];
    double base[kNP];   // f0, gains and offsets of every start; ang1 of starts 0 .. 5
    int32_t status, pad;
};

// x, I, Q, wI, wQ: the n window points. One thread, ascending order.
LM_HD void guesses(const double* x, const double* I, const double* Q, const double* wI, const double* wQ, int32_t n,
                   int32_t k, Problem* pr) {
    bool finite = true;
    double xmin = x[0], xmax = x[0], xsum = 0.0, imin = I[0], imax = I[0], qmin = Q[0], qmax = Q[0];
    for (int32_t i = 0; i < n; ++i) {
        finite = finite && fin(x[i]) && fin(I[i]) && fin(Q[i]) && fin(wI[i]) && fin(wQ[i]);
        xsum = add(xsum, x[i]);
        xmin = x[i] < xmin ? x[i] : xmin, xmax = x[i] > xmax ? x[i] : xmax;
        imin = I[i] < imin ? I[i] : imin, imax = I[i] > imax ? I[i] : imax;
        qmin = Q[i] < qmin ? Q[i] : qmin, qmax = Q[i] > qmax ? Q[i] : qmax;
    }
    const double gI = sub(imax, imin), gQ = sub(qmax, qmin);
    const double icen = add(div(gI, 2.0), imin), qcen = add(div(gQ, 2.0), qmin);
    double ang = atan2(sub(Q[k], qcen), sub(I[k], icen));
    ang = ang >= 0.0 ? sub(ang, div(kPi, 2.0)) : add(ang, div(kPi, 2.0));
    pr->status = !finite ? MKID_LOOP_NONFINITE : ((gI == 0.0 || gQ == 0.0) ? MKID_LOOP_FLAT : 0);
    pr->pad = 0;
    const double alim = mul(1.1, kPi);
    pr->lo[0] = 5e3, pr->hi[0] = 1e6;
    pr->lo[1] = xmin, pr->hi[1] = xmax;
    pr->lo[2] = 1e-4, pr->hi[2] = 1e2;
    pr->lo[3] = 1.0, pr->hi[3] = 4e4;
    pr->lo[4] = -5e3, pr->hi[4] = 5e3;
    pr->lo[5] = -alim, pr->hi[5] = alim;
    pr->lo[6] = sub(gI, mul(0.5, gI)), pr->hi[6] = add(gI, mul(0.5, gI));
    pr->lo[7] = sub(gQ, mul(0.5, gQ)), pr->hi[7] = add(gQ, mul(0.5, gI));   // :215 as written
    pr->lo[8] = sub(icen, mul(0.5, fabs(icen))), pr->hi[8] = add(icen, mul(0.5, fabs(icen)));
    pr->lo[9] = sub(qcen, mul(0.5, fabs(qcen))), pr->hi[9] = add(qcen, mul(0.5, fabs(qcen)));
    for (int32_t i = 0; i < kNP; ++i) pr->base[i] = 0.0;
    pr->base[1] = div(xsum, (double)n);
    pr->base[5] = ang, pr->base[6] = gI, pr->base[7] = gQ, pr->base[8] = icen, pr->base[9] = qcen;
}

// start s of a channel; d = its five draws (g, u2, u3, u4, u5), qg = the caller's Q guess or NaN
LM_HD void make_start(const Problem& pr, int32_t s, const double* d, bool have_q, double qg, double* p) {
    const double qs = have_q ? qg : mul(10000.0, (double)s);
    const double qt = add(qs, mul(20000.0, d[0]));
    p[0] = qt < 5000.0 ? 5000.0 : qt;
    p[1] = pr.base[1];
    p[2] = add(1.1e-4, mul(90.0, d[1]));
    p[3] = add(1.0, mul(3e4, d[2]));
    p[4] = sub(mul(9000.0, d[3]), 4500.0);
    p[5] = s <= 5 ? pr.base[5] : mul(kPi, d[4]);
    p[6] = pr.base[6], p[7] = pr.base[7], p[8] = pr.base[8], p[9] = pr.base[9];
    for (int32_t i = 0; i < kNP; ++i) p[i] = clip(p[i], pr.lo[i], pr.hi[i]);
}

// ---- the model, its Jacobian and its share of the sums ----------------------------------------------
// the model at one frequency (RESDIFF); ca, sa = cos(p5), sin(p5)
struct Point {
    double dx, t, t2, den, c, s, re, im, Ix, Qx, mI, mQ;
};
LM_HD Point model_point(const double* p, double ca, double sa, double x) {
    Point m;
    m.dx = div(sub(x, p[1]), p[1]);
    m.t = mul(mul(2.0, p[0]), m.dx);
    m.t2 = mul(m.t, m.t);
    m.den = add(1.0, m.t2);
    const double ph = mul(m.dx, p[3]);
    m.c = cos(ph), m.s = sin(ph);
    m.re = add(add(mul(p[4], m.dx), sub(div(m.t2, m.den), 0.5)), mul(p[2], sub(1.0, m.c)));
    m.im = sub(div(m.t, m.den), mul(p[2], m.s));
    m.Ix = mul(m.re, p[6]), m.Qx = mul(m.im, p[7]);
    m.mI = add(add(mul(m.Ix, ca), mul(m.Qx, sa)), p[8]);
    m.mQ = add(sub(mul(m.Qx, ca), mul(m.Ix, sa)), p[9]);
    return m;
}

// One window point: residuals r = (y - model) w and J = w d(model)/dp, the I half then the Q half.
LM_HD void point_terms(const double* p, double ca, double sa, double x, double yI, double yQ, double wI, double wQ,
                       double* JI, double* JQ, double* rI, double* rQ) {
    const Point m = model_point(p, ca, sa, x);
    *rI = mul(sub(yI, m.mI), wI), *rQ = mul(sub(yQ, m.mQ), wQ);
    const double den2 = mul(m.den, m.den), twoQ = mul(2.0, p[0]), twodx = mul(2.0, m.dx);
    const double ddx = div(-x, mul(p[1], p[1]));        // d dx / d f0
    const double a = div(mul(2.0, m.t), den2);          // d Re / dt of the dip
    const double b = div(sub(1.0, m.t2), den2);         // d Im / dt
    const double as = mul(p[2], m.s), ac = mul(p[2], m.c);
    double dre[5], dim[5];
    dre[0] = mul(a, twodx), dim[0] = mul(b, twodx);
    dre[1] = mul(ddx, add(add(p[4], mul(twoQ, a)), mul(as, p[3])));
    dim[1] = mul(ddx, sub(mul(twoQ, b), mul(ac, p[3])));
    dre[2] = sub(1.0, m.c), dim[2] = -m.s;
    dre[3] = mul(as, m.dx), dim[3] = -mul(ac, m.dx);
    dre[4] = m.dx, dim[4] = 0.0;
    LM_UNROLL
    for (int32_t k = 0; k < 5; ++k) {
        const double u = mul(p[6], dre[k]), v = mul(p[7], dim[k]);
        JI[k] = mul(add(mul(u, ca), mul(v, sa)), wI);
        JQ[k] = mul(sub(mul(v, ca), mul(u, sa)), wQ);
    }
    JI[5] = mul(sub(mul(m.Qx, ca), mul(m.Ix, sa)), wI);
    JQ[5] = mul(-add(mul(m.Ix, ca), mul(m.Qx, sa)), wQ);
    JI[6] = mul(mul(m.re, ca), wI), JQ[6] = mul(-mul(m.re, sa), wQ);
    JI[7] = mul(mul(m.im, sa), wI), JQ[7] = mul(mul(m.im, ca), wQ);
    JI[8] = wI, JQ[8] = 0.0;
    JI[9] = 0.0, JQ[9] = wQ;
}

// Lane `lane` of 64: points lane, lane + 64, .. of the window in ascending order, I then Q.
LM_HD void lane_partial(const double* p, const double* x, const double* I, const double* Q, const double* wI,
                        const double* wQ, int32_t n, int32_t lane, Sums* s) {
    lm::zero(s);
    const double ca = cos(p[5]), sa = sin(p[5]);
    for (int32_t i = lane; i < n; i += kLanes) {
        double JI[kNP], JQ[kNP], rI, rQ;
        point_terms(p, ca, sa, x[i], I[i], Q[i], wI[i], wQ[i], JI, JQ, &rI, &rQ);
        lm::accumulate(s, JI, rI);
        lm::accumulate(s, JQ, rQ);
    }
}

// ---- the result -------------------------------------------------------------------------------------
LM_HD void finish(const Window& w, int32_t status, const StartResult* best, int32_t best_s, mkid_loop_fit* f) {
    f->cidx = w.cidx, f->low = w.low, f->high = w.high, f->n = w.n, f->pad = 0;
    if (status == 0 && best_s < 0) status = MKID_LOOP_NO_FIT;
    if (status != 0) {
        for (int32_t i = 0; i < kNP; ++i) f->p[i] = nan64();
        f->chisq = f->qc = f->qi = f->dipdb = nan64();
        f->best_start = -1, f->evals = 0, f->status = status;
        return;
    }
    const double* p = best->p;
    for (int32_t i = 0; i < kNP; ++i) f->p[i] = p[i];
    const double rad = div(fabs(add(p[6], p[7])), 4.0);
    const double diam = div(mul(2.0, rad), add(sqrt(add(mul(p[8], p[8]), mul(p[9], p[9]))), rad));
    f->chisq = best->chi;
    f->qc = div(p[0], diam);
    f->qi = div(p[0], sub(1.0, diam));
    f->dipdb = mul(20.0, log10(sub(1.0, diam)));
    f->best_start = best_s, f->evals = best->evals;
    f->status = best->hit_max ? MKID_LOOP_MAX_ITER : 0;
}

// ---- the host twin ----------------------------------------------------------------------------------
// One channel on the host. freq, I, Q (and isd, qsd when given): its fsteps points; draws [S][5].
inline void fit_channel_host(const double* freq, const double* I, const double* Q, const double* isd, const double* qsd,
                             const double* draws, bool have_q, double qg, int32_t fsteps, int32_t S, int32_t max_iter,
                             double ftol, const double* wn, mkid_loop_fit* fit, double* chisq_all) {
    double wI[kMaxWindow], wQ[kMaxWindow];
    const Window w = window_host(I, Q, fsteps, wn);
    for (int32_t i = 0; i < w.n; ++i) {
        wI[i] = isd ? div(1.0, isd[w.low + i]) : 1.0;
        wQ[i] = qsd ? div(1.0, qsd[w.low + i]) : 1.0;
    }
    const double *x = freq + w.low, *yI = I + w.low, *yQ = Q + w.low;
    Problem pr;
    guesses(x, yI, yQ, wI, wQ, w.n, w.cidx - w.low, &pr);
    StartResult best{};
    const int32_t best_s = lm::run_starts_host(
        pr.status, S, max_iter, ftol,
        [&](int32_t s, double* p) { make_start(pr, s, draws + (int64_t)s * 5, have_q, qg, p); },
        lm::host_eval<kNP>(
            [&](const double* p, int32_t lane, Sums* s) { lane_partial(p, x, yI, yQ, wI, wQ, w.n, lane, s); }),
        pr.lo, pr.hi, &best, chisq_all);
    finish(w, pr.status, &best, best_s, fit);
}

inline void fit_host(const double* freq, const double* I, const double* Q, const double* isd, const double* qsd,
                     const double* draws, const double* qguess, int32_t nch, int32_t fsteps, int32_t S, int32_t max_iter,
                     double ftol, mkid_loop_fit* fits, double* chisq_all) {
    double wn[kWin];
    window_weights(wn);
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t o = c * fsteps;
        fit_channel_host(freq + o, I + o, Q + o, isd ? isd + o : nullptr, qsd ? qsd + o : nullptr,
                         draws + c * S * 5, qguess != nullptr, qguess ? qguess[c] : 0.0, fsteps, S, max_iter, ftol, wn,
                         fits + c, chisq_all ? chisq_all + c * S : nullptr);
    }
}

}  // namespace lfit
}  // namespace mkid
