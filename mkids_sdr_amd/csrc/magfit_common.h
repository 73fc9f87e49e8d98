// Resonator magnitude fits (include/mkidgpu.h mkid_fit_mags states the rules), one definition for the
// kernel of k_magfit.hip and for the host entry point mkid_fit_mags_host: the normalised magnitude
// over the whole sweep, the bounds, the starts, the six-parameter magnitude model with its analytic
// Jacobian, its lane partial of the sums and the result. The solver and the drivers that run the
// starts, on the host and in the workgroup, are lm_common.h's at N = 6; the velocity-maximum index
// is the loop fit's (loopfit_common.h: window_host, window_group). No HIP is used: the host loops
// below are the whole of the host entry point, so that the CPU sanitizer build
// (tools/plan_fuzz.cpp) runs them.
//
// Kept from the reference's IQsweep.FitMagMP (lib/iqsweep.py:293-356): the model MAGDIFF (:913-917),
// the normalisation by the largest magnitude, the constant error 1e-5, the bounds, the recipe of the
// ten starts and "the lowest chi^2 wins". The optimiser is this repository's, as in the loop fit.
//
// Every float operation is rounded once and never fused, every sum has a written order, and the
// model uses +, -, x, /, sqrt, |.| and comparisons only, so that device, host twin and a float64
// restatement agree in every bit.
#pragma once
#include "lm_common.h"
#include "loopfit_common.h"

namespace mkid {
namespace mfit {

using lm::add;
using lm::clip;
using lm::div;
using lm::fin;
using lm::kLanes;
using lm::kMaxStarts;
using lm::mul;
using lm::nan64;
using lm::sub;

constexpr int32_t kNP = MKID_MAG_NPAR;   // 6 parameters: Q, f0, carrier, depth, slope, curve
constexpr int32_t kMinSteps = lfit::kMinSteps, kMaxSteps = lfit::kMaxSteps;   // the sweeps are the loop fit's
constexpr double kQFail = 50000.0;       // d_qout of a channel without a fit: FitLoopMP's default Q (:193)

using Sums = lm::SumsT<kNP>;
using StartResult = lm::StartResultT<kNP>;

inline bool args_ok(const double* freq, const double* i, const double* q, const double* draws, int32_t nch, int32_t fsteps,
                    int32_t S, int32_t max_iter, double ftol, const mkid_mag_fit* fits) {
    return freq && i && q && draws && fits && nch >= 1 && fsteps >= kMinSteps && fsteps <= kMaxSteps && S >= 1 &&
           S <= kMaxStarts && max_iter >= 1 && ftol > 0.0;
}

// ---- the data ---------------------------------------------------------------------------------------
LM_HD double magnitude(double I, double Q) { return sqrt(add(mul(I, I), mul(Q, Q))); }
LM_HD double weight() { return div(1.0, 1e-5); }

// ---- bounds and starts ------------------------------------------------------------------------------
struct Problem {
    double lo[kNP], hi[kNP];
    double f0;   // the start's f0 before clipping: (sum of x, ascending) / n
    int32_t status, pad;
};

// x: the n sweep frequencies. One thread, ascending order. nonfinite: a value of x, I or Q that is not
// finite was seen; norm: the largest magnitude.
LM_HD void problem(const double* x, int32_t n, bool nonfinite, double norm, Problem* pr) {
    double xmin = x[0], xmax = x[0], xsum = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        xsum = add(xsum, x[i]);
        xmin = x[i] < xmin ? x[i] : xmin, xmax = x[i] > xmax ? x[i] : xmax;
    }
    pr->status = nonfinite ? MKID_LOOP_NONFINITE : (norm == 0.0 ? MKID_LOOP_FLAT : 0);
    pr->pad = 0;
    pr->lo[0] = 5e3, pr->hi[0] = 1e6;
    pr->lo[1] = xmin, pr->hi[1] = xmax;
    pr->lo[2] = 1e-4, pr->hi[2] = 1e2;
    pr->lo[3] = 0.01, pr->hi[3] = 10.0;
    pr->lo[4] = -5e3, pr->hi[4] = 5e3;
    pr->lo[5] = -1e8, pr->hi[5] = 1e8;
    pr->f0 = div(xsum, (double)n);
}

// start s of a channel; g = its draw (a standard normal)
LM_HD void make_start(const Problem& pr, int32_t s, double g, double* p) {
    const double qt = add(mul(10000.0, (double)s), mul(5000.0, g));
    p[0] = qt < 5000.0 ? 5000.0 : qt;
    p[1] = pr.f0;
    p[2] = 1.0, p[3] = 0.7, p[4] = 0.1, p[5] = -10.0;
    for (int32_t i = 0; i < kNP; ++i) p[i] = clip(p[i], pr.lo[i], pr.hi[i]);
}

// ---- the model, its Jacobian and the sums ---------------------------------------------------------
// the model at one frequency (MAGDIFF) with what the Jacobian shares with it
struct Point {
    double dx, t, den, r, a, m;
};
LM_HD Point model_point(const double* p, double x) {
    Point m;
    m.dx = div(sub(x, p[1]), p[1]);
    m.t = mul(mul(2.0, p[0]), m.dx);
    m.den = add(1.0, mul(m.t, m.t));
    m.r = sqrt(m.den);
    m.a = div(fabs(m.t), m.r);
    m.m = add(add(add(mul(sub(m.a, 1.0), p[3]), p[2]), mul(p[4], m.dx)), mul(mul(p[5], m.dx), m.dx));
    return m;
}

// One point: the residual res = (y - m) w and J = w d(m)/dp.
LM_HD void point_terms(const double* p, double x, double y, double w, double* J, double* res) {
    const Point m = model_point(p, x);
    *res = mul(sub(y, m.m), w);
    const double sg = (double)((m.t > 0.0) - (m.t < 0.0));   // 0 at the cusp t = 0
    const double k = div(sg, mul(m.den, m.r));               // d a / d t
    const double ddx = div(-x, mul(p[1], p[1]));             // d dx / d f0
    const double dk = mul(p[3], k), twoQ = mul(2.0, p[0]);
    J[0] = mul(w, mul(dk, mul(2.0, m.dx)));
    J[1] = mul(w, mul(ddx, add(add(mul(dk, twoQ), p[4]), mul(mul(2.0, p[5]), m.dx))));
    J[2] = w;
    J[3] = mul(w, sub(m.a, 1.0));
    J[4] = mul(w, m.dx);
    J[5] = mul(w, mul(m.dx, m.dx));
}

// Lane `lane` of 64: points lane, lane + 64, .. of the sweep in ascending order.
LM_HD void lane_partial(const double* p, const double* x, const double* y, int32_t n, int32_t lane, Sums* s) {
    lm::zero(s);
    const double w = weight();
    for (int32_t i = lane; i < n; i += kLanes) {
        double J[kNP], res;
        point_terms(p, x[i], y[i], w, J, &res);
        lm::accumulate(s, J, res);
    }
}

// ---- the result -------------------------------------------------------------------------------------
// -> the channel's d_qout value
LM_HD double finish(int32_t cidx, double norm, int32_t status, const StartResult* best, int32_t best_s, mkid_mag_fit* f) {
    f->cidx = cidx, f->norm = norm;
    if (status == 0 && best_s < 0) status = MKID_LOOP_NO_FIT;
    if (status != 0) {
        for (int32_t i = 0; i < kNP; ++i) f->p[i] = nan64();
        f->chisq = nan64();
        f->best_start = -1, f->evals = 0, f->status = status;
        return kQFail;
    }
    for (int32_t i = 0; i < kNP; ++i) f->p[i] = best->p[i];
    f->chisq = best->chi;
    f->best_start = best_s, f->evals = best->evals;
    f->status = best->hit_max ? MKID_LOOP_MAX_ITER : 0;
    return best->p[0];
}

// ---- the host twin ----------------------------------------------------------------------------------
// One channel on the host. freq, I, Q: its fsteps points; draws [S].
inline void fit_channel_host(const double* freq, const double* I, const double* Q, const double* draws, int32_t fsteps,
                             int32_t S, int32_t max_iter, double ftol, const double* wn, mkid_mag_fit* fit, double* qout,
                             double* chisq_all) {
    double y[kMaxSteps];
    const int32_t cidx = lfit::window_host(I, Q, fsteps, wn).cidx;
    bool nonfinite = false;
    for (int32_t i = 0; i < fsteps; ++i) {
        nonfinite = nonfinite || !(fin(freq[i]) && fin(I[i]) && fin(Q[i]));
        y[i] = magnitude(I[i], Q[i]);
    }
    double norm = y[0];
    for (int32_t i = 1; i < fsteps; ++i)
        if (y[i] > norm) norm = y[i];
    for (int32_t i = 0; i < fsteps; ++i) y[i] = div(y[i], norm);
    Problem pr;
    problem(freq, fsteps, nonfinite, norm, &pr);
    StartResult best{};
    const int32_t best_s = lm::run_starts_host(
        pr.status, S, max_iter, ftol, [&](int32_t s, double* p) { make_start(pr, s, draws[s], p); },
        lm::host_eval<kNP>([&](const double* p, int32_t lane, Sums* s) { lane_partial(p, freq, y, fsteps, lane, s); }),
        pr.lo, pr.hi, &best, chisq_all);
    const double qo = finish(cidx, norm, pr.status, &best, best_s, fit);
    if (qout) *qout = qo;
}

inline void fit_host(const double* freq, const double* I, const double* Q, const double* draws, int32_t nch, int32_t fsteps,
                     int32_t S, int32_t max_iter, double ftol, mkid_mag_fit* fits, double* qout, double* chisq_all) {
    double wn[lfit::kWin];
    lfit::window_weights(wn);
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t o = c * fsteps;
        fit_channel_host(freq + o, I + o, Q + o, draws + c * S, fsteps, S, max_iter, ftol, wn, fits + c,
                         qout ? qout + c : nullptr, chisq_all ? chisq_all + c * S : nullptr);
    }
}

}  // namespace mfit
}  // namespace mkid
