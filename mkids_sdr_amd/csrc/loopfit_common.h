// Resonator loop fits (include/mkidgpu.h mkid_fit_loops states the rules), one definition for the
// kernel of k_loopfit.hip and for the host entry point mkid_fit_loops_host: the IQ-velocity window,
// the guesses, the bounds, the starts, the ten-parameter loop model with its analytic Jacobian, the
// 64 lane partials with their butterfly, the damped normal equations with their Cholesky, the
// accept rule and the derived quantities. No HIP is used: the host loops below are the whole of the
// host entry point, so that the CPU sanitizer build (tools/plan_fuzz.cpp) runs them.
//
// Kept from the reference's IQsweep.FitLoopMP (lib/iqsweep.py:141-291): the model RESDIFF
// (:824-858), the window about the fastest point of the loop, the guesses, the bounds, the recipe of
// the random starts, "the lowest chi^2 of S starts wins" and the derived quantities. The optimiser is
// NOT the reference's: mpfit differences the model numerically and draws its starts from an unseeded
// generator, and FitLoopMP itself raises at :231 and re-slices an already windowed array at :211.
// The solver below (Levenberg-Marquardt on analytic normal equations, Marquardt's diagonal scaling,
// projected onto the bounds) is this repository's definition.
//
// Every float operation is rounded once and never fused with its neighbour (the helpers switch
// contraction off for their own statement, as wavecal_common.h's), and every sum has a written
// order, so that device, host twin and a float64 restatement differ only through sin, cos, atan2
// (and log10 in dipdb).
//
// The sums, the butterfly, the step and the run of one start are templates on the number of
// parameters N: the loop fit is their instance at N = 10 and the magnitude fit (magfit_common.h)
// at N = 6, so both fits share one Cholesky, one accept rule and one set of stop rules.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkidgpu.h"

#if defined(__HIPCC__)
#define LFIT_HD __host__ __device__ inline
#else
#define LFIT_HD inline
#endif
#if defined(__clang__)
#define LFIT_NO_FMA _Pragma("clang fp contract(off)")
#define LFIT_UNROLL _Pragma("unroll")
#else
#define LFIT_NO_FMA
#define LFIT_UNROLL
#endif

namespace mkid {
namespace lfit {

constexpr int32_t kNP = MKID_LOOP_NPAR;   // 10 parameters
constexpr int32_t kNA = 55;               // lower triangle of J^T J, entry (i, j <= i) at i (i + 1) / 2 + j
constexpr int32_t kLanes = 64;
constexpr int32_t kMinSteps = 12, kMaxSteps = 1024, kMaxWindow = kMaxSteps / 2, kMaxStarts = 16;
constexpr int32_t kWin = 10;              // hanning(10)
constexpr double kPi = 3.141592653589793;
constexpr double kLam0 = 1e-3, kLamMin = 1e-12, kLamMax = 1e12;

// one IEEE operation each
LFIT_HD double add(double a, double b) { LFIT_NO_FMA return a + b; }
LFIT_HD double sub(double a, double b) { LFIT_NO_FMA return a - b; }
LFIT_HD double mul(double a, double b) { LFIT_NO_FMA return a * b; }
LFIT_HD double div(double a, double b) { LFIT_NO_FMA return a / b; }
LFIT_HD double nan64() { return __builtin_nan(""); }
LFIT_HD bool fin(double v) { return __builtin_isfinite(v); }

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
LFIT_HD double velocity(const double* I, const double* Q, int32_t i) {
    const double dI = sub(I[i], I[i + 1]), dQ = sub(Q[i], Q[i + 1]);
    return sqrt(add(mul(dI, dI), mul(dQ, dQ)));
}

// smooth() of lib/iqsweep.py:919-971 on the nv = fsteps - 2 velocities: the padded signal
//   s = [2 v[0] - v[top - t] (t = 0 .. top - 2), v, 2 v[nv - 1] - v[nv - 1 - t] (t = 0 .. 8)],
// top = min(10, nv - 1) (numpy's slice v[10:1:-1]); out[i] = sum_{j = 0 .. 9} wn[j] s[i + 13 - j] in
// ascending j from 0.0, i = 0 .. smooth_len - 1 (the 'same' convolution cut to [9:-9]).
LFIT_HD int32_t smooth_len(int32_t nv) { return (nv - 1 < 10 ? nv - 1 : 10) - 1 + nv - 9; }
LFIT_HD double padded(const double* v, int32_t nv, int32_t t) {
    const int32_t top = nv - 1 < 10 ? nv - 1 : 10, left = top - 1;
    if (t < left) return sub(mul(2.0, v[0]), v[top - t]);
    if (t < left + nv) return v[t - left];
    return sub(mul(2.0, v[nv - 1]), v[nv - 1 - (t - left - nv)]);
}
LFIT_HD double smooth_at(const double* v, int32_t nv, const double* wn, int32_t i) {
    double acc = 0.0;
    for (int32_t j = 0; j < kWin; ++j) acc = add(acc, mul(wn[j], padded(v, nv, i + 13 - j)));
    return acc;
}

struct Window {
    int32_t cidx, low, high, n;
};
// cidx: the first index of the maximum, found with `>` from sv[0] (a NaN never wins a comparison)
LFIT_HD Window window(const double* sv, int32_t nsv, int32_t fsteps) {
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

// ---- guesses, bounds, starts --------------------------------------------------------------------
struct Problem {
    double lo[kNP], hi[kNP];
    double base[kNP];   // f0, gains and offsets of every start; ang1 of starts 0 .. 5
    int32_t status, pad;
};

LFIT_HD double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// x, I, Q, wI, wQ: the n window points. One thread, ascending order.
LFIT_HD void guesses(const double* x, const double* I, const double* Q, const double* wI, const double* wQ, int32_t n,
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
LFIT_HD void make_start(const Problem& pr, int32_t s, const double* d, bool have_q, double qg, double* p) {
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

// ---- the model, its Jacobian and the sums ---------------------------------------------------------
// The sums of a fit with N parameters (the magnitude fit of magfit_common.h has six): the lower
// triangle of A = J^T J, g = J^T r and chi^2.
template <int32_t N>
struct SumsT {
    double A[N * (N + 1) / 2], g[N], chi;
};
using Sums = SumsT<kNP>;
template <int32_t N>
LFIT_HD void zero(SumsT<N>* s) {
    LFIT_UNROLL
    for (int32_t i = 0; i < N * (N + 1) / 2; ++i) s->A[i] = 0.0;
    LFIT_UNROLL
    for (int32_t i = 0; i < N; ++i) s->g[i] = 0.0;
    s->chi = 0.0;
}

// the model at one frequency (RESDIFF); ca, sa = cos(p5), sin(p5)
struct Point {
    double dx, t, t2, den, c, s, re, im, Ix, Qx, mI, mQ;
};
LFIT_HD Point model_point(const double* p, double ca, double sa, double x) {
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

// one half of a point into the sums: chi, then g_i and A_ij (j <= i) by ascending i, j
template <int32_t N>
LFIT_HD void accumulate(SumsT<N>* s, const double* J, double r) {
    s->chi = add(s->chi, mul(r, r));
    LFIT_UNROLL
    for (int32_t i = 0; i < N; ++i) {
        s->g[i] = add(s->g[i], mul(J[i], r));
        LFIT_UNROLL
        for (int32_t j = 0; j <= i; ++j) s->A[i * (i + 1) / 2 + j] = add(s->A[i * (i + 1) / 2 + j], mul(J[i], J[j]));
    }
}

// One window point: residuals r = (y - model) w and J = w d(model)/dp, the I half then the Q half.
LFIT_HD void point_terms(const double* p, double ca, double sa, double x, double yI, double yQ, double wI, double wQ,
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
    LFIT_UNROLL
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
LFIT_HD void lane_partial(const double* p, const double* x, const double* I, const double* Q, const double* wI,
                          const double* wQ, int32_t n, int32_t lane, Sums* s) {
    zero(s);
    const double ca = cos(p[5]), sa = sin(p[5]);
    for (int32_t i = lane; i < n; i += kLanes) {
        double JI[kNP], JQ[kNP], rI, rQ;
        point_terms(p, ca, sa, x[i], I[i], Q[i], wI[i], wQ[i], JI, JQ, &rI, &rQ);
        accumulate(s, JI, rI);
        accumulate(s, JQ, rQ);
    }
}

// ---- the step -------------------------------------------------------------------------------------
// trial = clip(p + delta), (A + lam diag D) delta = g on the free set (hi > lo and D = A_ii > 0). A
// parameter outside the free set has its row and column replaced by the identity's and g = 0, so
// that its delta is exactly 0 and the others are those of the reduced system. Cholesky, column by
// column, every inner sum by ascending k. false: a pivot that is not positive and finite. N: the
// number of parameters (p, lo, hi, trial [N]).
template <int32_t N>
LFIT_HD bool step(const SumsT<N>& c, double lam, const double* p, const double* lo, const double* hi, double* trial,
                  int32_t* nfree) {
    double L[N * (N + 1) / 2], y[N];
    bool fr[N];
    int32_t nf = 0;
    LFIT_UNROLL
    for (int32_t i = 0; i < N; ++i) {
        fr[i] = hi[i] > lo[i] && c.A[i * (i + 1) / 2 + i] > 0.0;
        nf += fr[i] ? 1 : 0;
    }
    *nfree = nf;
    LFIT_UNROLL
    for (int32_t j = 0; j < N; ++j) {
        const double ajj = c.A[j * (j + 1) / 2 + j];
        double s = fr[j] ? add(ajj, mul(lam, ajj)) : 1.0;
        LFIT_UNROLL
        for (int32_t k = 0; k < j; ++k) s = sub(s, mul(L[j * (j + 1) / 2 + k], L[j * (j + 1) / 2 + k]));
        if (!(s > 0.0 && fin(s))) return false;
        const double d = sqrt(s);
        L[j * (j + 1) / 2 + j] = d;
        LFIT_UNROLL
        for (int32_t i = j + 1; i < N; ++i) {
            double t = fr[i] && fr[j] ? c.A[i * (i + 1) / 2 + j] : 0.0;
            LFIT_UNROLL
            for (int32_t k = 0; k < j; ++k) t = sub(t, mul(L[i * (i + 1) / 2 + k], L[j * (j + 1) / 2 + k]));
            L[i * (i + 1) / 2 + j] = div(t, d);
        }
    }
    LFIT_UNROLL
    for (int32_t i = 0; i < N; ++i) {   // L y = g
        double t = fr[i] ? c.g[i] : 0.0;
        LFIT_UNROLL
        for (int32_t k = 0; k < i; ++k) t = sub(t, mul(L[i * (i + 1) / 2 + k], y[k]));
        y[i] = div(t, L[i * (i + 1) / 2 + i]);
    }
    LFIT_UNROLL
    for (int32_t i = N - 1; i >= 0; --i) {   // L^T delta = y, delta kept in y
        double t = y[i];
        LFIT_UNROLL
        for (int32_t k = i + 1; k < N; ++k) t = sub(t, mul(L[k * (k + 1) / 2 + i], y[k]));
        y[i] = div(t, L[i * (i + 1) / 2 + i]);
    }
    LFIT_UNROLL
    for (int32_t i = 0; i < N; ++i) trial[i] = clip(add(p[i], y[i]), lo[i], hi[i]);
    return true;
}

// ---- one start --------------------------------------------------------------------------------------
template <int32_t N>
struct StartResultT {
    double p[N], chi;
    int32_t evals, hit_max;
};
using StartResult = StartResultT<kNP>;

// eval(p, &sums): the combined sums at p. solve(sums, lam, p, trial, &nfree): step() (the device has
// one lane run it and hands the result to the wave). r->p holds the start on entry.
template <int32_t N, class Eval, class Solve>
LFIT_HD void run_start(int32_t max_iter, double ftol, Eval&& eval, Solve&& solve, StartResultT<N>* r) {
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
            LFIT_UNROLL
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
LFIT_HD bool better(double chi, int32_t s, double best_chi, int32_t best_s) {
    if (!fin(chi)) return false;
    return best_s < 0 || chi < best_chi || (chi == best_chi && s < best_s);
}

// ---- the result -------------------------------------------------------------------------------------
LFIT_HD void finish(const Window& w, int32_t status, const StartResult* best, int32_t best_s, mkid_loop_fit* f) {
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

struct HostEval {
    const double *x, *I, *Q, *wI, *wQ;
    int32_t n;
    void operator()(const double* p, Sums* out) const {
        Sums part[kLanes];
        for (int32_t l = 0; l < kLanes; ++l) lane_partial(p, x, I, Q, wI, wQ, n, l, &part[l]);
        butterfly_host(part);
        *out = part[0];
    }
};

// One channel on the host. freq, I, Q (and isd, qsd when given): its fsteps points; draws [S][5].
inline void fit_channel_host(const double* freq, const double* I, const double* Q, const double* isd, const double* qsd,
                             const double* draws, bool have_q, double qg, int32_t fsteps, int32_t S, int32_t max_iter,
                             double ftol, const double* wn, mkid_loop_fit* fit, double* chisq_all) {
    double vel[kMaxSteps], sv[kMaxSteps], wI[kMaxWindow], wQ[kMaxWindow];
    const int32_t nv = fsteps - 2, nsv = smooth_len(nv);
    for (int32_t i = 0; i < nv; ++i) vel[i] = velocity(I, Q, i);
    for (int32_t i = 0; i < nsv; ++i) sv[i] = smooth_at(vel, nv, wn, i);
    const Window w = window(sv, nsv, fsteps);
    for (int32_t i = 0; i < w.n; ++i) {
        wI[i] = isd ? div(1.0, isd[w.low + i]) : 1.0;
        wQ[i] = qsd ? div(1.0, qsd[w.low + i]) : 1.0;
    }
    Problem pr;
    guesses(freq + w.low, I + w.low, Q + w.low, wI, wQ, w.n, w.cidx - w.low, &pr);
    StartResult best{}, r{};
    int32_t best_s = -1;
    for (int32_t s = 0; s < S; ++s) {
        if (pr.status != 0) {
            if (chisq_all) chisq_all[s] = nan64();
            continue;
        }
        make_start(pr, s, draws + (int64_t)s * 5, have_q, qg, r.p);
        const HostEval ev{freq + w.low, I + w.low, Q + w.low, wI, wQ, w.n};
        run_start(
            max_iter, ftol, ev,
            [&](const Sums& c, double lam, const double* p, double* trial, int32_t* nfree) {
                return step(c, lam, p, pr.lo, pr.hi, trial, nfree);
            },
            &r);
        if (chisq_all) chisq_all[s] = r.chi;
        if (better(r.chi, s, best.chi, best_s)) best = r, best_s = s;
    }
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
