// Welch spectra of two real float64 series per channel and the IQ noise analysis built on them
// (IQsweep.AnalyzeNoise, lib/iqsweep.py:770-822; include/mkidgpu.h mkid_welch_psd and mkid_iq_noise
// state the rules), one definition for the kernels of k_welch.hip and for the host entry points
// mkid_welch_psd_host and mkid_iq_noise_host: the butterflies, the pass structure with its index
// maps, the four-step split, the unpacking of two real series carried as one complex one, the strip
// sums, the density, and the per-sample phase and amplitude of an IQ record. The sources of the
// samples are loaders, ld(j) -> (a[j], b[j]), so that the engine and the analysis share every line
// below them.
//
// Every float64 operation is a single rounded IEEE operation in a fixed order (each function switches
// contraction off for itself), so device and host twin give the same bits wherever no atan2, sin or
// cos is involved.
//
// The transform of length n = 2^m is decimation in frequency, in place: radix 8 while three bits
// remain, then one pass of radix 4 or 2 (Plan). Pass s works on blocks of L = n / (r_0 .. r_{s-1})
// elements, M = L / r_s; butterfly u = b M + j reads the r elements at b L + j + q M, and its output t,
//     W_L^{j t} * sum_q x[b L + j + q M] W_r^{q t}           W_m = exp(-2 pi i / m),
// goes to b L + t M + j: a butterfly writes where it read, so a pass needs no second buffer. After the
// last pass bin k stands at pos_of_bin(k), the mixed-radix digit reversal. W_L^{j t} is entry
// j t (len / L) of a table of len entries W_len^i with n | len (the four-step transform's column and
// row transforms read the nfft-entry table with a stride).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "mkidgpu.h"

#if defined(__HIPCC__)
#define WELCH_HD __host__ __device__ inline
#else
#define WELCH_HD inline
#endif
#if defined(__clang__)
#define WELCH_NO_FMA _Pragma("clang fp contract(off)")
#else
#define WELCH_NO_FMA
#endif

namespace mkid {
namespace welch {

constexpr int32_t kStrip = MKID_WELCH_STRIP;
constexpr int32_t kLdsMaxN = MKID_WELCH_LDS_MAX_N;
constexpr int32_t kMaxN = MKID_WELCH_MAX_N;
constexpr double kSqrtHalf = 0.70710678118654752440;    // W_8^1 = kSqrtHalf (1 - i)

struct Cx {
    double re, im;
};

WELCH_HD bool pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }
WELCH_HD int32_t log2i(int32_t n) {
    int32_t m = 0;
    while ((1 << m) < n) ++m;
    return m;
}
WELCH_HD bool finite(double x) { return __builtin_isfinite(x); }
WELCH_HD double nan64() { return __builtin_nan(""); }

// ---- shapes ---------------------------------------------------------------------------------------
WELCH_HD int64_t segments(int64_t n, int32_t nfft) { return (n - nfft / 2) / (nfft / 2); }
WELCH_HD int64_t strips(int64_t nseg) { return (nseg + kStrip - 1) / kStrip; }
WELCH_HD bool four_step(int32_t nfft) { return nfft > kLdsMaxN; }
// nfft = n1 n2 for the four-step transform: n1 = 2^floor(log2(nfft) / 2)
WELCH_HD void split(int32_t nfft, int32_t& n1, int32_t& n2) {
    n1 = 1 << (log2i(nfft) / 2);
    n2 = nfft / n1;
}

inline bool psd_args_ok(const double* a, int64_t n, int64_t ld, int32_t nch, int32_t nfft, double fs, int32_t group,
                        const double* pa) {
    return a && pa && nch >= 1 && pow2(nfft) && nfft >= 8 && nfft <= kMaxN && n >= nfft && n <= INT32_MAX &&
           ld >= n && group >= 0 && finite(fs) && fs > 0.0;
}

// ---- the passes -----------------------------------------------------------------------------------
struct Plan {
    int32_t n, npass, n8, last;   // n8 passes of radix 8, then one of radix `last` (4 or 2) if npass > n8
};
WELCH_HD Plan make_plan(int32_t n) {   // n = 2^m, 2 <= n <= kLdsMaxN
    const int32_t m = log2i(n);
    return Plan{n, (m + 2) / 3, m / 3, 1 << (m % 3)};
}
WELCH_HD int32_t radix(const Plan& p, int32_t s) { return s < p.n8 ? 8 : p.last; }
// where bin k stands after the last pass
WELCH_HD int32_t pos_of_bin(const Plan& p, int32_t k) {
    int32_t L = p.n, pos = 0;
    for (int32_t s = 0; s < p.npass; ++s) {
        const int32_t r = radix(p, s), M = L / r;
        pos += (k & (r - 1)) * M;
        k /= r;
        L = M;
    }
    return pos;
}

WELCH_HD Cx cmul(Cx a, Cx b) {
    WELCH_NO_FMA
    return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// x[t] <- sum_q x[q] W_R^{q t}, in natural order
template <int R>
WELCH_HD void dft(Cx* x);
template <>
WELCH_HD void dft<2>(Cx* x) {
    WELCH_NO_FMA
    const Cx a = x[0], b = x[1];
    x[0] = Cx{a.re + b.re, a.im + b.im};
    x[1] = Cx{a.re - b.re, a.im - b.im};
}
template <>
WELCH_HD void dft<4>(Cx* x) {
    WELCH_NO_FMA
    const Cx s0{x[0].re + x[2].re, x[0].im + x[2].im}, s1{x[0].re - x[2].re, x[0].im - x[2].im};
    const Cx s2{x[1].re + x[3].re, x[1].im + x[3].im}, s3{x[1].re - x[3].re, x[1].im - x[3].im};
    x[0] = Cx{s0.re + s2.re, s0.im + s2.im};
    x[2] = Cx{s0.re - s2.re, s0.im - s2.im};
    x[1] = Cx{s1.re + s3.im, s1.im - s3.re};   // s1 - i s3
    x[3] = Cx{s1.re - s3.im, s1.im + s3.re};   // s1 + i s3
}
template <>
WELCH_HD void dft<8>(Cx* x) {
    WELCH_NO_FMA
    Cx e[4] = {x[0], x[2], x[4], x[6]}, o[4] = {x[1], x[3], x[5], x[7]};
    dft<4>(e);
    dft<4>(o);
    // o[t] W_8^t: 1, kSqrtHalf (1 - i), -i, kSqrtHalf (-1 - i)
    const Cx o1{kSqrtHalf * (o[1].re + o[1].im), kSqrtHalf * (o[1].im - o[1].re)};
    const Cx o2{o[2].im, -o[2].re};
    const Cx o3{kSqrtHalf * (o[3].im - o[3].re), -(kSqrtHalf * (o[3].re + o[3].im))};
    const Cx w[4] = {o[0], o1, o2, o3};
    for (int t = 0; t < 4; ++t) {
        x[t] = Cx{e[t].re + w[t].re, e[t].im + w[t].im};
        x[t + 4] = Cx{e[t].re - w[t].re, e[t].im - w[t].im};
    }
}

template <int R, class Z, class Tw>
WELCH_HD void butterfly_r(int32_t L, int32_t u, int32_t tws, Z z, Tw tw) {
    const int32_t M = L / R, b = u / M, j = u - b * M, base = b * L + j;
    Cx x[R];
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < R; ++q) x[q] = z(base + q * M);
    dft<R>(x);
    z(base) = x[0];
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 1; t < R; ++t) z(base + t * M) = j ? cmul(x[t], tw(j * t * tws)) : x[t];
}
// Butterfly u < n / r of a pass of radix r on blocks of L elements. z(i) is a reference to element i
// of the transform, tw(i) entry i of the twiddle table, tws = (the table's length) / L.
template <class Z, class Tw>
WELCH_HD void butterfly(int32_t r, int32_t L, int32_t u, int32_t tws, Z z, Tw tw) {
    if (r == 8)
        butterfly_r<8>(L, u, tws, z, tw);
    else if (r == 4)
        butterfly_r<4>(L, u, tws, z, tw);
    else
        butterfly_r<2>(L, u, tws, z, tw);
}

WELCH_HD Cx windowed(Cx v, double w) {
    WELCH_NO_FMA
    return Cx{v.re * w, v.im * w};
}
// the four-step transform's twiddle on column j2's output k1: W_nfft^{j2 k1}
template <class Tw>
WELCH_HD Cx step_twiddle(Cx v, int32_t idx, Tw tw) {
    return idx ? cmul(v, tw(idx)) : v;
}

// Two real series a and b carried as z = a + i b (noise_common.h unpack_power's statement): with
// Z1 = Z[k] and Z2 = Z[(n - k) mod n], A[k] = (Z1 + conj Z2) / 2 and B[k] = (Z1 - conj Z2) / 2i.
WELCH_HD void unpack_power(Cx z1, Cx z2, double& pa, double& pb) {
    WELCH_NO_FMA
    const double ar = z1.re + z2.re, ai = z1.im - z2.im;
    const double br = z1.re - z2.re, bi = z1.im + z2.im;
    pa = 0.25 * (ar * ar + ai * ai);
    pb = 0.25 * (br * br + bi * bi);
}

// a strip's sum gains a segment's power; the total gains a strip's sum: both start from 0.0
WELCH_HD double add(double acc, double p) {
    WELCH_NO_FMA
    return acc + p;
}

// P[k] from the total over the segments; den = fs * S2, one product made by the entry points
WELCH_HD double density(double tot, double nseg, double den, int32_t k, int32_t half) {
    WELCH_NO_FMA
    const double p = (tot / nseg) / den;
    return (k > 0 && k < half) ? p * 2.0 : p;
}

// ---- tables (host) --------------------------------------------------------------------------------
// W_n^i = (cos, -sin)(2 pi i / n), each from an argument in [0, pi / 4] (one rounding of a product)
// turned through the quadrant, so that the table's error is that of cos and sin themselves
inline Cx twiddle(int64_t i, int64_t n) {
    const int64_t qd = (4 * i) / n, rem = 4 * i - qd * n;   // 2 pi i / n = (pi / 2) (qd + rem / n)
    const bool flip = 2 * rem > n;
    const double ang = M_PI_2 * ((double)(flip ? n - rem : rem) / (double)n);
    double c = cos(ang), s = sin(ang);
    if (flip) {
        const double t = c;
        c = s, s = t;
    }
    switch (qd & 3) {
        case 0: return Cx{c, -s};
        case 1: return Cx{-s, -c};
        case 2: return Cx{-c, s};
        default: return Cx{s, c};
    }
}
struct Tables {
    std::vector<double> w;   // [nfft] the window
    std::vector<Cx> tw;      // [nfft] W_nfft^i
    double S2 = 0.0;
};
// S2 is added in ascending j with Kahan's compensation: the plain sum's rounding error (2.4e-14 of S2 at
// nfft = 262144) scales every bin and would by itself take more than the tests' bar allows a bin
// that holds most of the power (the DC bin of an amplitude series).
inline void make_tables(int32_t nfft, Tables& t) {
    t.w.resize((size_t)nfft);
    t.tw.resize((size_t)nfft);
    double sum = 0.0, comp = 0.0;
    for (int32_t j = 0; j < nfft; ++j) {
        WELCH_NO_FMA
        const double w = 0.5 - 0.5 * cos(2.0 * M_PI * (double)j / (double)(nfft - 1));
        const double term = w * w - comp, next = sum + term;
        comp = (next - sum) - term;
        sum = next;
        t.w[(size_t)j] = w;
        t.tw[(size_t)j] = twiddle(j, nfft);
    }
    t.S2 = sum;
}

// ---- the sequential statement of the kernels (host twin) -------------------------------------------
// The powers of one segment: samples ld(base + j), j < nfft, windowed, transformed in z (nfft
// elements; y, nfft more, is the four-step transform's workspace) and unpacked into pa, pb [half + 1].
template <class Loader>
inline void segment_host(int32_t nfft, const Tables& t, Loader ld, int64_t base, Cx* z, Cx* y, double* pa,
                         double* pb) {
    const Cx* twp = t.tw.data();
    auto tw = [twp](int32_t i) { return twp[i]; };
    const int32_t half = nfft / 2;
    if (!four_step(nfft)) {
        const Plan p = make_plan(nfft);
        for (int32_t j = 0; j < nfft; ++j) z[j] = windowed(ld(base + j), t.w[(size_t)j]);
        int32_t L = nfft;
        for (int32_t s = 0; s < p.npass; L /= radix(p, s), ++s)
            for (int32_t u = 0; u < nfft / radix(p, s); ++u)
                butterfly(radix(p, s), L, u, nfft / L, [z](int32_t i) -> Cx& { return z[i]; }, tw);
        for (int32_t k = 0; k <= half; ++k)
            unpack_power(z[pos_of_bin(p, k)], z[pos_of_bin(p, (nfft - k) & (nfft - 1))], pa[k], pb[k]);
        return;
    }
    int32_t n1, n2;
    split(nfft, n1, n2);
    const Plan p1 = make_plan(n1), p2 = make_plan(n2);
    for (int32_t j2 = 0; j2 < n2; ++j2) {   // columns: over j1, then the twiddle
        for (int32_t j1 = 0; j1 < n1; ++j1) {
            const int32_t j = n2 * j1 + j2;
            z[j1] = windowed(ld(base + j), t.w[(size_t)j]);
        }
        int32_t L = n1;
        for (int32_t s = 0; s < p1.npass; L /= radix(p1, s), ++s)
            for (int32_t u = 0; u < n1 / radix(p1, s); ++u)
                butterfly(radix(p1, s), L, u, nfft / L, [z](int32_t i) -> Cx& { return z[i]; }, tw);
        for (int32_t k1 = 0; k1 < n1; ++k1) y[(size_t)k1 * n2 + j2] = step_twiddle(z[pos_of_bin(p1, k1)], j2 * k1, tw);
    }
    for (int32_t k1 = 0; k1 < n1; ++k1) {   // rows: over j2
        Cx* row = y + (size_t)k1 * n2;
        int32_t L = n2;
        for (int32_t s = 0; s < p2.npass; L /= radix(p2, s), ++s)
            for (int32_t u = 0; u < n2 / radix(p2, s); ++u)
                butterfly(radix(p2, s), L, u, nfft / L, [row](int32_t i) -> Cx& { return row[i]; }, tw);
    }
    for (int32_t k = 0; k <= half; ++k) {   // bin k = k1 + n1 k2 stands in row k1 at pos_of_bin(k2)
        const int32_t kk = (nfft - k) & (nfft - 1);
        const Cx z1 = y[(size_t)(k % n1) * n2 + pos_of_bin(p2, k / n1)];
        const Cx z2 = y[(size_t)(kk % n1) * n2 + pos_of_bin(p2, kk / n1)];
        unpack_power(z1, z2, pa[k], pb[k]);
    }
}

// Where a channel's densities go: bins k_lo .. k_hi - 1 to out_a[off + k - k_lo] (and out_b, nullable)
struct Sink {
    double* out_a;
    double* out_b;
    int32_t k_lo, k_hi;
    int64_t off;
};

// One channel: the strips in ascending order, a strip's segments in ascending order
template <class Loader>
inline void channel_host(int32_t nfft, const Tables& t, Loader ld, int64_t n, double fs, const Sink& o) {
    const int32_t half = nfft / 2;
    const int64_t nseg = segments(n, nfft);
    std::vector<Cx> z((size_t)nfft), y(four_step(nfft) ? (size_t)nfft : 1);
    std::vector<double> pa((size_t)half + 1), pb((size_t)half + 1), sa((size_t)half + 1), sb((size_t)half + 1),
        ta((size_t)half + 1, 0.0), tb((size_t)half + 1, 0.0);
    for (int64_t s0 = 0; s0 < nseg; s0 += kStrip) {
        std::fill(sa.begin(), sa.end(), 0.0);
        std::fill(sb.begin(), sb.end(), 0.0);
        for (int64_t s = s0; s < nseg && s < s0 + kStrip; ++s) {
            segment_host(nfft, t, ld, s * half, z.data(), y.data(), pa.data(), pb.data());
            for (int32_t k = 0; k <= half; ++k) sa[(size_t)k] = add(sa[(size_t)k], pa[(size_t)k]), sb[(size_t)k] = add(sb[(size_t)k], pb[(size_t)k]);
        }
        for (int32_t k = 0; k <= half; ++k) ta[(size_t)k] = add(ta[(size_t)k], sa[(size_t)k]), tb[(size_t)k] = add(tb[(size_t)k], sb[(size_t)k]);
    }
    const double den = fs * t.S2;
    for (int32_t k = o.k_lo; k < o.k_hi; ++k) {
        o.out_a[o.off + k - o.k_lo] = density(ta[(size_t)k], (double)nseg, den, k, half);
        if (o.out_b) o.out_b[o.off + k - o.k_lo] = density(tb[(size_t)k], (double)nseg, den, k, half);
    }
}

// the engine's loader: two float64 rows (b null: zeros)
struct RowLoader {
    const double* a;
    const double* b;
    WELCH_HD Cx operator()(int64_t j) const { return Cx{a[j], b ? b[j] : 0.0}; }
};

// ---- the IQ noise analysis ------------------------------------------------------------------------
inline bool iq_cfg_ok(const mkid_iqnoise_cfg* c) {
    if (!c) return false;
    if (!pow2(c->nfft_high) || c->nfft_high < 8 || c->nfft_high > kLdsMaxN) return false;
    if (!pow2(c->nfft_low) || c->nfft_low <= c->nfft_high || c->nfft_low > kMaxN) return false;
    const int64_t r = c->nfft_low / c->nfft_high;
    if (c->k_join < 1 || c->k_join >= c->nfft_high / 2 || r * c->k_join > c->nfft_low / 2) return false;
    const int64_t nout = r * c->k_join + c->nfft_high / 2 - c->k_join;
    if (c->fit_count < 2 || c->fit_first < 0 || (int64_t)c->fit_first + c->fit_count > nout) return false;
    if (c->group < 0 || !finite(c->samprate) || c->samprate <= 0.0 || !finite(c->f_eval)) return false;
    return finite(c->gain) && c->gain != 0.0 && finite(c->full_scale) && c->full_scale != 0.0;
}
inline bool iq_args_ok(const int16_t* i, const int16_t* q, int64_t n, int64_t ld, int32_t nch, const double* i0,
                       const double* q0, const double* icen, const double* qcen, const double* qfit,
                       const mkid_iqnoise_cfg* c, const double* pn, const double* an,
                       const mkid_iqnoise_result* res) {
    return i && q && i0 && q0 && icen && qcen && qfit && pn && an && res && iq_cfg_ok(c) && nch >= 1 &&
           n >= c->nfft_low && n <= INT32_MAX && ld >= n;
}
WELCH_HD int32_t iq_join(const mkid_iqnoise_cfg& c) { return (c.nfft_low / c.nfft_high) * c.k_join; }
WELCH_HD int32_t iq_nout(const mkid_iqnoise_cfg& c) { return iq_join(c) + c.nfft_high / 2 - c.k_join; }
// the frequency of stitched bin b: that of the bin's own resolution
WELCH_HD double iq_freq(const mkid_iqnoise_cfg& c, int32_t b) {
    const int32_t jn = iq_join(c);
    return b < jn ? (double)b * (c.samprate / (double)c.nfft_low)
                  : (double)(b - jn + c.k_join) * (c.samprate / (double)c.nfft_high);
}

// a sample or a mean in counts -> moved to the loop centre
WELCH_HD double iq_centred(double x, double gain, double full_scale, double z0, double cen) {
    WELCH_NO_FMA
    return (((x * gain) / full_scale) - z0) - cen;
}

// a channel's constants from its exact sums; fn1k is left for iq_fn1k
WELCH_HD void iq_means(int64_t SI, int64_t SQ, int64_t n, const mkid_iqnoise_cfg& c, double i0, double q0, double icen,
                       double qcen, double qfit, mkid_iqnoise_result* r) {
    WELCH_NO_FMA
    const double mI = iq_centred((double)SI / (double)n, c.gain, c.full_scale, i0, icen);
    const double mQ = iq_centred((double)SQ / (double)n, c.gain, c.full_scale, q0, qcen);
    const double ang = atan2(mQ, mI), cs = cos(ang), sn = sin(ang);
    const double rad = mI * cs + mQ * sn;
    int32_t st = 0;
    if (!(finite(i0) && finite(q0) && finite(icen) && finite(qcen))) st |= MKID_IQN_NONFINITE;
    if (!finite(rad) || rad == 0.0) st |= MKID_IQN_BAD_RAD;
    if (!finite(qfit) || qfit == 0.0) st |= MKID_IQN_BAD_Q;
    r->mean_i = mI, r->mean_q = mQ, r->resang = ang, r->rad = rad, r->fn1k = nan64();
    r->sum_i = SI, r->sum_q = SQ;
    r->nseg_low = (int32_t)segments(n, c.nfft_low), r->nseg_high = (int32_t)segments(n, c.nfft_high);
    r->status = st, r->pad = 0;
}

// the analysis's loader: (phase, amp) of sample j of an int16 IQ record; a channel whose rad is
// unusable loads zeros (its spectra are overwritten with NaN by iq_fn1k)
struct IqLoader {
    const int16_t* xi;
    const int16_t* xq;
    double gain, full_scale, i0, q0, icen, qcen, cs, sn, rad;
    bool bad;
    WELCH_HD IqLoader(const int16_t* i, const int16_t* q, const mkid_iqnoise_cfg& c, double i0_, double q0_,
                      double icen_, double qcen_, const mkid_iqnoise_result& r)
        : xi(i), xq(q), gain(c.gain), full_scale(c.full_scale), i0(i0_), q0(q0_), icen(icen_), qcen(qcen_),
          cs(cos(r.resang)), sn(sin(r.resang)), rad(r.rad), bad((r.status & MKID_IQN_BAD_RAD) != 0) {}
    WELCH_HD Cx operator()(int64_t j) const {
        WELCH_NO_FMA
        if (bad) return Cx{0.0, 0.0};
        const double Ia = iq_centred((double)xi[j], gain, full_scale, i0, icen);
        const double Qa = iq_centred((double)xq[j], gain, full_scale, q0, qcen);
        const double nI = (Ia * cs + Qa * sn) / rad, nQ = (Qa * cs - Ia * sn) / rad;
        return Cx{atan2(nQ, nI), sqrt(nI * nI + nQ * nQ)};
    }
};

// The line through stitched bins fit_first .. of pn, read at f_eval, over 16 Q^2; NaN where the status
// says so. (The caller fills pn and an with NaN first where rad is unusable.)
WELCH_HD double iq_fn1k(const mkid_iqnoise_cfg& c, const double* pn, double qfit, int32_t status) {
    WELCH_NO_FMA
    if (status & (MKID_IQN_BAD_RAD | MKID_IQN_BAD_Q)) return nan64();
    const int32_t b0 = c.fit_first, m = c.fit_count;
    double xm = 0.0, ym = 0.0;
    for (int32_t i = 0; i < m; ++i) xm = xm + iq_freq(c, b0 + i), ym = ym + pn[b0 + i];
    xm = xm / (double)m, ym = ym / (double)m;
    double sxy = 0.0, sxx = 0.0;
    for (int32_t i = 0; i < m; ++i) {
        const double dx = iq_freq(c, b0 + i) - xm, dy = pn[b0 + i] - ym;
        sxy = sxy + dx * dy;
        sxx = sxx + dx * dx;
    }
    const double slope = sxy / sxx;
    const double v = ym + slope * (c.f_eval - xm);
    return v / (16.0 * (qfit * qfit));
}

// the sinks of the two resolutions into a channel's stitched rows
WELCH_HD Sink iq_sink_low(const mkid_iqnoise_cfg& c, double* pn, double* an) { return Sink{pn, an, 0, iq_join(c), 0}; }
WELCH_HD Sink iq_sink_high(const mkid_iqnoise_cfg& c, double* pn, double* an) {
    return Sink{pn, an, c.k_join, c.nfft_high / 2, iq_join(c)};
}

}  // namespace welch
}  // namespace mkid
