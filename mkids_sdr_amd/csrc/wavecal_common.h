// Energy calibration from laser spectra and the energy cube (include/mkidgpu.h mkid_spectrum_lines,
// mkid_energy_cube state the rules), one definition for the kernels of k_wavecal.hip and for the host
// entry points mkid_spectrum_lines_host / mkid_energy_cube_host: the smoothed spectrum, which bins
// are line candidates, the greedy selection, a line's fit window, Caruana's log-parabola in float64,
// the height -> energy polynomial with the resolving power, and a photon's energy and cube column.
// No HIP is used: the host loops below are the whole of the host entry points, so that the CPU
// sanitizer build (tools/plan_fuzz.cpp) runs them.
//
// Every float operation here is rounded once and never fused with its neighbour. The device's
// __dmul_rn / __dadd_rn / __fmul_rn / __fadd_rn are plain operators to the compiler, which contracts
// a product and a sum written next to each other into one fma whatever they are called, so each
// helper below switches contraction off for its own statement instead; the hosts built for have no
// fused instruction.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mkidgpu.h"
#include "obs_common.h"

#if defined(__HIPCC__)
#define WCAL_HD __host__ __device__ inline
#else
#define WCAL_HD inline
#endif
#if defined(__clang__)
#define WCAL_NO_FMA _Pragma("clang fp contract(off)")
#else
#define WCAL_NO_FMA
#endif

namespace mkid {
namespace wcal {

constexpr int32_t kMaxLines = MKID_CAL_MAX_LINES;
constexpr int32_t kMaxSmooth = 64;
constexpr int32_t kMaxFitHalf = 64;
constexpr double kFwhm = 2.3548200450309493;   // 2 sqrt(2 ln 2)

struct Params {
    int32_t nbins, P, w, min_sep, g, pad;
    int64_t min_peak;
    double E[kMaxLines];
};

// one IEEE operation each
WCAL_HD double add(double a, double b) { WCAL_NO_FMA return a + b; }
WCAL_HD double sub(double a, double b) { WCAL_NO_FMA return a - b; }
WCAL_HD double mul(double a, double b) { WCAL_NO_FMA return a * b; }
WCAL_HD double div(double a, double b) { WCAL_NO_FMA return a / b; }
WCAL_HD float addf(float a, float b) { WCAL_NO_FMA return a + b; }
WCAL_HD float mulf(float a, float b) { WCAL_NO_FMA return a * b; }
WCAL_HD float divf(float a, float b) { WCAL_NO_FMA return a / b; }
WCAL_HD double nan64() { return __builtin_nan(""); }
WCAL_HD float nan32() {   // the one NaN an energy is stored as
    float f;
    __builtin_memcpy(&f, &obs::kNanBits, 4);
    return f;
}

inline bool energies_ok(const double* E, int32_t P) {
    if (!E || P < 1 || P > kMaxLines) return false;
    for (int32_t p = 0; p < P; ++p) {
        if (!(__builtin_isfinite(E[p]) && E[p] > 0.0)) return false;
        for (int32_t q = 0; q < p; ++q)
            if (E[q] == E[p]) return false;
    }
    return true;
}

inline bool lines_args_ok(const int32_t* spectra, const float* lo, const float* step, int32_t nch, int32_t nbins,
                          int32_t P, const double* E, int32_t w, int32_t min_sep, int32_t g, const mkid_line_fit* lines,
                          const mkid_energy_cal* cal, const float* cal_f) {
    return spectra && lo && step && lines && cal && cal_f && nch >= 1 && obs::bins_ok(nbins) && energies_ok(E, P) &&
           w >= 0 && w <= kMaxSmooth && min_sep >= 1 && g >= 1 && g <= kMaxFitHalf;
}

inline Params make_params(int32_t nbins, int32_t P, const double* E, int32_t w, int32_t min_sep, int64_t min_peak,
                          int32_t g) {
    Params p{};
    p.nbins = nbins, p.P = P, p.w = w, p.min_sep = min_sep, p.g = g, p.min_peak = min_peak;
    for (int32_t i = 0; i < kMaxLines; ++i) p.E[i] = i < P ? E[i] : nan64();
    return p;
}

// ---- integer part -------------------------------------------------------------------------------
// n: the nbins bins of one channel (columns 1 .. nbins of its spectra row), a count read as uint32.
WCAL_HD int64_t count(const int32_t* n, int32_t nbins, int32_t b) {
    return b < 0 || b >= nbins ? 0 : (int64_t)(uint32_t)n[b];
}

// s[b] = sum_{k = -w .. w} (w + 1 - |k|) n[b + k]; at most 65^2 (2^32 - 1) < 2^45
WCAL_HD int64_t smooth_at(const int32_t* n, int32_t nbins, int32_t w, int32_t b) {
    if (b < 0 || b >= nbins) return 0;
    int64_t s = 0;
    for (int32_t k = -w; k <= w; ++k) s += (int64_t)(w + 1 - (k < 0 ? -k : k)) * count(n, nbins, b + k);
    return s;
}

// The selection key of bin b: 0 when b is no candidate, else s[b] 2^15 + (32767 - b), so that the
// largest key is the largest s and, among equal s, the lowest bin.
WCAL_HD uint64_t candidate_key(const int32_t* n, int32_t nbins, int32_t w, int64_t min_peak, int32_t b) {
    const int64_t s = smooth_at(n, nbins, w, b);
    if (s < min_peak || s < 1) return 0;   // s > s[b - 1] >= 0 needs s >= 1
    if (!(s > smooth_at(n, nbins, w, b - 1) && s >= smooth_at(n, nbins, w, b + 1))) return 0;
    return (uint64_t)s << 15 | (uint64_t)(32767 - b);
}
WCAL_HD int32_t key_bin(uint64_t key) { return 32767 - (int32_t)(key & 32767); }

// bin b lies closer than min_sep to one of the r lines chosen so far
WCAL_HD bool excluded(int32_t b, const int32_t* chosen, int32_t r, int32_t min_sep) {
    for (int32_t i = 0; i < r; ++i) {
        const int32_t d = b - chosen[i];
        if ((d < 0 ? -d : d) < min_sep) return true;
    }
    return false;
}

WCAL_HD void sort_bins(int32_t* bins, int32_t found) {
    for (int32_t i = 1; i < found; ++i)
        for (int32_t j = i; j > 0 && bins[j - 1] > bins[j]; --j) {
            const int32_t t = bins[j];
            bins[j] = bins[j - 1], bins[j - 1] = t;
        }
}

// Fit window of line p of the `found` lines at ascending bins: b0 .. b1 inclusive.
struct Window {
    int32_t b0, b1;
};
WCAL_HD Window window(const int32_t* bins, int32_t found, int32_t p, int32_t g, int32_t nbins) {
    const int32_t m = bins[p];
    const int32_t L = p > 0 ? (bins[p - 1] + m) / 2 + 1 : 0;
    const int32_t H = p + 1 < found ? (m + bins[p + 1]) / 2 : nbins - 1;
    return Window{m - g > L ? m - g : L, m + g < H ? m + g : H};
}

// ---- float64 part -------------------------------------------------------------------------------
WCAL_HD void no_line(mkid_line_fit* f) {
    f->bin = -1, f->nfit = 0, f->peak_s = 0, f->counts = 0;
    f->mu = f->sigma = f->amp = nan64();
}

// (a0, a1, a2) of [S0 S1 S2; S1 S2 S3; S2 S3 S4] a = T by cofactor expansion along the first row of
// each determinant, in this written order.
struct Sums {   // named scalars, so that the fit's lane keeps them in registers
    double S0, S1, S2, S3, S4, T0, T1, T2;
};
struct Coef {
    double a0, a1, a2;
};
WCAL_HD Coef solve3(const Sums& q) {
    const double m00 = sub(mul(q.S2, q.S4), mul(q.S3, q.S3));
    const double m01 = sub(mul(q.S1, q.S4), mul(q.S3, q.S2));
    const double m02 = sub(mul(q.S1, q.S3), mul(q.S2, q.S2));
    const double det = add(sub(mul(q.S0, m00), mul(q.S1, m01)), mul(q.S2, m02));
    const double t14 = sub(mul(q.T1, q.S4), mul(q.S3, q.T2));
    const double t13 = sub(mul(q.T1, q.S3), mul(q.S2, q.T2));
    const double t12 = sub(mul(q.S1, q.T2), mul(q.T1, q.S2));
    const double t23 = sub(mul(q.S2, q.T2), mul(q.T1, q.S3));
    const double d0 = add(sub(mul(q.T0, m00), mul(q.S1, t14)), mul(q.S2, t13));
    const double d1 = add(sub(mul(q.S0, t14), mul(q.T0, m01)), mul(q.S2, t12));
    const double d2 = add(sub(mul(q.S0, t23), mul(q.S1, t12)), mul(q.T0, m02));
    return Coef{div(d0, det), div(d1, det), div(d2, det)};
}

// Line at bin m fitted over the window: the sums in ascending b, then the vertex.
WCAL_HD void fit_line(const int32_t* n, int32_t nbins, int32_t w, int32_t m, Window win, int32_t g, float lo, float step,
                      mkid_line_fit* f) {
    Sums q{0, 0, 0, 0, 0, 0, 0, 0};
    int64_t counts = 0;
    int32_t nfit = 0;
    for (int32_t b = win.b0; b <= win.b1; ++b) {
        const int64_t c = count(n, nbins, b);
        counts += c;
        if (c < 1) continue;
        ++nfit;
        const double x = (double)(b - m), y = log((double)c);
        const double w0 = mul((double)c, (double)c);
        const double w1 = mul(w0, x), w2 = mul(w1, x), w3 = mul(w2, x), w4 = mul(w3, x);
        q.S0 = add(q.S0, w0), q.S1 = add(q.S1, w1), q.S2 = add(q.S2, w2), q.S3 = add(q.S3, w3), q.S4 = add(q.S4, w4);
        q.T0 = add(q.T0, mul(w0, y)), q.T1 = add(q.T1, mul(w1, y)), q.T2 = add(q.T2, mul(w2, y));
    }
    f->bin = m, f->nfit = nfit, f->peak_s = smooth_at(n, nbins, w, m), f->counts = counts;
    f->mu = f->sigma = f->amp = nan64();
    if (nfit < 3) return;
    const Coef a = solve3(q);
    if (!(a.a2 < 0.0)) return;
    const double mu_x = div(-a.a1, mul(2.0, a.a2));
    const double sigma_x = sqrt(div(-1.0, mul(2.0, a.a2)));
    const double amp = exp(sub(a.a0, div(mul(a.a1, a.a1), mul(4.0, a.a2))));
    const double mu = add((double)lo, mul(add(add((double)m, 0.5), mu_x), (double)step));
    const double sigma = mul(sigma_x, fabs((double)step));
    if (!(__builtin_isfinite(mu_x) && __builtin_isfinite(sigma_x) && __builtin_isfinite(amp) && __builtin_isfinite(mu) &&
          __builtin_isfinite(sigma)) ||
        fabs(mu_x) > (double)g)
        return;
    f->mu = mu, f->sigma = sigma, f->amp = amp;
}

// ---- calibration --------------------------------------------------------------------------------
// E(h) = c0 + c1 h + c2 h^2 through the P points (mu_p, E_p), Newton's divided differences expanded
// in this written order; R_p = E_p / (kFwhm |dE/dh(mu_p)| sigma_p).
WCAL_HD void calibrate(const Params& pr, const mkid_line_fit* fits, int32_t found, mkid_energy_cal* cal, float* cal_f) {
    const int32_t P = pr.P;
    int32_t status = found < P ? MKID_CAL_FEW_LINES : 0;
    for (int32_t p = 0; p < found; ++p)
        if (!__builtin_isfinite(fits[p].mu)) status |= MKID_CAL_FIT_FAILED << p;
    double c[3] = {nan64(), nan64(), nan64()}, r[3] = {nan64(), nan64(), nan64()};
    if (status == 0) {
        const double* E = pr.E;
        const double m0 = fits[0].mu, m1 = P > 1 ? fits[1].mu : 0.0, m2 = P > 2 ? fits[2].mu : 0.0;
        if (P == 1) {
            c[0] = 0.0, c[1] = div(E[0], m0), c[2] = 0.0;
        } else if (P == 2) {
            c[1] = div(sub(E[1], E[0]), sub(m1, m0));
            c[0] = sub(E[0], mul(c[1], m0)), c[2] = 0.0;
        } else {
            const double f01 = div(sub(E[1], E[0]), sub(m1, m0)), f12 = div(sub(E[2], E[1]), sub(m2, m1));
            const double f012 = div(sub(f12, f01), sub(m2, m0));
            c[2] = f012;
            c[1] = sub(f01, mul(f012, add(m0, m1)));
            c[0] = add(sub(E[0], mul(m0, f01)), mul(f012, mul(m0, m1)));
        }
        double d[3] = {0, 0, 0};
        bool ok = true;
        for (int32_t p = 0; p < P; ++p) {
            d[p] = add(c[1], mul(mul(2.0, c[2]), fits[p].mu));
            ok = ok && __builtin_isfinite(d[p]) && d[p] != 0.0;
        }
        ok = ok && __builtin_isfinite(c[0]) && (d[0] > 0.0) == (d[P - 1] > 0.0);
        if (!ok) {
            status |= MKID_CAL_BAD_SLOPE;
            c[0] = c[1] = c[2] = nan64();
        } else {
            for (int32_t p = 0; p < P; ++p) r[p] = div(E[p], mul(mul(kFwhm, fabs(d[p])), fits[p].sigma));
        }
    }
    for (int32_t i = 0; i < 3; ++i) cal->c[i] = c[i], cal->r[i] = r[i];
    cal->n_found = found, cal->status = status;
    cal_f[0] = (float)c[0], cal_f[1] = (float)c[1], cal_f[2] = (float)c[2], cal_f[3] = status == 0 ? 1.0f : 0.0f;
}

// One channel on the host: selection, fits, calibration. The device kernel (k_wavecal.hip) runs the
// same steps with the candidate scan spread over a workgroup.
inline void lines_channel_host(const int32_t* n, float lo, float step, const Params& pr, mkid_line_fit* lines,
                               mkid_energy_cal* cal, float* cal_f) {
    int32_t chosen[kMaxLines], found = 0;
    for (int32_t r = 0; r < pr.P; ++r) {
        uint64_t best = 0;
        for (int32_t b = 0; b < pr.nbins; ++b) {
            if (excluded(b, chosen, r, pr.min_sep)) continue;
            const uint64_t k = candidate_key(n, pr.nbins, pr.w, pr.min_peak, b);
            if (k > best) best = k;
        }
        if (!best) break;
        chosen[found++] = key_bin(best);
    }
    sort_bins(chosen, found);
    for (int32_t p = 0; p < pr.P; ++p) {
        if (p < found)
            fit_line(n, pr.nbins, pr.w, chosen[p], window(chosen, found, p, pr.g, pr.nbins), pr.g, lo, step, &lines[p]);
        else
            no_line(&lines[p]);
    }
    calibrate(pr, lines, found, cal, cal_f);
}

inline void lines_host(const int32_t* spectra, const float* lo, const float* step, int32_t nch, const Params& pr,
                       mkid_line_fit* lines, mkid_energy_cal* cal, float* cal_f) {
    for (int32_t ch = 0; ch < nch; ++ch)
        lines_channel_host(spectra + (int64_t)ch * (pr.nbins + obs::kExtraCols) + 1, lo[ch], step[ch], pr,
                           lines + (int64_t)ch * pr.P, cal + ch, cal_f + (int64_t)ch * 4);
}

// ---- the energy cube ----------------------------------------------------------------------------
OBS_HD bool mode_ok(int32_t mode) { return mode == MKID_CUBE_ENERGY || mode == MKID_CUBE_WAVELENGTH; }

// e = c0 + h (c1 + h c2) in fp32, each operation rounded once; the one NaN of nan32() where the
// channel is not usable (cf[3] == 0), h is not finite, or the arithmetic gives no number.
WCAL_HD float energy(float h, const float* cf) {
    if (cf[3] == 0.f || !__builtin_isfinite(h)) return nan32();
    const float e = addf(cf[0], mulf(h, addf(cf[1], mulf(h, cf[2]))));
    return e != e ? nan32() : e;
}

// the binned value: e, or hc / e
WCAL_HD float cube_value(float e, int32_t mode, float hc) { return mode == MKID_CUBE_ENERGY ? e : divf(hc, e); }

struct CubeRule {
    int64_t j0, j_defer;
    int32_t C, nb, mode;
    float hc, vlo, vinv;
};

// Where packet (word, h) is counted: ch (nb + 3) + column, or -1 for a packet that touches no cell
// (ch >= C, or deferred); *e_out = its energy and *pixel = (ch < C).
WCAL_HD int64_t cube_cell(uint64_t word, float h, const float* cal_f, const CubeRule& r, float* e_out, bool* pixel) {
    const pkt::Stamp st = pkt::decode(word, r.j0);
    *pixel = st.ch < r.C;
    if (!*pixel) return -1;
    const float e = energy(h, cal_f + (int64_t)st.ch * 4);
    *e_out = e;
    if (obs::deferred(h, st.jg, r.j_defer)) return -1;
    return (int64_t)st.ch * (r.nb + obs::kExtraCols) + obs::column(cube_value(e, r.mode, r.hc), r.vlo, r.vinv, r.nb);
}

inline bool cube_args_ok(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int32_t C,
                         const float* cal_f, int32_t mode, int32_t nb, const int32_t* cube) {
    return cal_f && cube && (n == 0 || (events && heights)) && n >= 0 && j0 >= 0 && C >= 1 && C <= 4096 && mode_ok(mode) &&
           obs::bins_ok(nb);
}

inline void cube_host(const uint64_t* events, const float* heights, int64_t n, const float* cal_f, const CubeRule& r,
                      int32_t* cube, float* energy_out) {
    for (int64_t p = 0; p < n; ++p) {
        float e;
        bool pixel;
        const int64_t k = cube_cell(events[p], heights[p], cal_f, r, &e, &pixel);
        if (pixel && energy_out) obs::copy_bits(energy_out + p, &e);
        if (k >= 0) cube[k] = (int32_t)((uint32_t)cube[k] + 1u);
    }
}

}  // namespace wcal
}  // namespace mkid
