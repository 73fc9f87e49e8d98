// The phase-noise spectrum of a channel (ROACH_Pulses.py:521-543 longsnapshot; include/mkidgpu.h
// mkid_phase_noise_spectra states the rule), one definition for the kernel of k_noise.hip (float) and
// for the host entry point mkid_phase_noise_spectra_host (double): the offset taken off a piece, one
// output of one pass of the in-place mixed-radix transform, the unpacking of two real pieces carried
// as one complex piece, and the finish. Every index below is an integer computed the same way on
// both sides, so tools/plan_fuzz.cpp and tests/test_noise_host.py prove the index maps on the CPU.
//
// The transform of length n = r_0 r_1 ... r_{m-1} (plan::plan_noise, mkid_plan.h) is decimation in
// frequency, in place: pass s works on blocks of L = n / (r_0 ... r_{s-1}) elements, M = L / r_s.
// Output (b, t, j) of the pass, at position b L + t M + j, is
//     W_L^{j t} * sum_q x[b L + j + q M] W_r^{q t}          W_m = exp(-2 pi i / m)
// with W_r^{qt} from the pass's r-entry table at the exact index (q t) mod r and W_L^{jt} from the
// n-entry table at the exact index j t (n / L) < n. A pass reads r inputs per output and is computed
// "all outputs first, then all writes", so any radix, prime ones included, runs in place; the cost
// is n * sum of the radices. After the last pass position p holds bin k = bin_of_pos[p] (the
// mixed-radix digit reversal), which the plan tabulates together with partner[p], the position of
// bin (n - k) mod n.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NOISE_HD __host__ __device__ inline
#else
#define NOISE_HD inline
#endif

namespace mkid {
namespace noise {

constexpr int kMaxPasses = 14;   // n <= 2^14, every radix >= 2

template <class T>
struct Cx {
    T re, im;
};

// one pass: radix r on blocks of L elements, M = L / r, stride = n / L; its W_r table starts at
// entry tw_off of the radix tables
struct Pass {
    int32_t r, L, M, stride, tw_off;
};

// what a transform of length n reads: the passes and the tables (T = float on the device, double
// on the host)
template <class T>
struct View {
    int32_t n, npass;
    const Pass* pass;
    const Cx<T>* wn;              // [n]      W_n^i
    const Cx<T>* wr;              // [sum r]  W_r^i per pass, at Pass::tw_off
    const uint16_t* bin_of_pos;   // [n]
    const uint16_t* partner;      // [n]
};

// The integer nearest to sum / n (halves away from zero): the offset taken off every sample of a
// piece before the transform. Samples and offset are integers, so the subtraction is exact in
// either width and only bin 0 changes; bin 0 is then the integer sum itself. Without it a mean of
// 20 000 counts beside a noise of 5 would leave float32 rounding of the mean in every bin.
NOISE_HD int32_t round_mean(int32_t sum, int32_t n) {
    return sum >= 0 ? (sum + n / 2) / n : -((-sum + n / 2) / n);
}

template <class T>
NOISE_HD Cx<T> cmul(Cx<T> a, Cx<T> b) {
    return Cx<T>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// One output of pass `ps` at position p < n. x(i) reads element i of the piece, wr(i) entry i < r of
// the pass's radix table, wn(i) entry i < n of the n-entry table.
template <class T, class LoadX, class LoadWr, class LoadWn>
NOISE_HD Cx<T> pass_output(const Pass& ps, int32_t p, LoadX x, LoadWr wr, LoadWn wn) {
    const int32_t b = p / ps.L, rem = p - b * ps.L;
    const int32_t t = rem / ps.M, j = rem - t * ps.M;
    const int32_t base = b * ps.L + j;
    Cx<T> s = x(base);
    int32_t idx = 0;   // (q t) mod r
#if defined(__clang__)
#pragma unroll 4
#endif
    for (int32_t q = 1; q < ps.r; ++q) {
        idx += t;
        if (idx >= ps.r) idx -= ps.r;
        const Cx<T> v = x(base + q * ps.M), w = wr(idx);
        s.re += v.re * w.re - v.im * w.im;
        s.im += v.re * w.im + v.im * w.re;
    }
    const int32_t ti = j * t * ps.stride;   // j t < L, so ti < n
    return ti ? cmul(s, wn(ti)) : s;
}

// Two real pieces a and b carried as z = a + i b: with Z1 = Z[k] and Z2 = Z[(n - k) mod n],
// A[k] = (Z1 + conj Z2) / 2 and B[k] = (Z1 - conj Z2) / 2i. Returns |A[k]|^2 and |B[k]|^2.
template <class T>
NOISE_HD void unpack_power(Cx<T> z1, Cx<T> z2, T& pa, T& pb) {
    const T ar = z1.re + z2.re, ai = z1.im - z2.im;
    const T br = z1.re - z2.re, bi = z1.im + z2.im;
    pa = T(0.25) * (ar * ar + ai * ai);
    pb = T(0.25) * (br * br + bi * bi);
}

// |A[k]|^2 and |B[k]|^2 of the pair at one position. Bin 0 is the square of the piece's integer sum
// (sa, sb). A piece whose samples are all equal (flat_a, flat_b: the OR over the piece of
// x ^ x[0] is 0) has no power outside bin 0: that is said here, because what the other piece of
// the pair leaves of it after rounding is not zero; an all-zero piece so gives -inf in every bin.
template <class T>
NOISE_HD void bin_power(bool bin0, Cx<T> z1, Cx<T> z2, int32_t sa, int32_t sb, bool flat_a, bool flat_b, T& pa,
                        T& pb) {
    if (bin0) {
        pa = (T)sa * (T)sa, pb = (T)sb * (T)sb;
        return;
    }
    unpack_power(z1, z2, pa, pb);
    if (flat_a) pa = T(0);
    if (flat_b) pb = T(0);
}

// acc = sum over the pieces of log2 |X|^2; the spectrum is (10 log10 2 / n_averages) acc +
// 20 log10(scale / norm1 / 1e-6). mul and add are made once per call by the entry points.
NOISE_HD double finish(double acc, double mul, double add) {
    return acc * mul + add;
}

// The sequential statement of what a workgroup of k_noise.hip does with one pair of pieces (colB
// null: the unpaired last piece): the elements of the pieces are colA[j ld] and colB[j ld], j < n;
// z and y are n-element work arrays, log2 is the logarithm to use, and acc[p] gains
// log2 |A[k]|^2 (+ log2 |B[k]|^2), k = bin_of_pos[p], a before b.
template <class T, class Log2>
inline void pair_host(const View<T>& v, const int16_t* colA, const int16_t* colB, int64_t ld, Cx<T>* z, Cx<T>* y,
                      double* acc, Log2 log2) {
    const int32_t n = v.n;
    const int32_t fa = colA[0], fb = colB ? colB[0] : 0;
    int32_t sa = 0, sb = 0, va = 0, vb = 0;
    for (int32_t j = 0; j < n; ++j) {
        const int32_t xa = colA[(int64_t)j * ld], xb = colB ? colB[(int64_t)j * ld] : 0;
        sa += xa, sb += xb;
        va |= xa ^ fa, vb |= xb ^ fb;
        z[j] = Cx<T>{(T)xa, (T)xb};
    }
    const T oa = (T)round_mean(sa, n), ob = (T)round_mean(sb, n);
    for (int32_t j = 0; j < n; ++j) z[j].re -= oa, z[j].im -= ob;
    for (int32_t s = 0; s < v.npass; ++s) {
        const Pass ps = v.pass[s];
        const Cx<T>* wr = v.wr + ps.tw_off;
        for (int32_t p = 0; p < n; ++p)
            y[p] = pass_output<T>(
                ps, p, [z](int32_t i) { return z[i]; }, [wr](int32_t i) { return wr[i]; },
                [&v](int32_t i) { return v.wn[i]; });
        for (int32_t p = 0; p < n; ++p) z[p] = y[p];
    }
    for (int32_t p = 0; p < n; ++p) {
        T pa, pb;
        bin_power(v.bin_of_pos[p] == 0, z[p], z[v.partner[p]], sa, sb, va == 0, vb == 0, pa, pb);
        acc[p] += (double)log2(pa);
        if (colB) acc[p] += (double)log2(pb);
    }
}

}  // namespace noise
}  // namespace mkid
