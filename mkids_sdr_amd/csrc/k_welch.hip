// mkid_welch_psd and mkid_iq_noise: Welch spectra of two real float64 series per channel
// (include/mkidgpu.h states the rules; every butterfly, index map and sum is welch_common.h's, which
// the host twins run too). The two series of a channel travel as the real and
// imaginary part of one complex float64 transform.
//
// k_welch_lds   nfft <= 4096. One workgroup of 512 threads per (channel, strip of 32 segments). Per
//               segment it loads the windowed samples into LDS (16 B an element, at most 64 KiB),
//               runs the in-place passes (a thread takes butterflies tid, tid + 512, ..: a butterfly
//               writes where it read, so one barrier a pass), and thread t adds |A[k]|^2, |B[k]|^2
//               of bins k = t, t + 512, .. to the strip sums it keeps in registers. The end writes
//               the strip's sums to the workspace. Nothing is accumulated in memory.
// k_welch_cols  nfft > 4096 = n1 n2, step 1 and 2 for one segment of every (channel, strip): a
// k_welch_rows  workgroup loads a tile of 4096 / n1 adjacent columns (runs of 4096 / n1 samples from
//               each of n1 rows) into LDS, transforms them over j1, multiplies by W_nfft^{j2 k1} and
//               writes Y[k1][j2] to the workspace. Step 3: a workgroup loads rows k1 and n1 - k1 of Y
//               (16 KiB at most), transforms both over j2, and since bin nfft - k of row k1 lies in row
//               n1 - k1 takes the powers of both rows' bins k <= nfft / 2 from the pair and adds
//               them to the strip sums in the workspace: one thread per bin, the launches of a
//               strip's segments in stream order, so the order of the sum is the segments'.
// k_welch_finish  adds a channel's strip sums in ascending order and writes the densities.
// k_iq_means, k_iq_fn1k  the head and tail of mkid_iq_noise: exact int64 sums and the channel's
//               constants; the fn1k line, and NaN over the spectra of a channel with an unusable rad.
// No floating-point atomics anywhere; every index is bounded by the launch geometry below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "mkid_internal.h"
#include "welch_common.h"

namespace mkid {
namespace {

using welch::Cx;
constexpr int kT = 512;                                       // k_welch_lds, k_welch_cols
constexpr int kPer = (welch::kLdsMaxN / 2 + kT) / kT;         // bins tid + i kT <= nfft / 2 of a thread
constexpr int kColElems = 4096;                               // LDS elements of a column tile
constexpr int kRowT = 256;                                    // k_welch_rows, k_welch_finish, k_iq_means
constexpr int kLdsBytes = welch::kLdsMaxN * (int)sizeof(Cx);  // 64 KiB
static_assert(kColElems * sizeof(Cx) <= (size_t)kLdsBytes, "column tile");

struct TwTab {
    const Cx* p;
    __device__ Cx operator()(int32_t i) const { return p[i]; }
};
struct LdsZ {
    Cx* p;
    __device__ Cx& operator()(int32_t i) const { return p[i]; }
};
struct LdsStrided {   // element i of the column at p: a tile's columns are interleaved
    Cx* p;
    int32_t stride;
    __device__ Cx& operator()(int32_t i) const { return p[i * stride]; }
};

template <bool IQ>
struct Src;
template <>
struct Src<false> {
    static __device__ welch::RowLoader make(const WelchArgs& a, int64_t c) {
        return welch::RowLoader{a.a + c * a.ld, a.b ? a.b + c * a.ld : nullptr};
    }
};
template <>
struct Src<true> {
    static __device__ welch::IqLoader make(const WelchArgs& a, int64_t c) {
        return welch::IqLoader(a.xi + c * a.ld, a.xq + c * a.ld, a.cfg, a.i0[c], a.q0[c], a.icen[c], a.qcen[c], a.res[c]);
    }
};

// the strip sums of (channel cl of the group, strip): [2][half + 1]
__device__ double* strip_sums(const WelchArgs& a, int32_t cl, int64_t strip) {
    return a.part + ((int64_t)cl * a.nstrips + strip) * 2 * (a.nfft / 2 + 1);
}

template <bool IQ>
__global__ __launch_bounds__(kT) void k_welch_lds(const WelchArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    Cx* z = (Cx*)s_dyn;   // [nfft]
    const int tid = threadIdx.x;
    const int32_t n = a.nfft, half = n / 2;
    const int64_t strip = blockIdx.x;
    const int32_t cl = blockIdx.y;
    const auto ld = Src<IQ>::make(a, a.c0 + cl);
    const welch::Plan p = welch::make_plan(n);
    const TwTab tw{(const Cx*)a.tw};
    double sa[kPer], sb[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) sa[i] = 0.0, sb[i] = 0.0;
    const int64_t s_end = std::min<int64_t>(a.nseg, (strip + 1) * welch::kStrip);
    for (int64_t s = strip * welch::kStrip; s < s_end; ++s) {
        const int64_t base = s * half;
        for (int32_t j = tid; j < n; j += kT) z[j] = welch::windowed(ld(base + j), a.w[j]);
        __syncthreads();
        int32_t L = n;
        for (int32_t ps = 0; ps < p.npass; ++ps) {
            const int32_t r = welch::radix(p, ps);
            for (int32_t u = tid; u < n / r; u += kT) welch::butterfly(r, L, u, n / L, LdsZ{z}, tw);
            __syncthreads();
            L /= r;
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int32_t k = tid + i * kT;
            if (k <= half) {
                double pa, pb;
                welch::unpack_power(z[welch::pos_of_bin(p, k)], z[welch::pos_of_bin(p, (n - k) & (n - 1))], pa, pb);
                sa[i] = welch::add(sa[i], pa), sb[i] = welch::add(sb[i], pb);
            }
        }
        __syncthreads();   // the next segment overwrites z
    }
    double* pt = strip_sums(a, cl, strip);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int32_t k = tid + i * kT;
        if (k <= half) pt[k] = sa[i], pt[half + 1 + k] = sb[i];
    }
}

// segment iseg of every strip: the column transforms and the twiddle; grid (n2 / cw, nstrips, g)
template <bool IQ>
__global__ __launch_bounds__(kT) void k_welch_cols(const WelchArgs a, int32_t iseg) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    Cx* z = (Cx*)s_dyn;   // [n1][cw]
    const int tid = threadIdx.x;
    const int64_t strip = blockIdx.y, s = strip * welch::kStrip + iseg;
    if (s >= a.nseg) return;   // the whole workgroup: the last strip may be short
    const int32_t cl = blockIdx.z;
    int32_t n1, n2;
    welch::split(a.nfft, n1, n2);
    const int32_t cw = kColElems / n1, col0 = blockIdx.x * cw;
    const auto ld = Src<IQ>::make(a, a.c0 + cl);
    const welch::Plan p = welch::make_plan(n1);
    const TwTab tw{(const Cx*)a.tw};
    const int64_t base = s * (a.nfft / 2);
    for (int32_t idx = tid; idx < kColElems; idx += kT) {
        const int32_t j1 = idx / cw, j = n2 * j1 + col0 + (idx - j1 * cw);
        z[idx] = welch::windowed(ld(base + j), a.w[j]);
    }
    __syncthreads();
    int32_t L = n1;
    for (int32_t ps = 0; ps < p.npass; ++ps) {
        const int32_t r = welch::radix(p, ps);
        for (int32_t idx = tid; idx < kColElems / r; idx += kT) {
            const int32_t u = idx / cw;
            welch::butterfly(r, L, u, a.nfft / L, LdsStrided{z + (idx - u * cw), cw}, tw);
        }
        __syncthreads();
        L /= r;
    }
    Cx* y = (Cx*)a.y + ((int64_t)cl * a.nstrips + strip) * a.nfft;
    for (int32_t idx = tid; idx < kColElems; idx += kT) {
        const int32_t k1 = idx / cw, cj = idx - k1 * cw, j2 = col0 + cj;
        y[(int64_t)k1 * n2 + j2] = welch::step_twiddle(z[welch::pos_of_bin(p, k1) * cw + cj], j2 * k1, tw);
    }
}

// segment iseg of every strip: rows k1 and n1 - k1, their powers into the strip sums; grid
// (n1 / 2 + 1, nstrips, g)
__global__ __launch_bounds__(kRowT) void k_welch_rows(const WelchArgs a, int32_t iseg) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int tid = threadIdx.x;
    const int64_t strip = blockIdx.y;
    if (strip * welch::kStrip + iseg >= a.nseg) return;   // the whole workgroup
    const int32_t cl = blockIdx.z;
    int32_t n1, n2;
    welch::split(a.nfft, n1, n2);
    const int32_t k1 = blockIdx.x, kb = n1 - k1, half = a.nfft / 2, hn2 = n2 / 2;
    const bool self = k1 == 0 || 2 * k1 == n1;   // the row is its own partner
    Cx* A = (Cx*)s_dyn;                          // [n2] row k1
    Cx* B = self ? A : A + n2;                   // [n2] row n1 - k1
    const Cx* y = (const Cx*)a.y + ((int64_t)cl * a.nstrips + strip) * a.nfft;
    for (int32_t j = tid; j < n2; j += kRowT) {
        A[j] = y[(int64_t)k1 * n2 + j];
        if (!self) B[j] = y[(int64_t)kb * n2 + j];
    }
    __syncthreads();
    const welch::Plan p = welch::make_plan(n2);
    const TwTab tw{(const Cx*)a.tw};
    int32_t L = n2;
    for (int32_t ps = 0; ps < p.npass; ++ps) {
        const int32_t r = welch::radix(p, ps), nb = n2 / r;
        for (int32_t idx = tid; idx < (self ? nb : 2 * nb); idx += kRowT)
            welch::butterfly(r, L, idx < nb ? idx : idx - nb, a.nfft / L, LdsZ{idx < nb ? A : B}, tw);
        __syncthreads();
        L /= r;
    }
    double* pt = strip_sums(a, cl, strip);
    const bool first = iseg == 0;   // a strip's sum starts from 0.0
    auto gain = [&](int32_t k, Cx z1, Cx z2) {
        double pa, pb;
        welch::unpack_power(z1, z2, pa, pb);
        pt[k] = welch::add(first ? 0.0 : pt[k], pa);
        pt[half + 1 + k] = welch::add(first ? 0.0 : pt[half + 1 + k], pb);
    };
    if (k1 == 0) {   // bins n1 k2, k2 <= n2 / 2; the partner (n2 - k2) mod n2 is in the row
        for (int32_t k2 = tid; k2 <= hn2; k2 += kRowT)
            gain(n1 * k2, A[welch::pos_of_bin(p, k2)], A[welch::pos_of_bin(p, (n2 - k2) & (n2 - 1))]);
    } else {         // bins k1 + n1 k2 and (n1 - k1) + n1 k2, k2 < n2 / 2; the partners at n2 - 1 - k2
        for (int32_t k2 = tid; k2 < hn2; k2 += kRowT) {
            const int32_t pk = welch::pos_of_bin(p, k2), pp = welch::pos_of_bin(p, n2 - 1 - k2);
            gain(k1 + n1 * k2, A[pk], B[pp]);
            if (!self) gain(kb + n1 * k2, B[pk], A[pp]);
        }
    }
}

// grid (ceil((k_hi - k_lo) / kRowT), g)
__global__ __launch_bounds__(kRowT) void k_welch_finish(const WelchArgs a) {
    const int32_t k = a.k_lo + blockIdx.x * kRowT + threadIdx.x, cl = blockIdx.y, half = a.nfft / 2;
    if (k >= a.k_hi) return;
    double ta = 0.0, tb = 0.0;
    for (int64_t st = 0; st < a.nstrips; ++st) {
        const double* pt = strip_sums(a, cl, st);
        ta = welch::add(ta, pt[k]), tb = welch::add(tb, pt[half + 1 + k]);
    }
    const int64_t o = (int64_t)(a.c0 + cl) * a.ldo + a.off + (k - a.k_lo);
    a.out_a[o] = welch::density(ta, (double)a.nseg, a.den, k, half);
    if (a.out_b) a.out_b[o] = welch::density(tb, (double)a.nseg, a.den, k, half);
}

__global__ __launch_bounds__(kRowT) void k_iq_means(const IqNoiseArgs a) {
    __shared__ long long s_red[2 * (kRowT / 64)];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int16_t *xi = a.xi + c * a.ld, *xq = a.xq + c * a.ld;
    long long si = 0, sq = 0;
    for (int64_t j = tid; j < a.n; j += kRowT) si += xi[j], sq += xq[j];
    for (int o = 32; o > 0; o >>= 1) si += __shfl_xor(si, o, 64), sq += __shfl_xor(sq, o, 64);
    if ((tid & 63) == 0) s_red[2 * (tid >> 6)] = si, s_red[2 * (tid >> 6) + 1] = sq;
    __syncthreads();
    if (tid == 0) {
        si = 0, sq = 0;
        for (int w = 0; w < kRowT / 64; ++w) si += s_red[2 * w], sq += s_red[2 * w + 1];
        welch::iq_means(si, sq, a.n, a.cfg, a.i0[c], a.q0[c], a.icen[c], a.qcen[c], a.qfit[c], &a.res[c]);
    }
}

__global__ __launch_bounds__(64) void k_iq_fn1k(const IqNoiseArgs a) {
    const int64_t c = blockIdx.x;
    const int32_t nout = welch::iq_nout(a.cfg), st = a.res[c].status;
    double* pn = a.pn + c * nout;
    double* an = a.an + c * nout;
    if (st & MKID_IQN_BAD_RAD)
        for (int32_t b = threadIdx.x; b < nout; b += 64) pn[b] = welch::nan64(), an[b] = welch::nan64();
    if (threadIdx.x == 0) a.res[c].fn1k = welch::iq_fn1k(a.cfg, pn, a.qfit[c], st);   // reads no NaN-filled row
}

template <bool IQ>
hipError_t launch_segments(const WelchArgs& a, hipStream_t s) {
    static std::atomic<uint64_t> lds_direct{0}, lds_cols{0};
    if (!welch::four_step(a.nfft)) {
        hipError_t e = ensure_lds_attr(lds_direct, (const void*)k_welch_lds<IQ>, kLdsBytes);
        if (e != hipSuccess) return e;
        k_welch_lds<IQ><<<dim3((unsigned)a.nstrips, (unsigned)a.g), dim3(kT), (size_t)a.nfft * sizeof(Cx), s>>>(a);
        return hipGetLastError();
    }
    hipError_t e = ensure_lds_attr(lds_cols, (const void*)k_welch_cols<IQ>, kLdsBytes);
    if (e != hipSuccess) return e;
    int32_t n1, n2;
    welch::split(a.nfft, n1, n2);
    const int32_t cw = kColElems / n1;
    if (n1 > kColElems || n2 % cw != 0 || n2 > welch::kLdsMaxN) return hipErrorInvalidValue;
    const int32_t in_strip = (int32_t)std::min<int64_t>(a.nseg, welch::kStrip);
    for (int32_t i = 0; i < in_strip; ++i) {
        k_welch_cols<IQ><<<dim3((unsigned)(n2 / cw), (unsigned)a.nstrips, (unsigned)a.g), dim3(kT),
                           kColElems * sizeof(Cx), s>>>(a, i);
        k_welch_rows<<<dim3((unsigned)(n1 / 2 + 1), (unsigned)a.nstrips, (unsigned)a.g), dim3(kRowT),
                       2 * (size_t)n2 * sizeof(Cx), s>>>(a, i);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_welch_group(const WelchArgs& a, hipStream_t s) {
    if (!welch::pow2(a.nfft) || a.nfft < 8 || a.nfft > welch::kMaxN || a.g < 1 || a.g > 65535 || a.nseg < 1 ||
        a.nstrips != welch::strips(a.nseg) || (welch::four_step(a.nfft) && (a.nstrips > 65535 || !a.y)) || !a.part ||
        a.k_lo < 0 || a.k_hi > a.nfft / 2 + 1 || a.k_lo >= a.k_hi)
        return hipErrorInvalidValue;
    hipError_t e = a.xi ? launch_segments<true>(a, s) : launch_segments<false>(a, s);
    if (e != hipSuccess) return e;
    k_welch_finish<<<dim3((unsigned)((a.k_hi - a.k_lo + kRowT - 1) / kRowT), (unsigned)a.g), dim3(kRowT), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_iq_means(const IqNoiseArgs& a, hipStream_t s) {
    if (a.nch < 1) return hipErrorInvalidValue;
    k_iq_means<<<dim3((unsigned)a.nch), dim3(kRowT), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_iq_fn1k(const IqNoiseArgs& a, hipStream_t s) {
    if (a.nch < 1) return hipErrorInvalidValue;
    k_iq_fn1k<<<dim3((unsigned)a.nch), dim3(64), 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace mkid
