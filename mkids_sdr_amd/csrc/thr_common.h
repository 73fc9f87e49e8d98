// The reference's threshold rule (ROACH_Pulses.py:211-299 loadThresholds; include/mkidgpu.h
// mkid_phase_thresholds states it), one definition for the kernels of k_thresholds.hip and for the
// host entry point mkid_phase_thresholds_host: the bin edges and integer cut points of a channel,
// the bin of a sample, numpy's prefix sums of the bin fractions, the two argmins and the threshold.
// Every float64 operation below is a single rounded IEEE operation in a fixed order (no fused
// multiply-add, no reassociation), so host and device give the same bits as numpy's float64 code.
#pragma once
#include <stdint.h>

#include "mkidgpu.h"

#if defined(__HIPCC__)
#define THR_HD __host__ __device__ inline
#else
#define THR_HD inline
#endif

namespace mkid {
namespace thr {

constexpr int kBins = 100;              // np.histogram(phase, bins=100)
constexpr int32_t kThrFloor = -25736;   // -pi in Fix16_13: the lowest threshold loaded

// The outer edges of a channel whose samples span lo..hi: a constant channel gets a unit-wide range
// around its value (numpy's _get_outer_edges).
struct Range {
    double lo, hi, step;
};
THR_HD Range make_range(int32_t lo, int32_t hi) {
    Range r{(double)lo, (double)hi, 0.0};
    if (lo == hi) r.lo -= 0.5, r.hi += 0.5;
    r.step = (r.hi - r.lo) / (double)kBins;
    return r;
}

// a b + c with the product rounded before the sum. hipcc contracts a * b + c into one fused
// multiply-add by default, on the device and on x86 hosts with FMA alike, and HIP's __dmul_rn /
// __dadd_rn are plain operators that contract just the same: contraction is switched off here.
THR_HD double mul_then_add(double a, double b, double c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = a * b;
    return p + c;
}
// Edge i of np.linspace(lo, hi, 101): arange(101) * step + lo with the last one replaced by hi.
THR_HD double edge(const Range& r, int i) { return i >= kBins ? r.hi : mul_then_add((double)i, r.step, r.lo); }

// Cut point i (1..99): the first integer >= edge i, so that for an integer sample x
// edge(i) <= x  <=>  cut(i) <= x. Edges lie in [-32768.5, 32767.5]: the result fits easily.
THR_HD int32_t cut(const Range& r, int i) {
    const double e = edge(r, i);
    const int32_t t = (int32_t)e;   // toward zero
    return (double)t < e ? t + 1 : t;
}

// The bin of sample x: the largest i <= 99 with edge(i) <= x, from the channel's cut table ct[0..100]
// with ct[0] <= every sample and ct[100] > every sample (the callers store INT32_MIN / INT32_MAX
// there), starting from any estimate b in 0..99.
THR_HD int bin_of(int32_t x, const int32_t* ct, int b) {
    while (x < ct[b]) --b;
    while (x >= ct[b + 1]) ++b;
    return b;
}

// Fraction of bin i: np.array(n, dtype='float32') / np.sum(n), a float32 array over an int64 scalar,
// which numpy 2 divides in float64.
THR_HD double fraction(uint32_t count, int64_t rows) { return (double)(float)count / (double)rows; }

// np.sum(n[:m]) for m <= 100 float64 values: numpy's pairwise sum below its 128-element block, i.e.
// sequential below 8 elements, else 8 accumulators over the multiple-of-8 prefix, combined as a
// tree, then the remainder (k_replay.hip pw_leaf is the same order on phase samples). n(i) gives
// element i.
template <class F>
THR_HD double prefix_sum(const F& n, int m) {
    if (m < 8) {
        double res = 0.0;
        for (int i = 0; i < m; ++i) res += n(i);
        return res;
    }
    double r0 = n(0), r1 = n(1), r2 = n(2), r3 = n(3), r4 = n(4), r5 = n(5), r6 = n(6), r7 = n(7);
    int i = 8;
    for (; i < m - (m % 8); i += 8) {
        r0 += n(i), r1 += n(i + 1), r2 += n(i + 2), r3 += n(i + 3);
        r4 += n(i + 4), r5 += n(i + 5), r6 += n(i + 6), r7 += n(i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < m; ++i) res += n(i);
    return res;
}

// First argmin of |tot - 0.5| and of |tot - 0.05| over a set of edge indices: the smallest distance,
// and among equal distances the smallest index (np.argmin). Distances are never NaN.
struct Pick {
    double d50, d05;
    int32_t i50, i05;
};
THR_HD Pick no_pick() { return Pick{2.0, 2.0, kBins + 1, kBins + 1}; }   // every distance is <= 1
THR_HD double absd(double v) { return v < 0.0 ? -v : v; }
THR_HD void pick_add(Pick& p, int i, double tot) {
    const double a = absd(tot - 0.5), b = absd(tot - 0.05);
    if (a < p.d50 || (a == p.d50 && i < p.i50)) p.d50 = a, p.i50 = i;
    if (b < p.d05 || (b == p.d05 && i < p.i05)) p.d05 = b, p.i05 = i;
}
THR_HD void pick_merge(Pick& p, const Pick& q) {
    if (q.d50 < p.d50 || (q.d50 == p.d50 && q.i50 < p.i50)) p.d50 = q.d50, p.i50 = q.i50;
    if (q.d05 < p.d05 || (q.d05 == p.d05 && q.i05 < p.i05)) p.d05 = q.d05, p.i05 = q.i05;
}
// the picks of edges i0, i0 + stride, ... <= 100
template <class F>
THR_HD Pick pick_scan(const F& n, int i0, int stride) {
    Pick p = no_pick();
    for (int i = i0; i <= kBins; i += stride) pick_add(p, i, prefix_sum(n, i));
    return p;
}

// The threshold from the picks over all 101 edges: int(-nsigma |med - p05|), truncated toward zero,
// at least -25736; nsigma is finite and >= 0, so the product is <= 0 and never NaN.
THR_HD int32_t finish(int32_t lo, int32_t hi, const Pick& p, double nsigma, mkid_thr_stats* st) {
    const Range r = make_range(lo, hi);
    const double med = edge(r, p.i50), p05 = edge(r, p.i05);
    const double v = -nsigma * absd(med - p05);
    if (st) st->med = med, st->p05 = p05, st->lo = lo, st->hi = hi;
    return v <= (double)kThrFloor ? kThrFloor : (int32_t)v;
}

}  // namespace thr
}  // namespace mkid
