// The pulse-height fit (include/mkidgpu.h mkid_pulse_fit states it), one definition for the kernel
// of k_heights_fit.hip and for the host entry point mkid_pulse_fit_host: the test that a packet's
// search window lies inside the rows (its channel and unwrapped stamp are pkt_common.h decode's),
// and the choice of the lag with the 3-point parabolic vertex around it. The vertex is the
// reference's peakfit (Utils/bin.py:12-16), y2 - (y3 - y1)^2 / (8 (y3 + y1 - 2 y2)), written with the
// two non-negative differences a = y2 - y1 and b = y2 - y3 so that the same terms give the vertex's
// position.
#pragma once
#include <stdint.h>

#include "mkidgpu.h"

#if defined(__HIPCC__)
#define FIT_HD __host__ __device__ inline
#else
#define FIT_HD inline
#endif

namespace mkid {
namespace fit {

constexpr int kMaxSearch = 31;   // the 2 L + 1 lags of a packet fit one wave
constexpr int kMaxCoeff = 4096;  // mkid_set_pulse_filter's bound

FIT_HD bool params_ok(int32_t search, int32_t polarity) {
    return search >= 0 && search <= kMaxSearch && (polarity == 1 || polarity == -1);
}

// Rows r0 - L .. r0 + L + ncoeff - 1 (relative to the call's first row) inside (hrows carried rows,
// rows) and a channel the context has.
FIT_HD bool inside(int32_t ch, int32_t C, int64_t r0, int32_t L, int32_t ncoeff, int64_t hrows, int64_t rows) {
    return ch < C && r0 - L >= -hrows && r0 + L + ncoeff <= rows;
}

template <typename T>
struct Result {
    T height, dt, h0;
    int32_t lag;
};

// H[0 .. 2 L] are the lag values of d = -L .. L. The lowest d that maximises s H[d] is chosen; at
// the edge of the search (always for L = 0) or on a flat top the value at that lag stands, else the
// vertex of the parabola through the three values around it: |dt - d*| <= 1/2.
template <typename T>
FIT_HD Result<T> select(const T* H, int32_t L, int32_t s) {
    const T sg = (T)s;
    int32_t k = 0;
    T y2 = sg * H[0];
    for (int32_t i = 1; i <= 2 * L; ++i) {
        const T y = sg * H[i];
        if (y > y2) y2 = y, k = i;
    }
    Result<T> r{H[k], (T)(k - L), H[L], k - L};
    if (k == 0 || k == 2 * L) return r;
    const T a = y2 - sg * H[k - 1], b = y2 - sg * H[k + 1], c = a + b;
    if (c == (T)0) return r;
    const T e = a - b;
    r.height = sg * (y2 + e * e / ((T)8 * c));
    r.dt = (T)(k - L) + e / ((T)2 * c);
    return r;
}

}  // namespace fit
}  // namespace mkid
