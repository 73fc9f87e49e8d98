// MakeTemplate (DataReadout/ReadoutControls/lib/pulses.py:239-427) and the
// near-optimal filter it stubs (pulses.py:398; PulseAnalysis.coeff, pulses.py:59), on device.
//
// The reference loops over one resonator's pulses (I, Q float32 [P][2000]) twice in Python; here
// every pulse is one 256-thread workgroup:
//   prep     I += I1m - median(I[1:900]) (in place: the reference edits its table, so the first
//            1000 pulses are re-referenced again in pass 2), P1 = atan2(Q, I) (float32), numpy
//            unwrap (float32, sequential cumsum), rad2deg, linear polyfit over [0:900]+[1800:]
//            (float64), P3 = P2 - fit, bad = |mean(P3[:100]) - mean(P3[1900:])| > 2 std(P3[:100])
//   pass 1   peak = max P3[980:1050]; 15..120 deg; ploc (first index == peak) in 980..1020;
//            row = roll(P3, 1000 - ploc) / max
//   pass 2   ploc = argmax(convolve(tP[900:1500], P3)) - 1160, peak = P3[1000 + ploc] within
//            pm +- 4 pdev, |ploc| <= 30; row = roll(P3, -ploc) / max; noise row =
//            |DFT800(deg2rad(row-before-normalisation[50:850]))|^2
// Accumulations over pulses run column-parallel in pulse order (the reference's += order), the
// medians are exact order statistics (workgroup radix select), pm / pdev / std / mean follow
// numpy's pairwise float64 summation. Results agree with oracle/template_ref.py to float rounding
// (atan2f and the least-squares fit differ in the last bits), and every accept/skip decision away
// from a threshold is identical (tests/test_template.py, tests/test_gpu_template.py).
//
// Every stage is one device function and runs in one set of kernels, k_bank_*: a group of channels of
// a record bank per launch, every scalar (I1m/Q1m, pm/pdev, the counts, both status decisions) in
// device tables, I/Q or phase records read where they lie and never written. mkid_bank_filters
// launches them over a caller's bank; mkid_make_template is the same launch on one channel whose
// records are all ready (g = 1, R = ready = P, no filter), so a channel of a bank and the same
// records run alone give the same bits by construction. mkid_optimal_filter (k_tpl_optfilt) is the
// filter stage alone. DESIGN.md §5.7 has the launches and the workspace layout.
#include "mkid_internal.h"

namespace mkid {

constexpr int kTN = 2000;   // samples per pulse (RawPulse.I, pulses.py:42)
constexpr int kTNoise = 800;
constexpr int kTB = 256;

__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fval(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// k-th smallest (0-based) of get(0..n-1), exact, by the whole workgroup (4 radix-8 passes)
template <typename G>
__device__ float wg_select(G get, int n, int k) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_k;
    uint32_t prefix = 0, mask = 0;
    if (threadIdx.x == 0) s_k = (uint32_t)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const uint32_t key = fkey(get(i));
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t kk = s_k, cum = 0, sel = 255;
            for (int b = 0; b < 256; ++b) {
                if (cum + hist[b] > kk) { sel = (uint32_t)b; break; }
                cum += hist[b];
            }
            s_k = kk - cum;
            s_prefix = prefix | (sel << shift);
        }
        __syncthreads();
        prefix = s_prefix;
        mask |= 255u << shift;
        __syncthreads();
    }
    return fval(prefix);
}

// np.median of float32 data: middle element, or the float32 mean of the two middle elements
template <typename G>
__device__ float wg_median(G get, int n) {
    if (n & 1) return wg_select(get, n, n / 2);
    const float a = wg_select(get, n, n / 2 - 1);
    const float b = wg_select(get, n, n / 2);
    return (a + b) / 2.0f;
}

// numpy pairwise_sum over a double array (loops_utils.h.src), n <= 128 leaf / halving
__device__ double pw_leaf_d(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
__device__ double pw_sum_d(const double* a, int n) {
    if (n <= 128) return pw_leaf_d(a, n);
    // recursion n -> (n2 = n/2 - (n/2)%8, n - n2), unrolled with an explicit stack
    struct Fr { int o, n, state; double left; };
    Fr st[20];
    int sp = 0;
    st[0] = Fr{0, n, 0, 0.0};
    double ret = 0.0;
    while (sp >= 0) {
        Fr& f = st[sp];
        if (f.n <= 128) { ret = pw_leaf_d(a + f.o, f.n); --sp; continue; }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) { f.state = 1; st[sp + 1] = Fr{f.o, n2, 0, 0.0}; ++sp; }
        else if (f.state == 1) { f.left = ret; f.state = 2; st[sp + 1] = Fr{f.o + n2, f.n - n2, 0, 0.0}; ++sp; }
        else { ret = f.left + ret; --sp; }
    }
    return ret;
}
__device__ double np_mean(const double* a, int n) { return pw_sum_d(a, n) / (double)n; }
// np.std: sqrt(mean(abs(x - mean(x))**2)); tmp is scratch of n doubles
__device__ double np_std(const double* a, int n, double* tmp) {
    const double m = np_mean(a, n);
    for (int i = 0; i < n; ++i) {
        const double d = fabs(a[i] - m);
        tmp[i] = d * d;
    }
    return sqrt(pw_sum_d(tmp, n) / (double)n);
}

// numpy float mod (npy_divmodf): sign of the divisor
__device__ __forceinline__ float np_modf(float a, float b) {
    float m = fmodf(a, b);
    if (m != 0.0f) {
        if ((b < 0.0f) != (m < 0.0f)) m += b;
    } else {
        m = copysignf(0.0f, b);
    }
    return m;
}

// Workgroup reductions of kTB threads through one scratch pair per kernel. Each returns its result
// to every thread, with the scratch free for the next one.
struct WgRed {
    double v[kTB];
    int i[kTB];
};
__device__ __forceinline__ WgRed& wg_red() {
    __shared__ WgRed r;
    return r;
}
template <typename T, typename Op>
__device__ __forceinline__ T wg_reduce(T* red, T v, Op op) {
    const int t0 = threadIdx.x;
    red[t0] = v;
    __syncthreads();
    for (int o = kTB / 2; o > 0; o >>= 1) { if (t0 < o) red[t0] = op(red[t0], red[t0 + o]); __syncthreads(); }
    const T r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double wg_sum(double v) {
    return wg_reduce(wg_red().v, v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ double wg_max(double v) {
    return wg_reduce(wg_red().v, v, [](double a, double b) { return fmax(a, b); });
}
__device__ __forceinline__ int wg_argmin(int i) {
    return wg_reduce(wg_red().i, i, [](int a, int b) { return min(a, b); });
}
// index of the largest v, the smallest index among equals
__device__ __forceinline__ int wg_argmax_first(double v, int i) {
    double* red = wg_red().v;
    int* redi = wg_red().i;
    const int t0 = threadIdx.x;
    red[t0] = v;
    redi[t0] = i;
    __syncthreads();
    for (int o = kTB / 2; o > 0; o >>= 1) {
        if (t0 < o && (red[t0 + o] > red[t0] || (red[t0 + o] == red[t0] && redi[t0 + o] < redi[t0]))) {
            red[t0] = red[t0 + o];
            redi[t0] = redi[t0 + o];
        }
        __syncthreads();
    }
    const int r = redi[0];
    __syncthreads();
    return r;
}

// The direct 800-point DFT in float64: tw[k] = exp(-2 pi i k / 800) by the whole workgroup (the
// caller synchronises), and one row's walk, term(n, tw[n f mod 800]) for n = 0..799 in that order.
__device__ __forceinline__ void dft_twiddles(double* twr, double* twi) {
    for (int k = threadIdx.x; k < kTNoise; k += kTB) {
        double sn, cs;
        sincospi(-2.0 * k / kTNoise, &sn, &cs);
        twr[k] = cs;
        twi[k] = sn;
    }
}
template <typename F>
__device__ __forceinline__ void dft_row(int f, const double* twr, const double* twi, F term) {
    int ph = 0;
    for (int n = 0; n < kTNoise; ++n) {
        term(n, twr[ph], twi[ph]);
        ph += f;
        if (ph >= kTNoise) ph -= kTNoise;
    }
}

// One pulse as its workgroup sees it: the scalars of its set and its own slots of the set's tables.
struct TplPulse {
    float I1m, Q1m;
    const double* tP;    // pass-1 template (pass 2)
    double pm, pdev;     // pass-1 peak statistics (pass 2)
    double* row;         // [2000]
    double* nrow;        // [800] (pass 2)
    int32_t* accept;
    double* peak;        // pass 1
    int32_t* appended;   // pass 1
    int pass;
    int nref;            // re-references before the phase: 1, or 2 where pass 2 meets a pulse that
                         // pass 1 re-referenced already and whose source was left as it was
};

// I = cos(sign phi), Q = sin(sign phi), float32: template.iq_from_phase on the device
__device__ __forceinline__ void phase_iq(float sign, float phi, float& i, float& q) {
    const float a = sign * phi;
    i = cosf(a);
    q = sinf(a);
}
// Where a pulse's samples come from: the caller's record, I/Q or phase, read only.
struct SrcBank {
    const float* I;      // this pulse's record: I, or phase (rad) where Q is null
    const float* Q;
    float sign;
    __device__ __forceinline__ void load(int t, float& i, float& q) const {
        if (Q) { i = I[t]; q = Q[t]; }
        else phase_iq(sign, I[t], i, q);
    }
};

// One pulse: prep (re-reference, phase, unwrap, baseline) then the pass's selection.
__device__ __forceinline__ void tpl_pulse(const SrcBank src, const TplPulse a) {
    __shared__ float sI[kTN], sQ[kTN], sP2[kTN];
    __shared__ double sP3[kTN];
    __shared__ double sA[600];
    __shared__ double s_fit[2];
    __shared__ int s_bad;
    const int t0 = threadIdx.x;
    for (int t = t0; t < kTN; t += kTB) src.load(t, sI[t], sQ[t]);
    __syncthreads();
    for (int r = 0; r < a.nref; ++r) {
        // I += I1m - median(I[1:900]) (float32)
        const float mI = wg_median([&](int i) { return sI[1 + i]; }, 899);
        const float mQ = wg_median([&](int i) { return sQ[1 + i]; }, 899);
        const float dI = a.I1m - mI, dQ = a.Q1m - mQ;
        for (int t = t0; t < kTN; t += kTB) {
            sI[t] += dI;
            sQ[t] += dQ;
            sP2[t] = atan2f(sQ[t] - 0.0f, sI[t] - 0.0f);  // P1 (xc = yc = 0, pulses.py:274-275)
        }
        __syncthreads();
    }
    // np.unwrap (float32: period 2pi, discont pi) + rad2deg, sequential like the reference's cumsum
    if (t0 == 0) {
        const float hi = 3.14159265358979311600f, per = 6.28318530717958623200f;
        const float r2d = 180.0f / 3.14159265358979311600f;  // numpy float32 rad2deg: 180.0f/NPY_PIf
        float cum = 0.0f, prev = sP2[0];
        sP2[0] = sP2[0] * r2d;
        for (int t = 1; t < kTN; ++t) {
            const float p = sP2[t];
            const float dd = p - prev;
            float ddmod = np_modf(dd - (-hi), per) + (-hi);
            if (ddmod == -hi && dd > 0.0f) ddmod = hi;
            float corr = ddmod - dd;
            if (fabsf(dd) < hi) corr = 0.0f;
            cum += corr;
            prev = p;
            sP2[t] = (p + cum) * r2d;
        }
    }
    __syncthreads();
    // linear least squares of P2 on x = 2t over t in [0,900) u [1800,2000)  (polyfit deg 1)
    {
        double sx = 0, sy = 0;
        for (int t = t0; t < kTN; t += kTB)
            if (t < 900 || t >= 1800) { sx += 2.0 * t; sy += (double)sP2[t]; }
        const double xm = wg_sum(sx) / 1100.0;
        const double ym = wg_sum(sy) / 1100.0;
        double sxy = 0, sxx = 0;
        for (int t = t0; t < kTN; t += kTB)
            if (t < 900 || t >= 1800) {
                const double dx = 2.0 * t - xm;
                sxy += dx * ((double)sP2[t] - ym);
                sxx += dx * dx;
            }
        const double cxy = wg_sum(sxy);
        const double cxx = wg_sum(sxx);
        if (t0 == 0) {
            s_fit[0] = cxy / cxx;
            s_fit[1] = ym - s_fit[0] * xm;
        }
        __syncthreads();
    }
    for (int t = t0; t < kTN; t += kTB) sP3[t] = (double)sP2[t] - (s_fit[0] * (2.0 * t) + s_fit[1]);
    __syncthreads();
    if (t0 == 0) {
        double* tmp = sA;  // scratch (100 doubles)
        const double sd = np_std(sP3, 100, tmp);
        s_bad = fabs(np_mean(sP3, 100) - np_mean(sP3 + 1900, 100)) > sd * 2.0;
    }
    __syncthreads();
    if (s_bad) {
        if (t0 == 0) {
            *a.accept = 0;
            if (a.pass == 1) *a.appended = 0;
        }
        return;
    }
    // max over all of P3 (normalisation) and the pass's peak search
    double mx = -INFINITY;
    for (int t = t0; t < kTN; t += kTB) mx = fmax(mx, sP3[t]);
    const double pmax = wg_max(mx);
    int shift = 0;
    bool ok = true;
    if (a.pass == 1) {
        double pk = -INFINITY;
        for (int t = 980 + t0; t < 1050; t += kTB) pk = fmax(pk, sP3[t]);
        const double peak = wg_max(pk);
        int first = kTN;
        for (int t = t0; t < kTN; t += kTB)
            if (sP3[t] == peak && t < first) first = t;
        const int ploc = wg_argmin(first);
        if (t0 == 0) { *a.peak = peak; *a.appended = 1; }
        ok = !(peak < 15.0 || peak > 120.0) && !(ploc < 980 || ploc > 1020);
        shift = 1000 - ploc;
    } else {
        // conv[n] = sum_k tP[900+k] P3[n-k], n in [0, 2599); first argmax
        for (int k = t0; k < 600; k += kTB) sA[k] = a.tP[900 + k];
        __syncthreads();
        double best = -INFINITY;
        int bi = 1 << 30;
        for (int n = t0; n < 2599; n += kTB) {
            const int klo = n - (kTN - 1) > 0 ? n - (kTN - 1) : 0, khi = n < 599 ? n : 599;
            double s = 0.0;
            for (int k = klo; k <= khi; ++k) s += sA[k] * sP3[n - k];
            if (s > best) { best = s; bi = n; }
        }
        const int ploc = wg_argmax_first(best, bi) - 1160;
        int pi = 1000 + ploc;
        if (pi < 0) pi += kTN;  // numpy negative index
        const bool inr = pi >= 0 && pi < kTN;  // out of range: the reference raises; skipped here
        const double peak = inr ? sP3[pi] : 0.0;
        ok = inr && !(peak < a.pm - 4.0 * a.pdev || peak > a.pm + 4.0 * a.pdev) && !(ploc < -30 || ploc > 30);
        shift = -ploc;
    }
    if (t0 == 0) *a.accept = ok ? 1 : 0;
    if (!ok) return;
    // row = roll(P3, shift) / max(P3)
    double* row = a.row;
    for (int t = t0; t < kTN; t += kTB) {
        int src = t - shift;
        src %= kTN;
        if (src < 0) src += kTN;
        row[t] = sP3[src] / pmax;
    }
    if (a.pass == 2) {
        // |DFT800(deg2rad(roll(P3)[50:850]))|^2, direct in float64 with a twiddle table in the
        // (now free) sI/sQ space
        __syncthreads();
        __shared__ double win[kTNoise];
        double* twr = reinterpret_cast<double*>(sI);  // 800 doubles = 6400 B <= 8000 B
        double* twi = reinterpret_cast<double*>(sQ);
        dft_twiddles(twr, twi);
        for (int t = t0; t < kTNoise; t += kTB) {
            int src = 50 + t - shift;
            src %= kTN;
            if (src < 0) src += kTN;
            win[t] = sP3[src] * 0.017453292519943295;
        }
        __syncthreads();
        double* nrow = a.nrow;
        for (int f = t0; f < kTNoise; f += kTB) {
            double re = 0.0, im = 0.0;
            dft_row(f, twr, twi, [&](int n, double c, double s) {
                re += win[n] * c;
                im += win[n] * s;
            });
            nrow[f] = re * re + im * im;
        }
    }
}

// column sums over accepted rows in pulse order; out[t] = sum / count
__device__ __forceinline__ void tpl_colsum(const double* rows, const int32_t* accept, int64_t P, int width, int t,
                                           double* out, double* count) {
    if (t >= width) return;
    double s = 0.0, n = 0.0;
    for (int64_t j = 0; j < P; ++j)
        if (accept[j]) { s += rows[j * width + t]; n += 1.0; }
    out[t] = s / n;
    if (t == 0) *count = n;
}

// global reference medians I1m, Q1m over pulses [0, min(P,100)) x samples [0, 900); get(pulse,
// sample, i, q) reads one sample of the set
template <typename G>
__device__ __forceinline__ void tpl_refmed(G get, int64_t P, float* out) {
    const int np = (int)(P < 100 ? P : 100);
    const int n = np * 900;
    const float mi = wg_median([&](int k) { float i, q; get(k / 900, k % 900, i, q); return i; }, n);
    const float mq = wg_median([&](int k) { float i, q; get(k / 900, k % 900, i, q); return q; }, n);
    if (threadIdx.x == 0) { out[0] = mi; out[1] = mq; }
}

// pm, pdev: median / std of appended pass-1 peaks > 15 (pulses.py:334-336), in pulse order; one
// thread's work
__device__ void tpl_peakstats(const double* peaks, const int32_t* appended, int64_t P, double* out,
                              double* scratch) {
    int n = 0;
    for (int64_t j = 0; j < P; ++j)
        if (appended[j] && peaks[j] > 15.0) scratch[n++] = peaks[j];
    out[2] = n;
    if (n == 0) { out[0] = out[1] = NAN; return; }
    // std in pulse order (pairwise), then the median on a sorted copy (insertion sort, n <= 1000)
    double* tmp = scratch + P;
    out[1] = np_std(scratch, n, tmp);
    for (int i = 1; i < n; ++i) {
        const double v = scratch[i];
        int k = i - 1;
        while (k >= 0 && scratch[k] > v) { scratch[k + 1] = scratch[k]; --k; }
        scratch[k + 1] = v;
    }
    out[0] = (n & 1) ? scratch[n / 2] : (scratch[n / 2 - 1] + scratch[n / 2]) / 2.0;
}

// first index of the template's maximum (kTN when every sample is NaN), by a whole workgroup
__device__ __forceinline__ int tpl_peak(const double* tpl) {
    double best = -INFINITY;
    int bi = kTN;
    for (int t = threadIdx.x; t < kTN; t += kTB)
        if (tpl[t] > best || (tpl[t] == best && t < bi)) { best = tpl[t]; bi = t; }
    return wg_argmax_first(best, bi);
}

// near-optimal filter: s = deg2rad(template[pk-pre : pk-pre+800]); H = S / J, H[0] = 0;
// g = real(ifft(H)) (correlation weights), g /= g.s; coeff = g[pre-10 : pre-10+ncoeff]. By a whole
// workgroup of kTB threads; returns pk = tpl_peak(tpl) (every thread).
__device__ __forceinline__ int tpl_optfilt(const double* tpl, const double* noise, int pre, int ncoeff,
                                           double* coeff, double* work) {
    __shared__ double s[kTNoise];
    const int t0 = threadIdx.x;
    const int pk = tpl_peak(tpl);
    const int p0 = pk - pre;
    for (int t = t0; t < kTNoise; t += kTB) {
        const int i = p0 + t;
        s[t] = (i >= 0 && i < kTN) ? tpl[i] * 0.017453292519943295 : 0.0;
    }
    __syncthreads();
    double* Hr = work;
    double* Hi = work + kTNoise;
    double* g = work + 2 * kTNoise;
    __shared__ double twr[kTNoise], twi[kTNoise];
    dft_twiddles(twr, twi);
    __syncthreads();
    for (int f = t0; f < kTNoise; f += kTB) {
        double re = 0.0, im = 0.0;
        dft_row(f, twr, twi, [&](int n, double c, double sn) {
            re += s[n] * c;
            im += s[n] * sn;
        });
        const double J = noise[f];
        Hr[f] = f == 0 ? 0.0 : re / J;
        Hi[f] = f == 0 ? 0.0 : im / J;
    }
    __syncthreads();
    for (int m = t0; m < kTNoise; m += kTB) {
        double re = 0.0;
        dft_row(m, twr, twi, [&](int f, double c, double sn) {
            re += Hr[f] * c + Hi[f] * sn;  // exp(+i theta) = conj(tw)
        });
        g[m] = re / kTNoise;
    }
    __syncthreads();
    double d = 0.0;
    for (int m = t0; m < kTNoise; m += kTB) d += g[m] * s[m];
    const double norm = wg_sum(d);
    const int k0 = pre - 10;
    for (int i = t0; i < ncoeff; i += kTB) {
        const int m = k0 + i;
        coeff[i] = (m >= 0 && m < kTNoise) ? g[m] / norm : 0.0;
    }
    return pk;
}
__global__ void k_tpl_optfilt(const double* tpl, const double* noise, int pre, int ncoeff, double* coeff,
                              double* work) {
    tpl_optfilt(tpl, noise, pre, ncoeff, coeff, work);
}

// ---- the record bank: the same stages for every channel of a group at once -----------------------
// Channel b of the group (caller's channel c0 + b) owns slot b of every workspace table; its
// scalars (ready count, status, I1m/Q1m, pm/pdev, counts) stay in those tables from kernel to kernel.

__device__ __forceinline__ SrcBank bank_record(const BankArgs& a, int b, int64_t j) {
    const int64_t o = (((int64_t)(a.c0 + b)) * a.R + j) * kTN;
    return SrcBank{a.I + o, a.Q ? a.Q + o : nullptr, a.sign};
}

// ready and status of every channel, then I1m, Q1m of the channels worked on
__global__ __launch_bounds__(1024) void k_bank_refmed(BankArgs a) {
    const int b = blockIdx.x;
    int32_t rd = a.ready[(int64_t)(a.c0 + b) * a.ready_stride];
    rd = rd < 0 ? 0 : (rd > a.R ? a.R : rd);
    const int32_t need = a.min_records > 1 ? a.min_records : 1;
    const int32_t st = rd >= need ? 0 : 1;
    if (threadIdx.x == 0) { a.nready[b] = rd; a.status[b] = st; }
    if (st) return;
    tpl_refmed([&](int p, int t, float& i, float& q) { bank_record(a, b, p).load(t, i, q); }, rd,
               a.refmed + 2 * b);
}

__global__ __launch_bounds__(kTB) void k_bank_pulse(BankArgs a, int pass) {
    const int b = blockIdx.y;
    const int j = blockIdx.x;
    if (a.status[b]) return;
    const int P = a.nready[b];
    if (j >= (pass == 1 && P > 1000 ? 1000 : P)) return;
    const int64_t s = (int64_t)b * a.R + j;
    const double* st = a.stats + 8 * b;
    tpl_pulse(bank_record(a, b, j),
              TplPulse{a.refmed[2 * b], a.refmed[2 * b + 1], a.tP + (int64_t)b * kTN, st[0], st[1],
                       a.rows + s * kTN, a.nrows + s * kTNoise, a.accept + s, a.peaks + s, a.appended + s, pass,
                       pass == 2 && j < 1000 ? 2 : 1});
}

// which: 0 pass-1 rows -> tP, count1; 1 pass-2 rows -> tPf, count; 2 noise rows -> noise, count
__global__ void k_bank_colsum(BankArgs a, int which) {
    const int b = blockIdx.y;
    if (a.status[b]) return;
    int64_t P = a.nready[b];
    if (which == 0 && P > 1000) P = 1000;
    const int width = which == 2 ? kTNoise : kTN;
    const double* rows = which == 2 ? a.nrows + (int64_t)b * a.R * kTNoise : a.rows + (int64_t)b * a.R * kTN;
    double* out = which == 0 ? a.tP + (int64_t)b * kTN
                             : (which == 1 ? a.tPf + (int64_t)b * kTN : a.noise + (int64_t)b * kTNoise);
    tpl_colsum(rows, a.accept + (int64_t)b * a.R, P, width, blockIdx.x * blockDim.x + threadIdx.x, out,
               a.stats + 8 * b + (which == 0 ? 3 : 4));
}

// pm, pdev; then the first of the two status decisions: no pulse passed pass 1
__global__ void k_bank_peakstats(BankArgs a) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0 || a.status[b]) return;
    const int64_t P = a.nready[b] > 1000 ? 1000 : a.nready[b];
    double* st = a.stats + 8 * b;
    tpl_peakstats(a.peaks + (int64_t)b * a.R, a.appended + (int64_t)b * a.R, P, st,
                  a.scratch + (int64_t)b * (2 * (int64_t)a.R + 8));
    if (!(st[3] > 0)) a.status[b] = 2;
}

// the second decision (none passed pass 2), pstart and flag, the filter (where out_coeff is given),
// and the caller's rows: written at status 0 only
__global__ __launch_bounds__(kTB) void k_bank_finish(BankArgs a) {
    const int b = blockIdx.x;
    const int64_t c = a.c0 + b;
    const int t0 = threadIdx.x;
    const double* st = a.stats + 8 * b;
    int status = a.status[b];
    if (status == 0 && !(st[4] > 0)) status = 3;
    if (status) {
        if (t0 == 0) {
            mkid_bank_result r{};
            if (status >= 2) { r.count1 = st[3]; r.pm = st[0]; r.pdev = st[1]; }
            r.flag = r.pstart = -1;
            r.status = status;
            r.ready = a.nready[b];
            a.result[c] = r;
        }
        return;
    }
    const double* tpl = a.tPf + (int64_t)b * kTN;
    const double* noise = a.noise + (int64_t)b * kTNoise;
    int pk;
    if (a.out_coeff) {
        double* co = a.coeff + (int64_t)b * kTNoise;
        pk = tpl_optfilt(tpl, noise, a.pre, a.ncoeff, co, a.work + (int64_t)b * 3 * kTNoise);
        for (int i = t0; i < a.ncoeff; i += kTB) a.out_coeff[c * a.ncoeff + i] = (float)co[i];  // own writes
    } else {
        pk = tpl_peak(tpl);   // mkid_make_template: no filter, pstart alone
    }
    if (a.out_tpl)
        for (int t = t0; t < kTN; t += kTB) a.out_tpl[c * kTN + t] = tpl[t];
    if (a.out_noise)
        for (int t = t0; t < kTNoise; t += kTB) a.out_noise[c * kTNoise + t] = noise[t];
    if (t0 == 0) {
        mkid_bank_result r{};
        r.count = st[4]; r.count1 = st[3]; r.pm = st[0]; r.pdev = st[1];
        r.flag = (st[4] < 500 || st[0] < 10 || st[0] > 150) ? 1 : 0;
        // the scan `if (t[i] > t[ps]) ps = i` from ps = 0: the first maximum; 0 when t[0] is NaN
        r.pstart = (pk >= kTN || tpl[0] != tpl[0]) ? 0 : pk;
        r.status = 0;
        r.ready = a.nready[b];
        a.result[c] = r;
    }
}

hipError_t launch_bank_filters(const BankArgs& a, hipStream_t s) {
    const unsigned g = (unsigned)a.g, R = (unsigned)a.R, R1 = R < 1000 ? R : 1000;
    hipLaunchKernelGGL(k_bank_refmed, dim3(g), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_bank_pulse, dim3(R1, g), dim3(kTB), 0, s, a, 1);
    hipLaunchKernelGGL(k_bank_colsum, dim3((kTN + 255) / 256, g), dim3(256), 0, s, a, 0);
    hipLaunchKernelGGL(k_bank_peakstats, dim3(g), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_bank_pulse, dim3(R, g), dim3(kTB), 0, s, a, 2);
    hipLaunchKernelGGL(k_bank_colsum, dim3((kTN + 255) / 256, g), dim3(256), 0, s, a, 1);
    hipLaunchKernelGGL(k_bank_colsum, dim3((kTNoise + 255) / 256, g), dim3(256), 0, s, a, 2);
    hipLaunchKernelGGL(k_bank_finish, dim3(g), dim3(kTB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_optimal_filter(const double* tpl, const double* noise, int pre, int ncoeff, double* coeff,
                                 double* work, hipStream_t s) {
    hipLaunchKernelGGL(k_tpl_optfilt, dim3(1), dim3(kTB), 0, s, tpl, noise, pre, ncoeff, coeff, work);
    return hipGetLastError();
}

}  // namespace mkid
