// Per-packet pulse height with a lag search and a parabolic vertex (include/mkidgpu.h
// mkid_pulse_fit; the rule is fit_common.h): the optimal filter of k_heights.hip applied at the
// 2 L + 1 alignments d = -L .. L around the trigger's stamp,
//     H[d] = sum_{i < ncoeff} coeff[ch][i] * phase[jg - pre + d + i][ch]
// then the lowest lag of largest s H and the vertex of the parabola through its neighbours.
// One wave per packet, in a region of LDS of its own (mkid_plan.h FitPlan):
//   stage   lane l copies window rows l, l + 64, ... (W = ncoeff + 2 L rows from r0 - L on, each its
//           own cache line, read from global memory once per packet) and the channel's coefficients
//   lags    nl = 2 L + 1, G = 64 / nl: lane g nl + d adds taps i = g, g + G, ... of lag d - L in
//           ascending i with one fmaf each, reading cf[i] (one address per group: broadcast) and
//           w[i + d]. The addresses of a 32-lane half are the consecutive words i + g + d, at most
//           32 of them for every L, so no two share a bank (ds_read_b32: 32 banks per half).
//   sum     lane d < nl adds the G partial sums of its lag in ascending g
//   fit     lane 0 runs fit::select on the nl values and stores the outputs
// The order of every sum depends on ncoeff and L only, and there are no atomics: a packet's outputs
// are the same bits whatever its place in the list, the grid or the call that carries its rows.
// The region is the wave's own, so wave barriers (no workgroup barrier) order its phases.
#include "fit_common.h"
#include "mkid_internal.h"
#include "mkid_plan.h"

namespace mkid {

// Grid-stride over packets as k_pulse_heights: the count can be a device value.
__global__ __launch_bounds__(64 * plan::kFitWaves) void k_pulse_fit(FitArgs a) {
    extern __shared__ float fit_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    float* w = fit_lds + (size_t)wave * a.wave_floats;
    float* cf = w + a.off_cf;
    float* part = w + a.off_part;
    float* hv = w + a.off_h;
    const int g = lane / a.nl, d = lane - g * a.nl;
    const bool works = g < a.G;
    const int64_t n = pkt::count(a.d_n, a.n);
    const int64_t nw = (int64_t)gridDim.x * waves;
    const float nan = __builtin_nanf("");
    for (int64_t p = (int64_t)blockIdx.x * waves + wave; p < n; p += nw) {
        const pkt::Stamp st = pkt::decode(a.events[p], a.j0);
        const int64_t r0 = st.jg - a.j0 - a.pre;
        if (!fit::inside(st.ch, a.C, r0, a.L, a.ncoeff, a.hrows, a.rows)) {   // wave-uniform
            if (lane == 0) {
                a.heights[p] = nan;
                if (a.dt) a.dt[p] = nan;
                if (a.lag) a.lag[p] = INT32_MIN;
                if (a.h0) a.h0[p] = nan;
            }
            continue;
        }
        const int64_t rw = r0 - a.L;   // first row of the window (< 0: carried rows)
        for (int i = lane; i < a.W; i += 64) {
            const int64_t r = rw + i;
            w[i] = r >= 0 ? a.phase[r * a.C + st.ch] : a.hist[(a.hrows + r) * a.C + st.ch];
        }
        const float* co = a.coeff + (size_t)st.ch * a.ncoeff;
        for (int i = lane; i < a.ncoeff; i += 64) cf[i] = co[i];
        __builtin_amdgcn_wave_barrier();
        float acc = 0.f;
        if (works)
            for (int i = g; i < a.ncoeff; i += a.G) acc = fmaf(cf[i], w[i + d], acc);
        part[lane] = acc;
        __builtin_amdgcn_wave_barrier();
        if (lane < a.nl) {
            float h = part[lane];
            for (int k = 1; k < a.G; ++k) h += part[k * a.nl + lane];
            hv[lane] = h;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            const fit::Result<float> r = fit::select<float>(hv, a.L, a.s);
            a.heights[p] = r.height;
            if (a.dt) a.dt[p] = r.dt;
            if (a.lag) a.lag[p] = r.lag;
            if (a.h0) a.h0[p] = r.h0;
        }
        __builtin_amdgcn_wave_barrier();   // the next packet's staging overwrites the region
    }
}

hipError_t launch_pulse_fit(FitArgs a, const plan::FitPlan& p, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    a.W = p.W, a.nl = p.nl, a.G = p.G;
    a.off_cf = p.off_cf, a.off_part = p.off_part, a.off_h = p.off_h, a.wave_floats = p.wave_floats;
    hipLaunchKernelGGL(k_pulse_fit, dim3((unsigned)p.blocks(a.n)), dim3(64 * p.waves), (size_t)p.lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace mkid
