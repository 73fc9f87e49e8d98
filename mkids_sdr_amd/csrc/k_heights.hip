// Per-packet optimal-filter pulse height (BASELINE config 5: "per-channel optimal-filter
// pulse-height estimation (fp32)"). The reference computes the pulse template and noise PSD
// (MakeTemplate, pulses.py:239-427) but stubs the filter (pulses.py:398, PulseAnalysis.coeff
// Float32Col(100)); mkid_optimal_filter fills the stub and this kernel applies a per-channel
// filter of that form to the phase stream at every photon packet:
//     h_p = sum_{i < ncoeff} coeff[ch_p][i] * phase[ts_p - pre + i][ch_p]
// One wave per packet: lane l accumulates taps l, l + 64, ... in fp32, then wg::wave_reduce's
// fixed-order butterfly (deterministic). The phase rows of one packet's window are strided by
// C floats, so each lane's read is its own cache line; the volume is small (ncoeff x 4 B per
// packet). Windows that start before the call's first row read the context's carried history of
// the previous call's last rows (mkid_calib.hip pulse_heights), so a streamed run loses heights
// only at the stream start and for windows past the call's last row.
#include "mkid_internal.h"
#include "wg_common.h"

namespace mkid {

constexpr int kHeightWaves = 4;  // packets (waves) per 256-thread workgroup

// Grid-stride over packets: the count can be a device value (the trigger's written count,
// a.d_n) so that a step launches with no host round trip; waves beyond it exit at once.
__global__ __launch_bounds__(64 * kHeightWaves) void k_pulse_heights(HeightArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t n = pkt::count(a.d_n, a.n);
    const int64_t nw = (int64_t)gridDim.x * kHeightWaves;
    for (int64_t p = (int64_t)blockIdx.x * kHeightWaves + (threadIdx.x >> 6); p < n; p += nw) {
        const pkt::Stamp st = pkt::decode(a.events[p], a.j0);
        const int64_t r0 = st.jg - a.j0 - a.pre;  // first phase row of the window (< 0: history)
        const bool inside = st.ch < a.C && r0 >= -a.hrows && r0 + a.ncoeff <= a.rows;
        float acc = 0.f;
        if (inside) {
            const float* cf = a.coeff + (size_t)st.ch * a.ncoeff;
            for (int i = lane; i < a.ncoeff; i += 64) {
                const int64_t r = r0 + i;
                const float v = r >= 0 ? a.phase[r * a.C + st.ch] : a.hist[(a.hrows + r) * a.C + st.ch];
                acc = fmaf(cf[i], v, acc);
            }
        }
        acc = wg::wave_reduce(acc, wg::Add{});   // the order that gives the height its bits
        if (lane == 0) a.heights[p] = inside ? acc : __builtin_nanf("");
    }
}

hipError_t launch_pulse_heights(const HeightArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    // a wave per packet until 8 waves per SIMD on every CU (32 workgroups of 4), then grid-stride
    const int64_t blocks = pkt::grid_stride_blocks(a.n, kHeightWaves, a.ncu, 32);
    hipLaunchKernelGGL(k_pulse_heights, dim3((unsigned)blocks), dim3(64 * kHeightWaves), 0, s, a);
    return hipGetLastError();
}

}  // namespace mkid
