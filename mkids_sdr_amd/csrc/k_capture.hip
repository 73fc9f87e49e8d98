// Pulse capture: for every photon packet, copy the phase window around its stamp into a per-channel
// record bank, on the device, for all channels at once, across streamed calls (the scale-up of
// RoachPulses.contsnapshot, ROACH_Pulses.py:557-762, and of the window saving in
// pulse_triggering_v2.py:104-174). The bank feeds mkid_make_template / mkid_optimal_filter.
//
// Contract (include/mkidgpu.h mkid_capture_pulses; tests/capture_ref.py is its numpy statement).
// The capture is configured with length L, pre and max_per_ch R. A stream segment is a run of calls
// whose j0 each equal the previous j0 + rows; it covers global phase rows [j_first, j_end).
//   - a packet's 28-bit stamp is unwrapped by pkt::decode (pkt_common.h): base = max(j0 - 2^27, 0),
//     jg = base + ((ts - base) mod 2^28), with the j0 of the call that delivers the packet;
//   - a packet of channel c < C is eligible when its window start s = jg - pre >= j_first and the
//     context still carries row s (s >= j0 - carried rows: true for every packet passed with the
//     call that produced it, whose stamp is >= j0 - 1); packets of channels >= C are ignored;
//   - an eligible packet completes in the call where s + L <= j_end first holds; until then it waits
//     in the context's pending list (per channel, unwrapped stamps);
//   - completions of a channel come in list order, pending packets first: stamp order, since
//     packets are channel-major and time-ascending. The first R are recorded,
//     records[c][k][0:L] = phase[s : s + L, c] bit-identical and stamps[c][k] = jg; later ones are
//     counted in info[c].dropped, as are packets the pending list has no room for (it is sized so
//     that packets at least cfg.dead_time apart always fit);
//   - info[c] = {ready, dropped}: the caller zeroes it to start a bank, the kernels continue from
//     the ready they find, so slot numbers are deterministic.
// Any chunking of a segment gives the result of one call over the whole segment.
//
// Layout. k_capture_plan, one wave per channel: binary search of the channel's sub-list in the
// packets, then 64 candidates (pending, then new) per step; ballots rank the completing and the
// still-pending ones, which gives each completion its slot with no atomics. It writes the stamps,
// the new pending list (double-buffered), info, and the channel's work item {first slot, count}.
// k_capture_tiles then moves the data: phase is time-major [J][C], so a record is a column walk at
// a stride of 4 C bytes. A workgroup takes a 64-row x 64-channel tile of (carried rows ++ phase),
// finds per channel the records of this call that overlap the tile's rows (binary search in the
// stamps just written: they ascend), loads the tile with coalesced 256-byte row segments into LDS
// (row pitch 65 words: the transposed read is conflict-free), and writes each overlap as one
// contiguous run of up to 64 floats into records[c][slot]. Every phase row is read once and every
// record word written once; tiles that no record overlaps are not loaded.
#include <climits>

#include "mkid_internal.h"

namespace mkid {

constexpr int kCapTile = 64;          // tile rows = tile channels = lanes of a wave
constexpr int kCapPitch = kCapTile + 1;
constexpr int kCapWaves = 4;          // waves per workgroup (plan: channels; tiles: 16 columns each)
constexpr int kCapNear = 4;           // overlapping records per (tile, channel) whose stamps the search keeps

// first index in [0, n) whose channel field is >= c (n if none); the list is channel-major
__device__ __forceinline__ int64_t cap_lower(const uint64_t* ev, int64_t n, int c) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (pkt::channel(ev[mid]) < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64 * kCapWaves) void k_capture_plan(CaptureArgs a) {
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.x * kCapWaves + (threadIdx.x >> 6);
    if (c >= a.C) return;
    const int64_t n = pkt::count(a.d_n, a.n);
    const int64_t lo = cap_lower(a.events, n, c), hi = cap_lower(a.events, n, c + 1);
    const int np = min(max(a.pend_n_in[c], 0), a.PC);
    const int64_t total = np + (hi - lo);
    const int64_t j_end = a.j0 + a.rows, first = a.j0 - a.hrows;
    const int ready0 = min(max(a.info[2 * c], 0), a.R);
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    int64_t ncomp = 0, npend = 0;
    for (int64_t b0 = 0; b0 < total; b0 += 64) {
        const int64_t idx = b0 + lane;
        int64_t jg = 0;
        bool ok = false;
        if (idx < np) {
            jg = a.pend_in[(size_t)c * a.PC + idx];
            ok = true;
        } else if (idx < total) {
            const pkt::Stamp st = pkt::decode(a.events[lo + (idx - np)], a.j0);
            jg = st.jg;
            ok = st.ch == c && jg - a.pre >= first;
        }
        const bool comp = ok && jg - a.pre + a.L <= j_end;
        const bool pend = ok && !comp;
        const uint64_t mc = __ballot(comp), mp = __ballot(pend);
        const int64_t kc = ncomp + __popcll(mc & below), kp = npend + __popcll(mp & below);
        if (comp && ready0 + kc < a.R) a.stamps[(size_t)c * a.R + ready0 + kc] = jg;
        if (pend && kp < a.PC) a.pend_out[(size_t)c * a.PC + kp] = jg;
        ncomp += __popcll(mc);
        npend += __popcll(mp);
    }
    if (lane == 0) {
        const int64_t nrec = ncomp < a.R - ready0 ? ncomp : a.R - ready0;
        const int64_t over = npend > a.PC ? npend - a.PC : 0;
        a.info[2 * c] = ready0 + (int)nrec;
        a.info[2 * c + 1] += (int)(ncomp - nrec + over);
        a.pend_n_out[c] = (int)(npend - over);
        a.work[2 * c] = ready0;
        a.work[2 * c + 1] = (int)nrec;
    }
}

__global__ __launch_bounds__(64 * kCapWaves) void k_capture_tiles(CaptureArgs a) {
    __shared__ float tile[kCapTile * kCapPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = (int)blockIdx.y * kCapTile;
    const int64_t v0 = (int64_t)blockIdx.x * kCapTile - a.hrows;       // first tile row, relative to j0
    const int nvalid = (int)(a.rows - v0 < kCapTile ? a.rows - v0 : kCapTile);
    const int64_t g0 = a.j0 + v0, g1 = g0 + nvalid;                    // global rows [g0, g1)
    // lane j < 16 of a wave: the records of channel c0 + wave + 4 j that overlap [g0, g1), and the
    // stamps of the first kCapNear of them (the usual case: a record is far longer than a tile)
    int slot0 = 0, ka = 0, kb = 0;
    long long near[kCapNear] = {};
    if (lane < kCapTile / kCapWaves) {
        const int c = c0 + wave + kCapWaves * lane;
        if (c < a.C) {
            slot0 = a.work[2 * c];
            const int nrec = a.work[2 * c + 1];
            const int64_t* st = a.stamps + (size_t)c * a.R + slot0;
            int lo = 0, hi = nrec;          // first record that ends after g0
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (st[mid] - a.pre + a.L <= g0) lo = mid + 1; else hi = mid;
            }
            ka = lo;
#pragma unroll
            for (int q = 0; q < kCapNear; ++q) near[q] = ka + q < nrec ? (long long)st[ka + q] : LLONG_MAX;
            kb = ka;                        // first record that starts at or after g1
#pragma unroll
            for (int q = 0; q < kCapNear; ++q) kb += near[q] != LLONG_MAX && near[q] - a.pre < g1;
            if (kb == ka + kCapNear) {
                lo = kb;
                hi = nrec;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (st[mid] - a.pre < g1) lo = mid + 1; else hi = mid;
                }
                kb = lo;
            }
        }
    }
    if (!__syncthreads_or(kb > ka)) return;
    // 16 rows per wave, all loads in flight before the first LDS write
    float v[kCapTile / kCapWaves];
#pragma unroll
    for (int q = 0; q < kCapTile / kCapWaves; ++q) {
        const int r = wave + kCapWaves * q;
        const int64_t vr = v0 + r;
        const float* src = vr >= 0 ? a.phase + vr * a.C : a.hist + (a.hrows + vr) * a.C;
        v[q] = (r < nvalid && c0 + lane < a.C) ? src[c0 + lane] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < kCapTile / kCapWaves; ++q) tile[(wave + kCapWaves * q) * kCapPitch + lane] = v[q];
    __syncthreads();
    for (int j = 0; j < kCapTile / kCapWaves; ++j) {
        const int cc = wave + kCapWaves * j;
        const int s0 = __shfl(slot0, j, 64), k0 = __shfl(ka, j, 64), k1 = __shfl(kb, j, 64);
        if (k1 <= k0) continue;
        const size_t bank = (size_t)(c0 + cc) * a.R + s0;
        const float val = tile[lane * kCapPitch + cc];
#pragma unroll
        for (int q = 0; q < kCapNear; ++q) {
            const int64_t i = g0 + lane - ((int64_t)__shfl(near[q], j, 64) - a.pre);
            if (k0 + q < k1 && lane < nvalid && i >= 0 && i < a.L) a.records[(bank + k0 + q) * a.L + i] = val;
        }
        for (int kk = k0 + kCapNear; kk < k1; kk += 64) {   // dense packets: 64 stamps per step
            const int cnt = k1 - kk < 64 ? k1 - kk : 64;
            const long long mine = lane < cnt ? (long long)a.stamps[bank + kk + lane] : 0;
            for (int k = 0; k < cnt; ++k) {
                const int64_t i = g0 + lane - ((int64_t)__shfl(mine, k, 64) - a.pre);
                if (lane < nvalid && i >= 0 && i < a.L) a.records[(bank + kk + k) * a.L + i] = val;
            }
        }
    }
}

hipError_t launch_capture(const CaptureArgs& a, hipStream_t s) {
    if (a.C <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_capture_plan, dim3((unsigned)((a.C + kCapWaves - 1) / kCapWaves)), dim3(64 * kCapWaves), 0,
                       s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.hrows + a.rows <= 0) return e;
    const int64_t tr = (a.hrows + a.rows + kCapTile - 1) / kCapTile;
    hipLaunchKernelGGL(k_capture_tiles, dim3((unsigned)tr, (unsigned)((a.C + kCapTile - 1) / kCapTile)),
                       dim3(64 * kCapWaves), 0, s, a);
    return hipGetLastError();
}

}  // namespace mkid
