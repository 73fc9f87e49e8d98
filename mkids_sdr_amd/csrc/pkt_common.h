// The trigger's packet list (d_events, n | *d_count, j0) as every call after the trigger reads it,
// one definition for the kernels and for the host entry points: the fields of a wide packet word
// (include/mkidgpu.h MKID_PKT_*; trig_common.h pack_wide writes them), its unwrapped stamp, how many
// entries of a counted list are valid, the cut of a list into one slice per workgroup, the grid of a
// grid-stride pass, what the ends of a run of equal cells add, and the reference's packet word.
// No HIP is needed: tools/plan_fuzz.cpp runs the host side under the CPU sanitizers.
#pragma once
#include <stdint.h>

#include "mkidgpu.h"

#if defined(__HIPCC__)
#define PKT_HD __host__ __device__ inline
#else
#define PKT_HD inline
#endif

namespace mkid {

// A sliced pass (the spectra, the photon rows) runs at most kObsMaxBlocks workgroups, one thread
// each in the one-workgroup scan between its kernels, over slices of about kObsSlice packets.
constexpr int kObsMaxBlocks = 1024;
constexpr int kObsSlice = 2048;

namespace pkt {

PKT_HD int32_t channel(uint64_t w) { return (int32_t)((w >> MKID_PKT_CH_SHIFT) & 0xFFF); }
PKT_HD int32_t peak(uint64_t w) { return (int32_t)((w >> MKID_PKT_PEAK_SHIFT) & 0xFFF); }
PKT_HD int32_t base(uint64_t w) { return (int32_t)((w >> MKID_PKT_BASE_SHIFT) & 0xFFF); }

// Channel and global phase row of a wide packet delivered with the call whose first row is j0: with
// lo = max(j0 - 2^27, 0), the one row of [lo, lo + 2^28) that is congruent to the 28-bit stamp.
// (A packet emitted at a call's first sample is stamped at the previous call's last row, so the
// range opens below j0.)
struct Stamp {
    int32_t ch;
    int64_t jg;
};
PKT_HD Stamp decode(uint64_t w, int64_t j0) {
    const int64_t mask = (int64_t)MKID_PKT_TS_MASK;
    const int64_t ts = (int64_t)(w & MKID_PKT_TS_MASK);
    const int64_t lo = j0 > ((int64_t)1 << 27) ? j0 - ((int64_t)1 << 27) : 0;
    return Stamp{channel(w), lo + ((ts - (lo & mask)) & mask)};
}

// Valid entries of a list of capacity n: n itself, or the device-side count clamped into 0 .. n.
PKT_HD int64_t count(const int64_t* d_n, int64_t n) {
    if (!d_n) return n;
    const int64_t v = *d_n;
    return v < 0 ? 0 : (v < n ? v : n);
}

// One contiguous slice per workgroup: 1 .. kObsMaxBlocks slices of about kObsSlice packets, the
// slice a multiple of the workgroup's threads (a longer list makes the slices grow).
struct Slices {
    int32_t blocks;
    int64_t slice;
};
inline Slices slices(int64_t n, int32_t threads) {
    const int64_t want = (n + kObsSlice - 1) / kObsSlice;
    Slices p{(int32_t)(want < 1 ? 1 : (want > kObsMaxBlocks ? kObsMaxBlocks : want)), 0};
    const int64_t per = (n + p.blocks - 1) / p.blocks;
    p.slice = (per + threads - 1) / threads * threads;
    return p;
}
// Slice `block` of the first n packets: [b0, b1), empty where the count ends before it.
PKT_HD void bounds(int64_t block, int64_t slice, int64_t n, int64_t& b0, int64_t& b1) {
    b0 = block * slice;
    b1 = b0 + slice < n ? b0 + slice : n;
}

// Workgroups of a grid-stride pass over n items: one item per thread until per_cu workgroups on
// every compute unit are reached (ncu <= 0: 256 units).
inline int64_t grid_stride_blocks(int64_t n, int32_t threads, int32_t ncu, int32_t per_cu) {
    const int64_t need = (n + threads - 1) / threads, cap = (int64_t)(ncu > 0 ? ncu : 256) * per_cu;
    return need < cap ? need : cap;
}

// A run of packets i0 .. i1 of one cell is counted by its two ends: the first adds -i0 and the last
// i1 + 1 (i1 + 1 - i0 where they are the same packet), modulo 2^64 and so modulo 2^32.
PKT_HD uint64_t run_delta(int64_t i, bool first, bool last) {
    return (last ? (uint64_t)(i + 1) : 0) - (first ? (uint64_t)i : 0);
}

// The reference's 64-bit packet (packets.encode_wire): 8-bit channel, peak, peak - base + 2048
// clamped to 12 bits, base, and a 20-bit time.
PKT_HD uint64_t reference_word(uint64_t ch, int64_t peak, int64_t base, uint64_t t20) {
    const int64_t d = peak - base + 2048;
    const uint64_t p1 = (uint64_t)(d < 0 ? 0 : (d > 4095 ? 4095 : d));
    return ch << 56 | (uint64_t)peak << 44 | p1 << 32 | (uint64_t)base << 20 | (t20 & 0xFFFFF);
}

}  // namespace pkt
}  // namespace mkid
