// The observing products after the heights (include/mkidgpu.h mkid_count_photons and
// mkid_height_spectra state them), one definition for the kernels of k_observe.hip and for the host
// entry points mkid_count_photons_host / mkid_height_spectra_host: the second of a packet on the
// 1 PPS timebase (packets.Timebase.second), where a packet is counted, the spectrum column of a
// height, and which packets wait for their height; and, further down, the photon rows of
// mkid_list_photons / mkid_fill_photon_heights (k_photons.hip), their ring forms, and the packed
// second of mkid_pack_second / mkid_clear_second (k_pack.hip), with their host entry points. A
// packet's channel and unwrapped stamp are pkt::decode's (pkt_common.h). The host loops below are the
// whole of the host entry points, so that the CPU sanitizer build (tools/plan_fuzz.cpp) runs them
// without HIP.
#pragma once
#include <stdint.h>

#include "mkidgpu.h"
#include "pkt_common.h"

#if defined(__HIPCC__)
#define OBS_HD __host__ __device__ inline
#else
#define OBS_HD inline
#endif

namespace mkid {
namespace obs {

constexpr int32_t kMaxSeconds = 1 << 20;
constexpr int32_t kMaxBins = 16384;
constexpr int32_t kExtraCols = 3;   // under, over, no height

// The sample clock as Timebase takes it: a positive integer number of samples per second that a
// double holds exactly.
OBS_HD bool fs_ok(double fs) { return fs >= 1.0 && fs < 9007199254740992.0 && fs == (double)(int64_t)fs; }
OBS_HD bool seconds_ok(int32_t n_seconds) { return n_seconds >= 1 && n_seconds <= kMaxSeconds; }
OBS_HD bool bins_ok(int32_t nbins) { return nbins >= 1 && nbins <= kMaxBins; }
// every stamp of a call (below j0 + 2^28) times N stays inside int64
OBS_HD bool j0_ok(int64_t j0, int32_t N) { return j0 >= 0 && N >= 1 && j0 <= INT64_MAX / N - ((int64_t)1 << 28); }

// Second of phase row jg: ADC sample jg N at fs samples per second.
OBS_HD int64_t second(int64_t jg, int64_t N, int64_t fs) { return jg * N / fs; }

// Where a packet is counted: cell sec C + ch of the image, or one of the two `outside` counters.
constexpr int64_t kNonPixel = -1, kLate = -2;   // outside[0], outside[1]
OBS_HD int64_t cell(const pkt::Stamp& st, int32_t C, int64_t N, int64_t fs, int32_t n_seconds) {
    if (st.ch >= C) return kNonPixel;
    const int64_t sec = second(st.jg, N, fs);
    return sec < n_seconds ? sec * C + st.ch : kLate;
}

// Column of height h in a row of nbins + 3: 0 under, 1 .. nbins the bins, nbins + 1 over,
// nbins + 2 no height. t = h - lo and u = t inv are each rounded once in fp32, and the float
// compares come before the conversion to int, so every (h, lo, inv) has a defined column.
OBS_HD int32_t column(float h, float lo, float inv, int32_t nbins) {
    if (!__builtin_isfinite(h)) return nbins + 2;
#if defined(__HIP_DEVICE_COMPILE__)
    const float u = __fmul_rn(__fsub_rn(h, lo), inv);
#else
    const float t = h - lo;   // fp32 arithmetic on the hosts built for (no excess precision)
    const float u = t * inv;
#endif
    if (u != u) return nbins + 2;
    if (u < 0.f) return 0;
    if (u >= (float)nbins) return nbins + 1;
    return 1 + (int32_t)u;
}

// A packet that waits for its height: no finite height yet and a stamp whose window passes the
// call's last row.
OBS_HD bool deferred(float h, int64_t jg, int64_t j_defer) { return !__builtin_isfinite(h) && jg >= j_defer; }

inline bool count_args_ok(const uint64_t* events, int64_t n, int64_t j0, int32_t N, double fs, int32_t C,
                          int32_t n_seconds, const int32_t* image, const int64_t* outside) {
    return image && outside && (n == 0 || events) && n >= 0 && C >= 1 && C <= 4096 && seconds_ok(n_seconds) &&
           fs_ok(fs) && j0_ok(j0, N);
}

inline void count_host(const uint64_t* events, int64_t n, int64_t j0, int32_t N, double fs, int32_t C,
                       int32_t n_seconds, int32_t* image, int64_t* outside) {
    for (int64_t p = 0; p < n; ++p) {
        const int64_t k = cell(pkt::decode(events[p], j0), C, N, (int64_t)fs, n_seconds);
        if (k >= 0)
            ++image[k];
        else
            ++outside[k == kNonPixel ? 0 : 1];
    }
}

inline bool spectra_args_ok(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int32_t C,
                            const float* lo, const float* inv, int32_t nbins, const int32_t* spectra,
                            const uint64_t* deferred_out, int64_t cap_def, const int64_t* ndef) {
    return lo && inv && spectra && (n == 0 || (events && heights)) && n >= 0 && j0 >= 0 && C >= 1 && C <= 4096 &&
           bins_ok(nbins) && cap_def >= 0 && (!deferred_out || ndef);
}

inline void spectra_host(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int64_t j_defer,
                         int32_t C, const float* lo, const float* inv, int32_t nbins, int32_t* spectra,
                         uint64_t* deferred_out, int64_t cap_def, int64_t* ndef) {
    for (int64_t p = 0; p < n; ++p) {
        const pkt::Stamp st = pkt::decode(events[p], j0);
        if (st.ch >= C) continue;
        if (deferred_out && deferred(heights[p], st.jg, j_defer)) {
            ++ndef[0];
            if (ndef[1] >= 0 && ndef[1] < cap_def) deferred_out[ndef[1]++] = events[p];
            continue;
        }
        ++spectra[(int64_t)st.ch * (nbins + kExtraCols) + column(heights[p], lo[st.ch], inv[st.ch], nbins)];
    }
}

// ---- the per-pixel, per-second photon rows (mkid_list_photons, mkid_fill_photon_heights) ---------
// PacketMaster's /r#/p#/t<obs> table (PacketMaster.c:371-381, 978-1050) as [n_seconds][C][K]: the
// packets of cell (sec, ch) take slots in arrival order from the cell's count before the call, a
// packet whose slot is >= K is dropped (the reference's "first K kept", K = 2499 there).
constexpr int32_t kMaxRowSlots = 65536;
OBS_HD bool row_slots_ok(int32_t K) { return K >= 1 && K <= kMaxRowSlots; }
OBS_HD bool layout_ok(int32_t layout) { return layout == MKID_ROW_WIDE || layout == MKID_ROW_REFERENCE; }
// (fs - 1) 10^6 stays inside int64 for fs <= 2^43
OBS_HD bool fs_us_ok(double fs) { return fs_ok(fs) && fs <= 8796093022208.0; }
// the reference word's 8-bit channel field, 255 being the end-of-second marker
OBS_HD bool layout_fits(int32_t layout, int32_t C) { return layout != MKID_ROW_REFERENCE || C <= 254; }

// Microsecond since PPS of phase row jg (packets.Timebase.microsecond).
OBS_HD int64_t microsecond(int64_t jg, int64_t N, int64_t fs) { return jg * N % fs * 1000000 / fs; }

// The word stored for wide packet w at microsecond us: the packet with its time field replaced
// (packets.encode_wire wide), or the reference's word with us as its time (pkt::reference_word).
OBS_HD uint64_t row_word(uint64_t w, int64_t us, int32_t layout) {
    if (layout == MKID_ROW_WIDE) return (w & ~(uint64_t)MKID_PKT_TS_MASK) | (uint64_t)us;
    return pkt::reference_word((uint64_t)pkt::channel(w), pkt::peak(w), pkt::base(w), (uint64_t)us);
}

// Slots of a row that hold a packet, from the cell's count (modulo 2^32, as the image is kept).
OBS_HD int64_t row_fill(int32_t count, int32_t K) { return (uint32_t)count < (uint32_t)K ? (int64_t)(uint32_t)count : K; }

// Index of stamp jg in the ascending stamps[0 .. m), or -1.
OBS_HD int64_t find_stamp(const int64_t* stamps, int64_t m, int64_t jg) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (stamps[mid] < jg)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < m && stamps[lo] == jg ? lo : -1;
}

// ---- the ring of second slots (the _ring forms; mkid_pack_second, mkid_clear_second) -------------
// The tables are [n_slots][C][K], and second sec lives in slot sec mod n_slots while it is inside
// the window sec0 <= sec < min(sec0 + n_slots, sec_end). The unbounded tables are the window
// sec0 = 0, n_slots = sec_end = n_seconds, where ring_cell is cell.
constexpr int32_t kMaxSlots = 1 << 20;
constexpr int64_t kEarly = -3, kOverrun = -4;   // outside[2], outside[3]; a cell k < 0 counts in outside[-1 - k]
struct Window {
    int64_t sec0, sec_end;
    int32_t n_slots;
};
OBS_HD Window whole(int32_t n_seconds) { return Window{0, n_seconds, n_seconds}; }
// (sec_end + 1) fs, the first sample after the exposure's last second, stays inside int64
OBS_HD bool window_ok(const Window& w, double fs) {
    return w.n_slots >= 1 && w.n_slots <= kMaxSlots && w.sec0 >= 0 && w.sec0 <= w.sec_end && fs_ok(fs) &&
           w.sec_end <= INT64_MAX / (int64_t)fs - 1;
}
OBS_HD int64_t ring_cell(const pkt::Stamp& st, int32_t C, int64_t N, int64_t fs, const Window& w) {
    if (st.ch >= C) return kNonPixel;
    const int64_t sec = second(st.jg, N, fs);
    if (sec >= w.sec_end) return kLate;
    if (sec < w.sec0) return kEarly;
    if (sec - w.sec0 >= w.n_slots) return kOverrun;
    return sec % w.n_slots * C + st.ch;
}

inline bool list_ring_args_ok(const uint64_t* events, int64_t n, int64_t j0, int32_t N, double fs, int32_t C,
                              const Window& w, int32_t K, int32_t layout, const int32_t* image, const int64_t* outside,
                              const uint64_t* words, const int64_t* stamps, const int64_t* dropped) {
    return count_args_ok(events, n, j0, N, fs, C, 1, image, outside) && window_ok(w, fs) && words && stamps && dropped &&
           row_slots_ok(K) && layout_ok(layout) && fs_us_ok(fs) && layout_fits(layout, C);
}

inline void list_ring_host(const uint64_t* events, int64_t n, int64_t j0, int32_t N, double fs, int32_t C,
                           const Window& w, int32_t K, int32_t layout, int32_t* image, int64_t* outside,
                           uint64_t* words, int64_t* stamps, int64_t* dropped) {
    for (int64_t p = 0; p < n; ++p) {
        const pkt::Stamp st = pkt::decode(events[p], j0);
        const int64_t k = ring_cell(st, C, N, (int64_t)fs, w);
        if (k < 0) {
            ++outside[-1 - k];
            continue;
        }
        const uint32_t slot = (uint32_t)image[k];
        image[k] = (int32_t)(slot + 1);
        if (slot < (uint32_t)K) {
            words[k * K + slot] = row_word(events[p], microsecond(st.jg, N, (int64_t)fs), layout);
            stamps[k * K + slot] = st.jg;
        } else {
            ++dropped[0];
        }
    }
}

inline bool list_args_ok(const uint64_t* events, int64_t n, int64_t j0, int32_t N, double fs, int32_t C,
                         int32_t n_seconds, int32_t K, int32_t layout, const int32_t* image, const int64_t* outside,
                         const uint64_t* words, const int64_t* stamps, const int64_t* dropped) {
    return seconds_ok(n_seconds) &&
           list_ring_args_ok(events, n, j0, N, fs, C, whole(n_seconds), K, layout, image, outside, words, stamps, dropped);
}

inline void list_host(const uint64_t* events, int64_t n, int64_t j0, int32_t N, double fs, int32_t C,
                      int32_t n_seconds, int32_t K, int32_t layout, int32_t* image, int64_t* outside,
                      uint64_t* words, int64_t* stamps, int64_t* dropped) {
    list_ring_host(events, n, j0, N, fs, C, whole(n_seconds), K, layout, image, outside, words, stamps, dropped);
}

inline bool fill_ring_args_ok(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int32_t N,
                              double fs, int32_t C, const Window& w, int32_t K, const int32_t* image,
                              const int64_t* stamps, const float* row_height, const int64_t* fill) {
    return image && stamps && row_height && fill && (n == 0 || (events && heights)) && n >= 0 && C >= 1 && C <= 4096 &&
           window_ok(w, fs) && row_slots_ok(K) && fs_us_ok(fs) && j0_ok(j0, N);
}

inline bool fill_args_ok(const uint64_t* events, const float* heights, int64_t n, int64_t j0, int32_t N, double fs,
                         int32_t C, int32_t n_seconds, int32_t K, const int32_t* image, const int64_t* stamps,
                         const float* row_height, const int64_t* fill) {
    return seconds_ok(n_seconds) &&
           fill_ring_args_ok(events, heights, n, j0, N, fs, C, whole(n_seconds), K, image, stamps, row_height, fill);
}

// A height (and dt) is copied as its 32-bit pattern: a NaN keeps its payload.
OBS_HD void copy_bits(float* dst, const float* src) { __builtin_memcpy(dst, src, sizeof(float)); }

inline void fill_ring_host(const uint64_t* events, const float* heights, const float* dt, int64_t n, int64_t j0,
                           int64_t j_defer, int32_t N, double fs, int32_t C, const Window& w, int32_t K,
                           const int32_t* image, const int64_t* stamps, float* row_height, float* row_dt,
                           int64_t* fill) {
    for (int64_t p = 0; p < n; ++p) {
        const pkt::Stamp st = pkt::decode(events[p], j0);
        if (st.ch >= C || deferred(heights[p], st.jg, j_defer)) continue;
        const int64_t k = ring_cell(st, C, N, (int64_t)fs, w);
        const int64_t at = k < 0 ? -1 : find_stamp(stamps + k * K, row_fill(image[k], K), st.jg);
        if (at < 0) {
            ++fill[1];
            continue;
        }
        copy_bits(row_height + k * K + at, heights + p);
        if (dt && row_dt) copy_bits(row_dt + k * K + at, dt + p);
        ++fill[0];
    }
}

inline void fill_host(const uint64_t* events, const float* heights, const float* dt, int64_t n, int64_t j0,
                      int64_t j_defer, int32_t N, double fs, int32_t C, int32_t n_seconds, int32_t K,
                      const int32_t* image, const int64_t* stamps, float* row_height, float* row_dt, int64_t* fill) {
    fill_ring_host(events, heights, dt, n, j0, j_defer, N, fs, C, whole(n_seconds), K, image, stamps, row_height,
                   row_dt, fill);
}

// ---- a settled second out of its slot (mkid_pack_second) and the slot made free (mkid_clear_second)
// PacketMaster's hand-over of a finished second (PacketMaster.c:329-368, write_sec_data 978-1050):
// the rows of slot sec mod n_slots, each cut to its row_fill, laid end to end in pixel order.
constexpr uint32_t kNanBits = 0x7FC00000u;   // the NaN the height and dt tables are pre-filled with
OBS_HD int64_t slot_of(int64_t sec, int32_t n_slots) { return sec % n_slots; }

inline bool clear_args_ok(int64_t sec, int32_t n_slots, int32_t K, int32_t C, const int32_t* image,
                          const float* row_height) {
    return image && row_height && sec >= 0 && n_slots >= 1 && n_slots <= kMaxSlots && row_slots_ok(K) && C >= 1 &&
           C <= 4096;
}

inline bool pack_args_ok(int64_t sec, int32_t n_slots, int32_t K, int32_t C, const int32_t* image,
                         const uint64_t* words, const int64_t* stamps, const float* row_height, const float* row_dt,
                         int64_t cap_out, const int32_t* counts, const int64_t* offsets, const uint64_t* out_words,
                         const int64_t* out_stamps, const float* out_height, const float* out_dt, const int64_t* total) {
    return clear_args_ok(sec, n_slots, K, C, image, row_height) && words && counts && offsets && total && cap_out >= 0 &&
           (cap_out == 0 || (out_words && out_height)) && (!out_stamps || stamps) && (!out_dt || row_dt);
}

inline void pack_host(int64_t sec, int32_t n_slots, int32_t K, int32_t C, const int32_t* image, const uint64_t* words,
                      const int64_t* stamps, const float* row_height, const float* row_dt, int64_t cap_out,
                      int32_t* counts, int64_t* offsets, uint64_t* out_words, int64_t* out_stamps, float* out_height,
                      float* out_dt, int64_t* total) {
    const int64_t row0 = slot_of(sec, n_slots) * C;
    int64_t off = 0;
    for (int32_t c = 0; c < C; ++c) {
        const int64_t m = row_fill(image[row0 + c], K), src = (row0 + c) * K;
        counts[c] = image[row0 + c];
        offsets[c] = off;
        for (int64_t i = 0; i < m && off + i < cap_out; ++i) {
            out_words[off + i] = words[src + i];
            if (out_stamps) out_stamps[off + i] = stamps[src + i];
            copy_bits(out_height + off + i, row_height + src + i);
            if (out_dt) copy_bits(out_dt + off + i, row_dt + src + i);
        }
        off += m;
    }
    offsets[C] = off;
    total[0] = off;
    total[1] = off < cap_out ? off : cap_out;
}

inline void clear_host(int64_t sec, int32_t n_slots, int32_t K, int32_t C, int32_t* image, float* row_height,
                       float* row_dt) {
    const int64_t row0 = slot_of(sec, n_slots) * C;
    for (int32_t c = 0; c < C; ++c) {
        const int64_t m = row_fill(image[row0 + c], K), at = (row0 + c) * K;
        for (int64_t i = 0; i < m; ++i) {
            __builtin_memcpy(row_height + at + i, &kNanBits, 4);
            if (row_dt) __builtin_memcpy(row_dt + at + i, &kNanBits, 4);
        }
        image[row0 + c] = 0;
    }
}

}  // namespace obs
}  // namespace mkid
