// CPU fuzz driver for the host planning code (mkids_sdr_amd/csrc/mkid_plan.cpp) and the oracle
// trigger (oracle/trigger.c), built with -fsanitize=address,undefined by
// `make -C mkids_sdr_amd/csrc asan` and run by tests/test_asan.py. Every check is an invariant the
// device code relies on (include/mkidgpu.h); the slot-table writes are replayed into
// buffers of exactly the planned size, so an undersized plan is an ASan heap overflow, not a
// silent miscount (the ADVICE r02 scratch-sizing bug is that class).
// fuzz_observe, fuzz_photons and fuzz_pack drive the observing rules and the host twins' loops
// (csrc/obs_common.h) likewise, fuzz_pkt the packet list's host side (csrc/pkt_common.h),
// fuzz_wavecal those of the laser-line calibration and the energy cube (csrc/wavecal_common.h),
// fuzz_loopfit the resonator loop fits (csrc/loopfit_common.h), fuzz_magfit the resonator magnitude
// fits (csrc/magfit_common.h), fuzz_welch the Welch transforms' index maps and the IQ noise analysis
// (csrc/welch_common.h).
//   plan_fuzz [iterations] [seed]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "fit_common.h"
#include "loopfit_common.h"
#include "magfit_common.h"
#include "mkid_plan.h"
#include "obs_common.h"
#include "pkt_common.h"
#include "wavecal_common.h"
#include "welch_common.h"

extern "C" {
typedef struct {
    int32_t B, binit, st, cnt, f1, f2, pad0, pad1;
    int64_t low, band;
} trig_state;
void oracle_trig_reset_state(trig_state* st, int32_t C);
int64_t oracle_trigger(const int16_t* raw, int64_t J, int32_t C, const int16_t* taps, const int32_t* thr,
                       const int32_t* rearm, int32_t mode,
                       int32_t alpha, int32_t kf, int32_t kq, int32_t base_thr, int32_t dead, int16_t* hist,
                       trig_state* st, int64_t j0, uint64_t* ev, int64_t cap, int64_t* counts);
}

using namespace mkid::plan;

static int failures = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            if (++failures > 20) exit(1);                       \
        }                                                       \
    } while (0)

static std::mt19937_64 rng;
static int64_t rint_(int64_t lo, int64_t hi) { return std::uniform_int_distribution<int64_t>(lo, hi)(rng); }

// workspace sizing + call plans for random geometries and ragged calls; the kernels' slot-table
// writes ([C][nseg][capseg], per (channel, segment) at most seg_capacity(L) packets; fix-up scratch
// [C][capseg]) are replayed into exactly-sized buffers
static void fuzz_plans(int iters) {
    const int Cs[] = {64, 128, 256, 512, 1024, 2048};
    const int deads[] = {0, 1, 5, 32, 200};
    for (int it = 0; it < iters; ++it) {
        mkid_cfg cfg{};
        cfg.n_channels = Cs[rint_(0, 5)];
        cfg.fft_len = 2 * cfg.n_channels;
        const int C = cfg.n_channels, N = cfg.fft_len;
        cfg.pfb_taps = 4;
        cfg.fir_taps = 26;
        cfg.dds_entries = 65536 / C;
        cfg.dead_time = deads[rint_(0, 4)];
        const int me = (int)rint_(0, 3);
        cfg.max_events_per_ch = me == 0 ? 0 : (me == 1 ? 1 : (me == 2 ? 3 : (int)rint_(1, 5000)));
        // max_chunk: small (a few rows) to large (2^27 samples), sized so the replay stays small
        const int64_t rows_max = rint_(0, 3) == 0 ? rint_(1, 64) : rint_(1, std::max<int64_t>(1, (1 << 26) / N));
        cfg.max_chunk = rows_max * N;
        const int64_t trig_slots = rint_(0, 2) == 0 ? rint_(1, 64) : rint_(1, 40000);
        const int64_t svf_lanes = rint_(0, 2) == 0 ? rint_(1, 100) : (rint_(0, 1) ? 256 * 256 : 256 * 128);
        const int64_t svf_w = 26 * rint_(1, 4000);
        Workspace ws;
        const char* e = size_workspace(cfg, trig_slots, svf_lanes, svf_w, ws);
        CHECK(e == nullptr, "size_workspace failed: %s", e);
        if (e) continue;
        CHECK(ws.nseg_max >= 1 && ws.slot_cap > 0 && ws.scratch_cap > 0, "table sizes");
        for (int call = 0; call < 6; ++call) {
            const int mode = (int)rint_(0, 2);
            // ragged calls: one row, all rows, a random count, one past the end
            int64_t rows;
            switch (call) {
                case 0: rows = 1; break;
                case 1: rows = rows_max; break;
                case 5: rows = rows_max + rint_(1, 3); break;
                default: rows = rint_(1, rows_max);
            }
            const int64_t n = rows * N;
            TrigPlan p{};
            const char* pe = plan_call(ws, C, N, mode, cfg.dead_time, n, p);
            if (n > cfg.max_chunk) {
                CHECK(pe != nullptr, "a call longer than max_chunk was planned");
                continue;
            }
            CHECK(pe == nullptr, "plan_call failed: %s (C %d rows %lld mode %d)", pe, C, (long long)rows, mode);
            if (pe) continue;
            CHECK(p.J == rows && p.J <= ws.Jmax, "the plan covers %lld of %lld rows", (long long)p.J, (long long)rows);
            CHECK(p.nseg >= 1 && p.nseg <= ws.nseg_max, "nseg %d of %lld", p.nseg, (long long)ws.nseg_max);
            CHECK(p.L >= 1 && (int64_t)(p.nseg - 1) * p.L < p.J && (int64_t)p.nseg * p.L >= p.J,
                  "segments do not tile J: J %lld L %d nseg %d", (long long)p.J, p.L, p.nseg);
            CHECK(p.W >= 0 && p.W % 26 == 0, "warm-up %d", p.W);
            CHECK(p.nseg == 1 || p.L % 26 == 0, "segment starts off the 26-sample ring");
            CHECK(p.capseg >= seg_capacity(p.L, cfg.dead_time), "capseg");
            CHECK((int64_t)C * p.nseg * p.capseg <= ws.slot_cap, "slot table");
            CHECK(p.capseg <= ws.scratch_cap, "scratch");
            // replay the writes into exactly-sized tables (ASan catches any overrun)
            if (ws.slot_cap <= (int64_t)1 << 22 && (int64_t)C * ws.scratch_cap <= (int64_t)1 << 22) {
                std::vector<uint8_t> slots((size_t)ws.slot_cap), scratch((size_t)(C * ws.scratch_cap));
                const int64_t ch[] = {0, C - 1, rint_(0, C - 1)};
                for (int64_t c : ch)
                    for (int32_t s = 0; s < p.nseg; s += std::max<int32_t>(1, p.nseg - 1)) {
                        const int64_t base = (c * p.nseg + s) * (int64_t)p.capseg;
                        for (int32_t k = 0; k < p.capseg; k += std::max<int32_t>(1, p.capseg - 1))
                            slots[(size_t)(base + k)] = 1;
                        for (int32_t k = 0; k < p.capseg; k += std::max<int32_t>(1, p.capseg - 1))
                            scratch[(size_t)(c * p.capseg + k)] = 1;
                    }
            }
        }
    }
}

// Sizing-only pass at the bench's scale: max_chunk up to 2^31 samples and the trigger
// slot / SVF lane counts of an MI355X (256 CUs; k_trig_spec at 4 blocks of 4 waves per CU; one SVF
// segment per two SIMD lanes), so SVF segments longer than the EMA segment the slot table was sized
// from are planned too. Every legal call (n <= max_chunk, n a multiple of N) must be accepted; no
// buffers are replayed (they would be GiB).
static void fuzz_sizing(int iters) {
    const int Cs[] = {256, 1024, 2048};
    const int deads[] = {0, 32, 200};
    const int64_t trig_slots = 256 * 4 * 4, svf_lanes = 256 * 256;   // an MI355X (mkid_api.hip)
    for (int it = 0; it < iters; ++it) {
        mkid_cfg cfg{};
        cfg.n_channels = Cs[rint_(0, 2)];
        cfg.fft_len = 2 * cfg.n_channels;
        const int C = cfg.n_channels, N = cfg.fft_len;
        cfg.pfb_taps = 4;
        cfg.fir_taps = 26;
        cfg.dds_entries = 65536 / C;
        cfg.dead_time = deads[rint_(0, 2)];
        cfg.max_events_per_ch = rint_(0, 1) ? 0 : (int)rint_(1, 5000);
        const int64_t rows_max = rint_(1, ((int64_t)1 << rint_(20, 31)) / N);
        cfg.max_chunk = rows_max * N;
        Workspace ws;
        const char* e = size_workspace(cfg, trig_slots, svf_lanes, kSvfW, ws);
        CHECK(e == nullptr, "size_workspace failed at max_chunk %lld: %s", (long long)cfg.max_chunk, e);
        if (e) continue;
        for (int call = 0; call < 8; ++call) {
            const int mode = call % 3;
            const int64_t rows = call < 3 ? rows_max : rint_(1, rows_max);
            TrigPlan p{};
            const char* pe = plan_call(ws, C, N, mode, cfg.dead_time, rows * N, p);
            CHECK(pe == nullptr, "legal call refused: %s (C %d rows %lld of %lld, mode %d, dead %d)", pe, C,
                  (long long)rows, (long long)rows_max, mode, cfg.dead_time);
            if (pe) continue;
            CHECK((int64_t)C * p.nseg * p.capseg <= ws.slot_cap && p.capseg <= ws.scratch_cap, "tables");
        }
    }
}

// seg_capacity is a hard bound: the oracle trigger, driven to fire as often as it can, never puts
// more than seg_capacity(L, dead) packets of a channel into any window of L rows
static void fuzz_capacity(int iters) {
    for (int it = 0; it < iters; ++it) {
        const int C = (int)rint_(1, 8);
        const int64_t J = rint_(30, 3000);
        const int dead = (int)rint_(0, 40);
        const int mode = (int)rint_(0, 2);
        std::vector<int16_t> raw((size_t)(J * C)), taps((size_t)C * 26, 0), hist((size_t)25 * C, 0);
        std::vector<int32_t> thr(C), rearm(C);
        const int64_t q8 = rint_(0, 256);         // re-arm hysteresis (mkid_set_rearm)
        for (int c = 0; c < C; ++c) {
            taps[(size_t)c * 26] = 2047;          // identity matched filter: f = raw * 2047 >> 11
            thr[c] = (int32_t)rint_(-3000, 3000);
            rearm[c] = rearm_level(thr[c], (int32_t)q8);
        }
        const int kind = (int)rint_(0, 2);
        for (int64_t j = 0; j < J; ++j)
            for (int c = 0; c < C; ++c) {
                int v;
                if (kind == 0) v = (int)rint_(-32768, 32767);                         // noise
                else if (kind == 1) v = (j % 2) ? 20000 : -20000;                       // fastest cycling
                else v = (int)((j % (dead + 3)) == 0 ? -25000 : 25000) + (int)rint_(-50, 50);
                raw[(size_t)(j * C + c)] = (int16_t)v;
            }
        std::vector<trig_state> st(C);
        oracle_trig_reset_state(st.data(), C);
        const int64_t cap = J * C;
        std::vector<uint64_t> ev((size_t)cap);
        std::vector<int64_t> counts(C);
        const int64_t total = oracle_trigger(raw.data(), J, C, taps.data(), thr.data(), rearm.data(), mode, 41, 82, 93623,
                                             mode ? 8192 : 0, dead, hist.data(), st.data(), 0, ev.data(), cap,
                                             counts.data());
        CHECK(total <= cap, "trigger overflowed its own bound");
        // per channel: rows of its packets (ts = j - 1), every window of L rows
        std::vector<std::vector<int64_t>> rows(C);
        for (int64_t i = 0; i < std::min(total, cap); ++i) {
            const int c = (int)((ev[(size_t)i] >> MKID_PKT_CH_SHIFT) & 0xFFF);
            CHECK(c < C, "channel field");
            if (c < C) rows[c].push_back((int64_t)(ev[(size_t)i] & ((1ull << 28) - 1)));
        }
        for (int c = 0; c < C; ++c) {
            CHECK(counts[c] <= seg_capacity(J, dead), "whole-call bound: %lld > %lld", (long long)counts[c],
                  (long long)seg_capacity(J, dead));
            const std::vector<int64_t>& r = rows[c];
            CHECK(std::is_sorted(r.begin(), r.end()), "time order");
            for (int k = 0; k < 4 && !r.empty(); ++k) {
                const int64_t L = rint_(1, J);
                for (size_t a = 0; a < r.size(); ++a) {
                    const size_t b = std::upper_bound(r.begin(), r.end(), r[a] + L - 1) - r.begin();
                    CHECK((int64_t)(b - a) <= seg_capacity(L, dead), "window of %lld rows holds %lld > %lld",
                          (long long)L, (long long)(b - a), (long long)seg_capacity(L, dead));
                }
            }
        }
    }
}

static void fuzz_slot_order(int iters) {
    const int Cs[] = {64, 1024, 2048, 1024, 2048};
    for (int it = 0; it < iters; ++it) {
        const int C = Cs[rint_(0, 4)], N = 2 * C;
        std::vector<int32_t> bins(C);
        const int kind = (int)rint_(0, 2);
        for (int i = 0; i < C; ++i)
            bins[i] = kind == 0 ? (int32_t)rint_(0, N - 1) : (kind == 1 ? (int32_t)(i * 7 % N) : (int32_t)rint_(0, 3));
        std::vector<int16_t> so;
        slot_order(bins, C, so);
        std::vector<int> seen(C, 0);
        bool perm = (int)so.size() == C;
        for (int16_t v : so) perm = perm && v >= 0 && v < C && !seen[v]++;
        CHECK(perm, "slot order is not a permutation (C %d)", C);
        if (C == 1024 && perm)   // k_front3: wave w keeps channels 128 w .. 128 w + 127
            for (int slot = 0; slot < C; ++slot) {
                const int st = slot % (C / 2), w = st / 64;
                CHECK(so[slot] / 128 == w, "slot %d of wave %d holds channel %d", slot, w, so[slot]);
            }
        if (C == 2048 && perm)   // the k_front5 layout: each wave keeps the channels of its slots
            for (int slot = 0; slot < C; ++slot) {
                const int wave = slot < 1536 ? (slot % 512) / 64 : 8 + ((slot - 1536) % 256) / 64;
                const int ch = so[slot];
                const int cw = ch < 1536 ? (ch % 512) / 64 : 8 + ((ch - 1536) % 256) / 64;
                CHECK(cw == wave, "slot %d of wave %d holds channel %d", slot, wave, ch);
            }
    }
}

static void fuzz_quantize(int iters) {
    for (int it = 0; it < iters; ++it) {
        const int T = 4, N = (int)(1 << rint_(3, 12));
        std::vector<float> h((size_t)T * N);
        const int kind = (int)rint_(0, 3);
        const double scale = kind == 0 ? 1e-3 : (kind == 1 ? 1.0 : (kind == 2 ? 1e6 : 1e-30));
        for (float& v : h) v = (float)(std::uniform_real_distribution<double>(-1, 1)(rng) * scale);
        if (rint_(0, 5) == 0) std::fill(h.begin(), h.end(), 0.f);
        std::vector<int16_t> hq;
        const int S = quantize_pfb(h.data(), T, N, hq);
        CHECK((int)hq.size() == T * N && S >= -64 && S <= 64, "quantize geometry S %d", S);
        if (S > -64)
            for (int p = 0; p < N; ++p) {
                int64_t sp = 0;
                for (int t = 0; t < T; ++t) sp += std::abs((int64_t)hq[(size_t)t * N + p]);
                CHECK(sp <= 65535, "point %d tap sum %lld", p, (long long)sp);
            }
    }
}

static void fuzz_merge_pack(int iters) {
    for (int it = 0; it < iters; ++it) {
        const int C = (int)rint_(1, 300), nchunk = (int)rint_(1, 5);
        std::vector<uint64_t> ev;
        int64_t t0 = 0;
        for (int k = 0; k < nchunk; ++k) {   // each chunk channel-major, time-ascending
            for (int c = 0; c < C; ++c) {
                const int m = (int)rint_(0, 3);
                for (int i = 0; i < m; ++i)
                    ev.push_back(((uint64_t)c << MKID_PKT_CH_SHIFT) | ((uint64_t)rint_(0, 4095) << MKID_PKT_PEAK_SHIFT) |
                                 ((uint64_t)rint_(0, 4095) << MKID_PKT_BASE_SHIFT) | (uint64_t)(t0 + 10 * k + i));
            }
            t0 += 1000;
        }
        std::vector<uint64_t> m = ev;
        merge_channel_major(m.data(), (int64_t)m.size());
        bool ok = std::is_permutation(m.begin(), m.end(), ev.begin());
        for (size_t i = 1; i < m.size() && ok; ++i) {
            const uint64_t ca = m[i - 1] >> MKID_PKT_CH_SHIFT, cb = m[i] >> MKID_PKT_CH_SHIFT;
            ok = ca < cb || (ca == cb && (m[i - 1] & 0xFFFFFFF) < (m[i] & 0xFFFFFFF));
        }
        CHECK(ok, "merge is not channel-major / time-ascending");
        std::vector<uint64_t> out(m.size());
        const int r = pack_reference(m.data(), (int64_t)m.size(), out.data());
        uint64_t cmax = 0;
        for (uint64_t w : m) cmax = std::max<uint64_t>(cmax, w >> MKID_PKT_CH_SHIFT);
        CHECK((r == 0) == (m.empty() || cmax < 255), "pack_reference accepts exactly channels < 255 (max %llu, r %d)",
              (unsigned long long)cmax, r);
        if (r == 0)
            for (size_t i = 0; i < m.size(); ++i)
                CHECK((out[i] >> 56) == (m[i] >> MKID_PKT_CH_SHIFT) && (out[i] & 0xFFFFF) == (m[i] & 0xFFFFF),
                      "packed fields");
    }
}

// The packet list's host side (pkt_common.h): the valid count, the slices and their bounds (disjoint,
// in order, covering exactly the first `valid` packets, at most kObsMaxBlocks of them), the grid of a
// grid-stride pass, and the run ends' deltas, which must add up to every run's length.
static void fuzz_pkt(int iters) {
    using namespace mkid::pkt;
    for (int it = 0; it < iters; ++it) {
        const int64_t n = rint_(0, 3) == 0 ? rint_(0, 600) : rint_(0, (int64_t)1 << rint_(10, 33));
        const int64_t dn = rint_(0, 2) == 0 ? rint_(-5, 5) : rint_(-n - 5, n + 5);
        const int64_t valid = count(&dn, n);
        CHECK(count(nullptr, n) == n && valid == std::min(std::max<int64_t>(dn, 0), n), "count %lld of %lld",
              (long long)dn, (long long)n);
        const int32_t threads = (int32_t)(64 * rint_(1, 16));
        const Slices p = slices(n, threads);
        CHECK(p.blocks >= 1 && p.blocks <= mkid::kObsMaxBlocks && p.slice % threads == 0 && p.blocks * p.slice >= n &&
                  (p.blocks == mkid::kObsMaxBlocks || p.slice <= mkid::kObsSlice + threads),
              "slices of %lld: %d x %lld", (long long)n, p.blocks, (long long)p.slice);
        int64_t at = 0;
        for (int32_t b = 0; b < p.blocks; ++b) {
            int64_t b0, b1;
            bounds(b, p.slice, valid, b0, b1);
            if (b0 >= b1) continue;   // the count ended before this slice
            CHECK(b0 == at && b1 <= valid, "slice %d of %lld: [%lld, %lld)", b, (long long)valid, (long long)b0, (long long)b1);
            at = b1;
        }
        CHECK(at == valid, "the slices cover %lld of %lld", (long long)at, (long long)valid);
        const int32_t ncu = (int32_t)rint_(-1, 400), per = (int32_t)rint_(1, 32);
        const int64_t g = grid_stride_blocks(n, threads, ncu, per);
        CHECK(g >= 0 && g <= (int64_t)(ncu > 0 ? ncu : 256) * per && g * threads < n + threads && (g > 0) == (n > 0),
              "grid %lld for %lld", (long long)g, (long long)n);
        uint64_t sum = 0;   // runs of random length from a random start
        int64_t i = rint_(0, (int64_t)1 << 40), runs = rint_(1, 20), total = 0;
        for (int64_t r = 0; r < runs; ++r) {
            const int64_t len = rint_(1, 5);
            for (int64_t k = 0; k < len; ++k, ++i)
                if (k == 0 || k == len - 1) sum += run_delta(i, k == 0, k == len - 1);
            total += len;
        }
        CHECK(sum == (uint64_t)total, "run deltas add up to %llu of %lld", (unsigned long long)sum, (long long)total);
    }
}

// Carry (the validity bookkeeping of a carried history, pulse heights and capture) against a model
// that remembers which global row each row of the H-row buffer holds: calls of random length
// (0 included) that continue the stream, break it (a j0 that does not continue) or follow a drop().
// before(j0) must be the run of rows ..., j0 - 2, j0 - 1 at the buffer's end, offset(j0) its start.
static void fuzz_carry(int iters) {
    for (int it = 0; it < iters; ++it) {
        const int64_t H = rint_(1, 40);
        Carry k{H};
        std::vector<int64_t> buf((size_t)H, -1);   // global row held by each buffer row (-1: none)
        int64_t next = rint_(0, 1000);
        for (int call = 0; call < 30; ++call) {
            const int what = (int)rint_(0, 9);
            if (what == 0) {
                k.drop();
                std::fill(buf.begin(), buf.end(), -1);   // a drop forgets the rows even if j0 continues
            }
            const int64_t j0 = what == 1 ? next + rint_(1, 50) : (what == 2 ? std::max<int64_t>(0, next - rint_(1, 50)) : next);
            const int64_t n = rint_(0, 3) == 0 ? 0 : rint_(1, 2 * H + 3);
            int64_t want = 0;
            while (want < H && buf[(size_t)(H - 1 - want)] >= 0 && buf[(size_t)(H - 1 - want)] == j0 - 1 - want) ++want;
            CHECK(k.before(j0) == want, "before(%lld) = %lld, model %lld (H %lld)", (long long)j0,
                  (long long)k.before(j0), (long long)want, (long long)H);
            CHECK(k.offset(j0) == H - want && k.offset(j0) >= 0 && k.offset(j0) <= H, "offset(%lld) = %lld",
                  (long long)j0, (long long)k.offset(j0));
            // the roll: the last H of (the rows valid before j0, the n new rows); n = 0 does not roll,
            // but a call that broke the stream still starts a new one at j0 (capture's empty call)
            std::vector<int64_t> all;
            for (int64_t i = H - want; i < H; ++i) all.push_back(buf[(size_t)i]);
            for (int64_t i = 0; i < n; ++i) all.push_back(j0 + i);
            std::fill(buf.begin(), buf.end(), -1);
            for (int64_t i = 0; i < H && i < (int64_t)all.size(); ++i) buf[(size_t)(H - 1 - i)] = all[all.size() - 1 - (size_t)i];
            k.advance(j0, n);
            CHECK(k.end == j0 + n && k.rows == std::min<int64_t>(H, want + n), "advance: end %lld rows %lld",
                  (long long)k.end, (long long)k.rows);
            next = j0 + n;
        }
    }
}

// table extents of a plan for R records per channel: offset + group * per-channel bytes (sizes of
// BankArgs in mkid_internal.h), ascending, aligned, inside `bytes`; the last slot of every table is
// written into a buffer of exactly the planned size when that is small
static void check_bank_tables(const BankWs& w, int64_t R) {
    const int64_t off[15] = {w.rows, w.nrows, w.peaks, w.scratch, w.tP,       w.tPf,    w.noise, w.stats,
                             w.work, w.coeff, w.refmed, w.accept, w.appended, w.status, w.nready};
    const int64_t per[15] = {R * 16000, R * 6400, R * 8, (2 * R + 8) * 8, 16000, 16000, 6400, 64,
                             19200,     6400,     8,     R * 4,           R * 4, 4,     4};
    int64_t sum = 0;
    for (int i = 0; i < 15; ++i) {
        sum += per[i];
        CHECK(off[i] % kBankAlign == 0 && off[i] + w.group * per[i] <= (i < 14 ? off[i + 1] : w.bytes),
              "table %d overlaps the next", i);
    }
    CHECK(off[0] == 0 && sum == w.channel_bytes, "channel bytes %lld, tables %lld", (long long)w.channel_bytes,
          (long long)sum);
    if (w.bytes <= (1 << 22)) {
        std::vector<char> buf((size_t)w.bytes);
        for (int i = 0; i < 15; ++i) buf[(size_t)(off[i] + w.group * per[i] - 1)] = 1;
    }
}

// plan_bank (the workspace of mkid_bank_filters and mkid_make_template): group >= 1, the workspace
// within the budget whenever one channel fits, the groups covering 0..Cb-1 once, and the tables of
// the bank's plan and of the one-channel plan that mkid_make_template asks for
static void fuzz_bank(int iters) {
    int over = 0;
    for (int it = 0; it < iters; ++it) {
        const int64_t Cb = rint_(0, 3) == 0 ? rint_(1, 4) : rint_(1, 100000);
        const int64_t R = rint_(0, 3) == 0 ? rint_(1, 8) : (rint_(0, 5) == 0 ? rint_(1, 3000000) : rint_(1, 1200));
        const int64_t budget = rint_(0, 4) == 0 ? rint_(0, 100000) : (rint_(0, 1) ? kBankBudget : rint_(1, 1ll << 32));
        const int64_t want = rint_(0, 1) ? 0 : rint_(1, 2 * Cb);
        const BankWs w = plan_bank(Cb, R, budget, want);
        const BankWs one = plan_bank(1, R, budget, 0);
        CHECK(w.group >= 1 && w.group <= Cb && w.group <= kBankMaxGroup, "group %lld of %lld", (long long)w.group,
              (long long)Cb);
        CHECK(want == 0 || w.group <= want, "group %lld above the request %lld", (long long)w.group, (long long)want);
        CHECK(one.group == 1 && w.bytes >= one.bytes, "one channel: group %lld", (long long)one.group);
        if (one.bytes <= budget)
            CHECK(w.bytes <= budget, "bytes %lld over the budget %lld (Cb %lld R %lld)", (long long)w.bytes,
                  (long long)budget, (long long)Cb, (long long)R);
        else
            CHECK(w.group == 1, "group %lld although one channel does not fit", (long long)w.group);
        std::vector<int32_t> seen((size_t)Cb, 0);
        for (int64_t c0 = 0; c0 < Cb; c0 += w.group)
            for (int64_t b = 0; b < std::min(w.group, Cb - c0); ++b) ++seen[(size_t)(c0 + b)];
        CHECK(std::all_of(seen.begin(), seen.end(), [](int32_t n) { return n == 1; }), "groups do not cover the bank once");
        check_bank_tables(w, R);
        // mkid_make_template's request: one channel of R = P pulses at the product's budget, which
        // one channel alone exceeds from R = 11 964 on
        const BankWs tpl = plan_bank(1, R, kBankBudget);
        CHECK(tpl.group == 1 && tpl.bytes >= tpl.channel_bytes &&
                  tpl.bytes <= tpl.channel_bytes + 15 * (kBankAlign - 1),
              "make_template: group %lld, %lld bytes for R %lld", (long long)tpl.group, (long long)tpl.bytes,
              (long long)R);
        over += tpl.bytes > kBankBudget;
        check_bank_tables(tpl, R);
    }
    CHECK(iters < 100 || over > 0, "no one-channel plan above the budget in %d iterations", iters);
}

// plan_thresholds (mkid_phase_thresholds): the row blocks cover the rows once, the two launches'
// strips cover the channels once with whole 8-channel threads in the vector launch, the jobs of a
// small block replayed as the kernels decode them touch every sample once and stay inside the
// block, and the workspace tables lie inside `bytes` without overlap.
static void fuzz_thresholds(int iters) {
    for (int it = 0; it < iters; ++it) {
        const bool small = rint_(0, 1) == 0;
        const int64_t rows = small ? rint_(1, 700) : (rint_(0, 3) == 0 ? rint_(1, (1ll << 31) - 1) : rint_(1, 20000));
        const int32_t nch = (int32_t)(small ? rint_(1, 200) : (rint_(0, 3) == 0 ? rint_(1, (1ll << 31) - 1) : rint_(1, 5000)));
        const int64_t ld = std::min<int64_t>((int64_t)nch + (rint_(0, 1) ? 0 : rint_(0, 40)), (1ll << 31) - 1);
        const bool aligned = rint_(0, 2) != 0;
        const int ncu = (int)rint_(1, 512);
        const ThrPlan p = plan_thresholds(rows, ld, nch, aligned, ncu);
        CHECK(p.B >= kThrMinB && p.B <= kThrMaxB && p.B % kThrRowStep == 0, "B %lld", (long long)p.B);
        CHECK(p.row_blocks >= 1 && p.row_blocks * p.B >= rows && (p.row_blocks - 1) * p.B < rows,
              "%lld row blocks of %lld for %lld rows", (long long)p.row_blocks, (long long)p.B, (long long)rows);
        CHECK(p.vec == 1 || (p.vec == 8 && aligned && ld % 8 == 0), "vec %d (ld %lld)", p.vec, (long long)ld);
        CHECK(p.nch_vec >= 0 && p.nch_vec <= nch && p.nch_vec % 8 == 0 && (p.vec == 8 || p.nch_vec == 0) &&
                  (p.vec == 1 || nch - p.nch_vec < 8),
              "nch_vec %d of %d", p.nch_vec, nch);
        CHECK(p.strips_vec * kThrStrip >= p.nch_vec && (p.strips_vec == 0 || (p.strips_vec - 1) * kThrStrip < p.nch_vec),
              "vector strips %lld", (long long)p.strips_vec);
        CHECK(p.strips_tail * kThrStrip >= nch - p.nch_vec &&
                  (p.strips_tail == 0 || (p.strips_tail - 1) * kThrStrip < nch - p.nch_vec),
              "tail strips %lld", (long long)p.strips_tail);
        CHECK(p.grid_vec <= kThrMaxGrid && p.grid_tail <= kThrMaxGrid && (p.grid_vec > 0) == (p.strips_vec > 0) &&
                  (p.grid_tail > 0) == (p.strips_tail > 0) && p.grid_vec <= p.strips_vec * p.row_blocks &&
                  p.grid_tail <= p.strips_tail * p.row_blocks,
              "grids %lld %lld", (long long)p.grid_vec, (long long)p.grid_tail);
        CHECK(p.grid_init >= 1 && p.grid_init <= kThrMaxInitGrid && p.grid_finish >= 1 &&
                  p.grid_finish * kThrFinishCh >= nch && (p.grid_finish - 1) * kThrFinishCh < nch,
              "init grid %lld, finish grid %lld for %d channels", (long long)p.grid_init, (long long)p.grid_finish, nch);
        CHECK(p.off_lo == 0 && p.off_hi == p.off_lo + 4ll * nch && p.off_counts == p.off_hi + 4ll * nch &&
                  p.bytes == p.off_counts + 400ll * nch,
              "workspace layout for %d channels", nch);
        if (!small) continue;
        // replay both launches' jobs as k_thresholds.hip's Job decodes them
        std::vector<uint8_t> seen((size_t)(rows * ld), 0);
        for (int launch = 0; launch < 2; ++launch) {
            const int V = launch == 0 ? 8 : 1;
            const int64_t cbeg = launch == 0 ? 0 : p.nch_vec, cend = launch == 0 ? p.nch_vec : nch;
            const int64_t strips = launch == 0 ? p.strips_vec : p.strips_tail;
            if (launch == 0 && p.vec != 8) continue;
            const int cols = kThrStrip / V, rslots = kThrThreads / cols;
            for (int64_t job = 0; job < strips * p.row_blocks; ++job) {
                const int64_t rb = job / strips, st = job - rb * strips;
                const int64_t r0 = rb * p.B, r1 = std::min(r0 + p.B, rows), c0 = cbeg + st * kThrStrip;
                const int64_t nloc = std::min<int64_t>(cend - c0, kThrStrip);
                CHECK(nloc >= 1, "empty strip");
                for (int t = 0; t < kThrThreads; ++t) {
                    const int col = t % cols, rslot = t / cols;
                    if (col * V >= nloc) continue;
                    for (int64_t r = r0 + rslot; r < r1; r += rslots)
                        for (int k = 0; k < V; ++k) ++seen[(size_t)(r * ld + c0 + col * V + k)];   // ASan: in the block
                }
            }
        }
        bool once = true;
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t c = 0; c < ld; ++c) once = once && seen[(size_t)(r * ld + c)] == (c < nch ? 1 : 0);
        CHECK(once, "jobs do not touch every sample of %lld x %d (ld %lld) once", (long long)rows, nch, (long long)ld);
    }
}

// plan_noise (mkid_phase_noise_spectra): for random n and for 1, 2, 233, 10485, 16381 (prime) and
// 16384 the radices multiply to n and the passes chain (L, M, stride, tw_off), the tables have the
// planned sizes, bin_of_pos is a permutation with partner its reflection, the device image is
// written into a buffer of exactly `bytes`, the launch geometry covers n and the channel order is a
// permutation; then the host transform (noise_common.h pair_host, what the kernel does per pair of
// pieces) runs on buffers of exactly n elements and a block of exactly the rows it may read, paired
// and unpaired, and its bins are checked against a direct DFT at a few k. A length whose cost
// n * (sum of radices) is large is replayed only when it is one of the listed ones.
static void check_noise(int32_t n, bool replay) {
    NoisePlan p;
    CHECK(plan_noise(n, p), "no plan for n %d", n);
    if (p.n != n) return;
    int64_t prod = 1, sum = 0, L = n;
    for (const mkid::noise::Pass& ps : p.passes) {
        CHECK(ps.r >= 2 && ps.L == L && ps.M * ps.r == ps.L && ps.stride * ps.L == n && ps.tw_off == sum,
              "pass r %d L %d M %d stride %d tw_off %d (n %d)", ps.r, ps.L, ps.M, ps.stride, ps.tw_off, n);
        prod *= ps.r, sum += ps.r, L /= ps.r;
    }
    CHECK(prod == n && L == 1 && (int)p.passes.size() <= mkid::noise::kMaxPasses, "radices multiply to %lld, n %d",
          (long long)prod, n);
    CHECK((int64_t)p.wn.size() == n && (int64_t)p.wr.size() == sum && (int64_t)p.bin_of_pos.size() == n &&
              (int64_t)p.partner.size() == n,
          "table sizes (n %d)", n);
    std::vector<int> seen((size_t)n, 0);
    bool perm = true;
    for (int32_t pos = 0; pos < n && perm; ++pos) perm = p.bin_of_pos[(size_t)pos] < n && !seen[p.bin_of_pos[(size_t)pos]]++;
    CHECK(perm, "bin_of_pos is not a permutation (n %d)", n);
    for (int32_t pos = 0; pos < n && perm; ++pos) {
        const int32_t q = p.partner[(size_t)pos];
        CHECK(q < n && (p.bin_of_pos[(size_t)pos] + p.bin_of_pos[(size_t)q]) % n == 0, "partner of position %d (n %d)", pos, n);
    }
    CHECK(p.off_wn == 0 && p.off_wr >= 8ll * n && p.off_bin >= p.off_wr + 8 * sum && p.off_partner >= p.off_bin + 2ll * n &&
              p.bytes >= p.off_partner + 2ll * n && p.off_wr % 16 == 0 && p.off_bin % 16 == 0 && p.off_partner % 16 == 0,
          "device image layout (n %d)", n);
    std::vector<char> image((size_t)p.bytes);
    noise_pack_tables(p, image.data());   // ASan: inside `bytes`
    CHECK((int64_t)p.threads * p.per_thread >= n && (p.threads == kNoiseThreadsSmall || p.threads == kNoiseThreadsLarge) &&
              p.lds_bytes == 8ll * n + 8ll * kNoiseStageR + 16ll * (p.threads / 64) && p.lds_bytes <= 160 * 1024,
          "launch geometry (n %d)", n);
    if (!replay) return;
    const int64_t ld = rint_(1, 3), col = rint_(0, ld - 1);
    for (int pieces = 1; pieces <= 2; ++pieces) {
        std::vector<int16_t> raw((size_t)(((int64_t)pieces * n - 1) * ld + col + 1));   // the last row ends at the column
        for (int16_t& v : raw) v = (int16_t)rint_(-25736, 25736);
        std::vector<mkid::noise::Cx<double>> z((size_t)n), y((size_t)n);
        std::vector<double> acc((size_t)n, 0.0);
        const mkid::noise::View<double> v{n, (int32_t)p.passes.size(), p.passes.data(), p.wn.data(), p.wr.data(),
                                          p.bin_of_pos.data(), p.partner.data()};
        std::vector<double> pw((size_t)n * 2);
        int calls = 0;
        mkid::noise::pair_host<double>(v, raw.data() + col, pieces == 2 ? raw.data() + (int64_t)n * ld + col : nullptr, ld,
                                       z.data(), y.data(), acc.data(), [&pw, &calls](double x) {
                                           pw[(size_t)calls++] = x;   // |A[k]|^2 (, |B[k]|^2) in position order
                                           return 0.0;
                                       });
        CHECK(calls == pieces * n, "%d powers for %d pieces of %d", calls, pieces, n);
        for (int probe = 0; probe < 3; ++probe) {   // against the direct DFT
            const int32_t pos = (int32_t)rint_(0, n - 1), k = p.bin_of_pos[(size_t)pos];
            for (int w = 0; w < pieces; ++w) {
                double re = 0, im = 0, tot = 0;
                for (int32_t j = 0; j < n; ++j) {
                    const double x = raw[(size_t)(((int64_t)w * n + j) * ld + col)];
                    const mkid::noise::Cx<double> t = p.wn[(size_t)((int64_t)j * k % n)];
                    re += x * t.re, im += x * t.im, tot += x * x;
                }
                const double got = pw[(size_t)(pos * pieces + w)], want = re * re + im * im;
                CHECK(std::abs(got - want) <= 1e-9 * tot * n + 1e-9, "n %d bin %d piece %d: %g, direct %g", n, k, w, got, want);
            }
        }
    }
}

static void fuzz_noise(int iters) {
    const int32_t listed[] = {1, 2, 233, 10485, 16381, MKID_NOISE_MAX_N};
    for (int32_t n : listed) check_noise(n, true);
    NoisePlan none;
    CHECK(!plan_noise(0, none) && !plan_noise(MKID_NOISE_MAX_N + 1, none) && !plan_noise(-5, none), "n out of range planned");
    for (int it = 0; it < iters; ++it) {
        const int32_t n = (int32_t)(rint_(0, 2) == 0 ? rint_(1, 300) : rint_(1, MKID_NOISE_MAX_N));
        NoisePlan p;
        int64_t cost = 0;
        if (plan_noise(n, p))
            for (const mkid::noise::Pass& ps : p.passes) cost += (int64_t)n * ps.r;
        check_noise(n, cost <= 4000000);
    }
    // the order in which the blocks take the channels: a permutation of 0 .. blocks - 1
    for (int64_t nch : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1024, rint_(1, 5000)}) {
        const int64_t blocks = noise_blocks(nch);
        CHECK(blocks >= nch && blocks % kNoiseXcdSpan == 0 && blocks - nch < kNoiseXcdSpan, "blocks for %lld channels", (long long)nch);
        std::vector<int> seen((size_t)blocks, 0);
        bool ok = true;
        for (int64_t b = 0; b < blocks && ok; ++b) {
            const int64_t c = noise_channel_of_block(b);
            ok = c >= 0 && c < blocks && !seen[(size_t)c]++;
        }
        CHECK(ok, "channel order is not a permutation (%lld channels)", (long long)nch);
    }
}

// plan_fit (mkid_pulse_fit): for random and for boundary (ncoeff, L) the wave's LDS region is laid
// out without overlap, a workgroup's regions stay inside the static 64 KiB, and the kernel's maps,
// replayed as k_heights_fit.hip runs them into a buffer of exactly one wave's region, stay inside
// their tables: the staging writes touch every window row and coefficient once, every (tap, lag)
// pair is read by exactly one lane at window index tap + lag <= W - 1, the partial sums fill 64
// slots of which the sum pass reads G per lag, and fit::select on the nl lag values reads only those
// and returns a lag in -L .. L with |dt - lag| <= 1/2.
static void check_fit(int32_t ncoeff, int32_t L, int ncu) {
    const FitPlan p = plan_fit(ncoeff, L, ncu);
    CHECK(p.nl == 2 * L + 1 && p.G == 64 / p.nl && p.G >= 1 && p.G * p.nl <= 64 && p.W == ncoeff + 2 * L,
          "fit geometry (ncoeff %d, L %d)", ncoeff, L);
    CHECK(p.off_w == 0 && p.off_cf == p.off_w + p.W && p.off_part == p.off_cf + ncoeff && p.off_h == p.off_part + 64 &&
              p.wave_floats == p.off_h + 64,
          "fit region layout (ncoeff %d, L %d)", ncoeff, L);
    CHECK(p.waves >= 1 && p.waves <= kFitWaves && p.lds_bytes == 4ll * p.wave_floats * p.waves &&
              p.lds_bytes <= kFitLdsBytes && (p.waves == kFitWaves || 4ll * p.wave_floats * (p.waves + 1) > kFitLdsBytes),
          "fit workgroup: %d waves, %lld bytes (ncoeff %d, L %d)", p.waves, (long long)p.lds_bytes, ncoeff, L);
    CHECK(p.grid_cap >= 1 && p.blocks(1) == 1 && p.blocks(1ll << 40) == p.grid_cap &&
              p.blocks(p.waves + 1) == std::min<int64_t>(2, p.grid_cap),
          "fit grid (ncu %d)", ncu);
    std::vector<float> region((size_t)p.wave_floats, 0.f);   // ASan: every index below is inside it
    float* w = region.data() + p.off_w;
    float* cf = region.data() + p.off_cf;
    float* part = region.data() + p.off_part;
    float* hv = region.data() + p.off_h;
    for (int lane = 0; lane < 64; ++lane) {
        for (int i = lane; i < p.W; i += 64) w[i] += 1.f;
        for (int i = lane; i < ncoeff; i += 64) cf[i] += 1.f;
    }
    bool once = true;
    for (int i = 0; i < p.W; ++i) once = once && w[i] == 1.f;
    for (int i = 0; i < ncoeff; ++i) once = once && cf[i] == 1.f;
    CHECK(once, "staging does not fill the region once (ncoeff %d, L %d)", ncoeff, L);
    std::vector<int32_t> seen((size_t)ncoeff * p.nl, 0);
    for (int lane = 0; lane < 64; ++lane) {
        const int g = lane / p.nl, d = lane - g * p.nl;
        float acc = 0.f;
        if (g < p.G)
            for (int i = g; i < ncoeff; i += p.G) {
                acc += cf[i] * w[i + d];
                ++seen[(size_t)i * p.nl + d];
            }
        part[lane] = acc;
    }
    CHECK(std::all_of(seen.begin(), seen.end(), [](int32_t n) { return n == 1; }), "taps x lags not covered once (ncoeff %d, L %d)",
          ncoeff, L);
    for (int lane = 0; lane < p.nl; ++lane) {
        float h = part[lane];
        for (int k = 1; k < p.G; ++k) h += part[k * p.nl + lane];
        hv[lane] = h;
        CHECK(h == (float)ncoeff, "lag %d sums %g of %d products", lane - L, h, ncoeff);
    }
    for (int lane = 0; lane < p.nl; ++lane) hv[lane] = (float)rint_(-3, 3);
    for (int s = -1; s <= 1; s += 2) {
        const mkid::fit::Result<float> r = mkid::fit::select<float>(hv, L, s);
        CHECK(r.lag >= -L && r.lag <= L && std::abs(r.dt - (float)r.lag) <= 0.5f && r.h0 == hv[L] &&
                  (float)s * r.height >= (float)s * hv[r.lag + L],
              "select: lag %d dt %g (L %d)", r.lag, r.dt, L);
        for (int d = 0; d < p.nl; ++d)
            CHECK((float)s * hv[d] < (float)s * hv[r.lag + L] || (d >= r.lag + L && hv[d] == hv[r.lag + L]),
                  "select: lag %d is not the lowest maximum (L %d)", r.lag, L);
    }
}

static void fuzz_fit(int iters) {
    for (int32_t L : {0, 1, 2, 3, 8, 10, 15, 16, 21, 31})
        for (int32_t ncoeff : {1, 2, 63, 64, 65, 100, 800, 4095, 4096}) check_fit(ncoeff, L, 256);
    for (int it = 0; it < iters; ++it)
        check_fit((int32_t)(rint_(0, 1) ? rint_(1, 300) : rint_(1, mkid::fit::kMaxCoeff)), (int32_t)rint_(0, mkid::fit::kMaxSearch),
                  (int)rint_(1, 512));
    mkid::pkt::Stamp st = mkid::pkt::decode(((uint64_t)5 << MKID_PKT_CH_SHIFT) | 3, ((int64_t)1 << 28) + 1);
    CHECK(st.ch == 5 && st.jg == ((int64_t)1 << 28) + 3, "decode: channel %d stamp %lld", st.ch, (long long)st.jg);
    CHECK(mkid::fit::inside(0, 1, -3, 3, 10, 6, 10) && !mkid::fit::inside(0, 1, -4, 3, 10, 6, 10) &&
              !mkid::fit::inside(0, 1, -2, 3, 10, 6, 10) && !mkid::fit::inside(1, 1, -3, 3, 10, 6, 10),
          "window test");
}

// The observing rules (obs_common.h) and the loops of the two host twins on random words, heights
// (NaN, +-inf, +-0, bin edges) and shapes, against a plain per-packet restatement; the outputs are
// buffers of exactly the documented sizes, so a column or cell outside them is an ASan report.
static void fuzz_observe(int iters) {
    namespace obs = mkid::obs;
    CHECK(obs::fs_ok(1e6) && obs::fs_ok(1.0) && !obs::fs_ok(1e6 + 0.5) && !obs::fs_ok(0.0) && !obs::fs_ok(-2.0) &&
              !obs::fs_ok(9007199254740992.0) && !obs::fs_ok(NAN) && !obs::fs_ok(INFINITY),
          "fs_ok");
    CHECK(obs::column(-0.0f, 0.f, 1.f, 4) == 1 && obs::column(INFINITY, 0.f, 1.f, 4) == 6 &&
              obs::column(-INFINITY, 0.f, 1.f, 4) == 6 && obs::column(NAN, 0.f, 1.f, 4) == 6 &&
              obs::column(4.f, 0.f, 1.f, 4) == 5 && obs::column(3.9999f, 0.f, 1.f, 4) == 4 &&
              obs::column(-1e-30f, 0.f, 1.f, 4) == 0 && obs::column(1e38f, 0.f, 1e38f, 4) == 5 &&
              obs::column(0.f, 0.f, INFINITY, 4) == 6 && obs::column(1.f, 0.f, NAN, 4) == 6,
          "column rule fixed points");
    const float specials[] = {NAN, INFINITY, -INFINITY, -0.0f, 0.0f, 1e38f, -1e38f, 3.4e38f};
    for (int it = 0; it < iters; ++it) {
        const int32_t C = (int32_t)rint_(1, 70), N = (int32_t)(1 << rint_(0, 12)), nbins = (int32_t)(rint_(0, 3) ? rint_(1, 40) : rint_(1, obs::kMaxBins));
        const int32_t n_seconds = (int32_t)rint_(1, 6);
        const int64_t n = rint_(0, 300), j0 = rint_(0, 3) ? rint_(0, 5000) : rint_(0, (int64_t)1 << 40);
        const int64_t fs = (int64_t)N * rint_(1, 4000);   // 1 .. 4000 rows per second
        const int64_t j_defer = j0 + rint_(-10, 3000), cap_def = rint_(0, 40);
        const bool defer = rint_(0, 2) != 0;
        std::vector<uint64_t> ev((size_t)n);
        std::vector<float> h((size_t)n), lo((size_t)C), inv((size_t)C);
        for (auto& x : lo) x = (float)rint_(-300, 300) / 100.f;
        for (auto& x : inv) x = rint_(0, 20) ? (float)rint_(1, 4000) / 100.f : specials[rint_(0, 7)];
        for (int64_t p = 0; p < n; ++p) {
            const uint64_t ch = rint_(0, 5) ? (uint64_t)rint_(0, C - 1) : (uint64_t)rint_(0, 4095);
            const int64_t jg = j0 + rint_(j0 > 0 ? -1 : 0, 6000);
            ev[(size_t)p] = (ch << MKID_PKT_CH_SHIFT) | ((uint64_t)rint_(0, (1 << 24) - 1) << MKID_PKT_BASE_SHIFT) |
                            ((uint64_t)jg & MKID_PKT_TS_MASK);
            const int64_t k = rint_(0, 9);
            h[(size_t)p] = k == 0 ? specials[rint_(0, 7)]
                           : k == 1 ? lo[(size_t)std::min<uint64_t>(ch, C - 1)] + (float)rint_(0, nbins) / inv[(size_t)std::min<uint64_t>(ch, C - 1)]
                                    : (float)rint_(-2000, 2000) / 100.f;
        }
        std::vector<int32_t> image((size_t)n_seconds * C, 0), ref_image(image);
        int64_t outside[2] = {0, 0}, ref_outside[2] = {0, 0};
        CHECK(obs::count_args_ok(ev.data(), n, j0, N, (double)fs, C, n_seconds, image.data(), outside), "count args");
        // two calls over the halves: the results continue
        obs::count_host(ev.data(), n / 2, j0, N, (double)fs, C, n_seconds, image.data(), outside);
        obs::count_host(ev.data() + n / 2, n - n / 2, j0, N, (double)fs, C, n_seconds, image.data(), outside);
        const int64_t base = j0 > ((int64_t)1 << 27) ? j0 - ((int64_t)1 << 27) : 0;
        const int32_t cols = nbins + obs::kExtraCols;
        std::vector<int32_t> spectra((size_t)C * cols, 0), ref_spectra(spectra);
        std::vector<uint64_t> deferred((size_t)cap_def + 1), ref_deferred;   // + 1: never a null data()
        int64_t ndef[2] = {0, 0}, qualified = 0;
        obs::spectra_host(ev.data(), h.data(), n, j0, j_defer, C, lo.data(), inv.data(), nbins, spectra.data(),
                          defer ? deferred.data() : nullptr, cap_def, defer ? ndef : nullptr);
        for (int64_t p = 0; p < n; ++p) {
            const uint64_t w = ev[(size_t)p];
            const int64_t ch = (int64_t)(w >> 52), ts = (int64_t)(w & 0xFFFFFFF);
            const int64_t jg = base + (((ts - base) % (1 << 28)) + (1 << 28)) % (1 << 28);
            const mkid::pkt::Stamp st = mkid::pkt::decode(w, j0);
            CHECK(st.ch == ch && st.jg == jg, "decode");
            if (ch >= C) {
                ++ref_outside[0];
                continue;
            }
            const int64_t sec = (jg * N) / fs;
            CHECK(sec == obs::second(jg, N, fs), "second");
            if (sec >= n_seconds)
                ++ref_outside[1];
            else
                ++ref_image[(size_t)(sec * C + ch)];
            const float x = h[(size_t)p];
            if (defer && !std::isfinite(x) && jg >= j_defer) {
                ++qualified;
                if ((int64_t)ref_deferred.size() < cap_def) ref_deferred.push_back(w);
                continue;
            }
            int32_t col;
            const float u = (x - lo[(size_t)ch]) * inv[(size_t)ch];
            if (!std::isfinite(x) || std::isnan(u)) col = nbins + 2;
            else if (u < 0.f) col = 0;
            else if (u >= (float)nbins) col = nbins + 1;
            else col = 1 + (int32_t)u;
            CHECK(col == obs::column(x, lo[(size_t)ch], inv[(size_t)ch], nbins) && col >= 0 && col < cols, "column %d", col);
            ++ref_spectra[(size_t)ch * cols + col];
        }
        CHECK(image == ref_image && outside[0] == ref_outside[0] && outside[1] == ref_outside[1], "count image");
        CHECK(spectra == ref_spectra, "spectra");
        CHECK(ndef[1] <= cap_def, "deferred list past cap_def");
        deferred.resize((size_t)ndef[1]);
        CHECK(ndef[0] == qualified && ndef[1] == (int64_t)ref_deferred.size() && deferred == ref_deferred, "deferred list");
    }
    int32_t i4 = 0;
    int64_t o2[2] = {0, 0};
    uint64_t w1 = 0;
    float f1 = 0.f;
    CHECK(!obs::count_args_ok(&w1, 1, 0, 128, 1e6, 64, 0, &i4, o2) && !obs::count_args_ok(&w1, 1, 0, 128, 1e6, 64, (1 << 20) + 1, &i4, o2) &&
              !obs::count_args_ok(nullptr, 1, 0, 128, 1e6, 64, 1, &i4, o2) && !obs::count_args_ok(&w1, -1, 0, 128, 1e6, 64, 1, &i4, o2) &&
              !obs::count_args_ok(&w1, 1, -1, 128, 1e6, 64, 1, &i4, o2) && !obs::count_args_ok(&w1, 1, INT64_MAX / 128, 128, 1e6, 64, 1, &i4, o2) &&
              obs::count_args_ok(nullptr, 0, 0, 128, 1e6, 64, 1, &i4, o2),
          "count argument checks");
    CHECK(!obs::spectra_args_ok(&w1, &f1, 1, 0, 64, &f1, &f1, 0, &i4, nullptr, 0, nullptr) &&
              !obs::spectra_args_ok(&w1, &f1, 1, 0, 64, &f1, &f1, 16385, &i4, nullptr, 0, nullptr) &&
              !obs::spectra_args_ok(&w1, &f1, 1, 0, 64, &f1, &f1, 4, &i4, &w1, 0, nullptr) &&
              !obs::spectra_args_ok(&w1, &f1, 1, 0, 64, &f1, &f1, 4, &i4, &w1, -1, o2) &&
              obs::spectra_args_ok(&w1, &f1, 1, 0, 64, &f1, &f1, 4, &i4, &w1, 0, o2),
          "spectra argument checks");
}

// The photon rows (obs_common.h list_host, fill_host) on random words, stamps near the 28-bit wrap,
// K = 1, overflowing rows and fs edge values, against a per-packet dictionary; the tables are
// buffers of exactly the documented sizes, so a slot or cell outside them is an ASan report.
static void fuzz_photons(int iters) {
    namespace obs = mkid::obs;
    CHECK(obs::fs_us_ok(8796093022208.0) && !obs::fs_us_ok(8796093022209.0) && !obs::fs_us_ok(1e6 + 0.5) && obs::fs_us_ok(1.0),
          "fs_us_ok");
    CHECK(obs::microsecond(0, 1, 8796093022208) == 0 && obs::microsecond(8796093022207, 1, 8796093022208) == 999999 &&
              obs::microsecond(3, 128, 1000000) == 384 && obs::microsecond(7813, 128, 1000000) == 64,
          "microsecond fixed points");
    CHECK(obs::row_word(((uint64_t)3 << 52) | ((uint64_t)1500 << 40) | ((uint64_t)1900 << 28) | 77, 123456, MKID_ROW_WIDE) ==
                  (((uint64_t)3 << 52) | ((uint64_t)1500 << 40) | ((uint64_t)1900 << 28) | 123456) &&
              obs::row_word(((uint64_t)3 << 52) | ((uint64_t)1500 << 40) | ((uint64_t)1900 << 28) | 77, 123456, MKID_ROW_REFERENCE) ==
                  (((uint64_t)3 << 56) | ((uint64_t)1500 << 44) | ((uint64_t)1648 << 32) | ((uint64_t)1900 << 20) | 123456),
          "row word fixed points");
    for (int it = 0; it < iters; ++it) {
        const int32_t C = (int32_t)rint_(1, 40), N = (int32_t)(1 << rint_(0, 12));
        const int32_t n_seconds = (int32_t)rint_(1, 4), K = (int32_t)(rint_(0, 2) ? rint_(1, 6) : 1);
        const int32_t layout = (int32_t)rint_(0, 1);
        const int64_t edge = rint_(0, 5);
        // 1 .. 300 rows per second, or the clock's edges: fs = 1, fs = 2^43 (there a second is 2^43 / N rows)
        const int64_t fs = edge == 0 ? 1 : edge == 1 ? (int64_t)1 << 43 : (int64_t)N * rint_(1, 300);
        const int64_t wrap = (int64_t)1 << 28;
        const int64_t j0 = rint_(0, 2) ? rint_(0, 3) * wrap + rint_(-40, 40) + (rint_(0, 1) ? wrap / 2 : 0) : rint_(0, 2000);
        const int64_t j0c = j0 < 0 ? 0 : j0, n = rint_(0, 400);
        const int64_t base = j0c > wrap / 2 ? j0c - wrap / 2 : 0;
        std::vector<uint64_t> ev((size_t)n);
        std::vector<int64_t> jgs((size_t)n);
        for (int64_t p = 0; p < n; ++p) {
            const uint64_t ch = rint_(0, 7) ? (uint64_t)rint_(0, C - 1) : (uint64_t)rint_(0, 4095);
            int64_t jg = j0c + rint_(-30, 900);
            if (jg < base) jg = base;
            jgs[(size_t)p] = jg;
            ev[(size_t)p] = (ch << MKID_PKT_CH_SHIFT) | ((uint64_t)rint_(0, (1 << 24) - 1) << MKID_PKT_BASE_SHIFT) |
                            ((uint64_t)jg & MKID_PKT_TS_MASK);
        }
        const size_t cells = (size_t)n_seconds * C, slots = cells * K;
        std::vector<int32_t> image(cells, 0), ref_image(cells, 0);
        std::vector<uint64_t> words(slots, 0x5A5A), ref_words(slots, 0x5A5A);
        std::vector<int64_t> stamps(slots, -7), ref_stamps(slots, -7);
        int64_t outside[2] = {0, 0}, ref_outside[2] = {0, 0}, dropped = 0, ref_dropped = 0;
        CHECK(obs::list_args_ok(ev.data(), n, j0c, N, (double)fs, C, n_seconds, K, layout, image.data(), outside, words.data(),
                                stamps.data(), &dropped),
              "list args");
        // three calls over the thirds: the tables continue
        const int64_t cut[4] = {0, n / 3, 2 * n / 3, n};
        for (int k = 0; k < 3; ++k)
            obs::list_host(ev.data() + cut[k], cut[k + 1] - cut[k], j0c, N, (double)fs, C, n_seconds, K, layout, image.data(),
                           outside, words.data(), stamps.data(), &dropped);
        std::vector<std::vector<std::pair<uint64_t, int64_t>>> dict(cells);
        for (int64_t p = 0; p < n; ++p) {
            const uint64_t w = ev[(size_t)p];
            const int64_t ch = (int64_t)(w >> 52), jg = jgs[(size_t)p];
            CHECK(mkid::pkt::decode(w, j0c).jg == jg, "decode near the wrap");
            if (ch >= C) {
                ++ref_outside[0];
                continue;
            }
            const __int128 sample = (__int128)jg * N;
            const int64_t sec = (int64_t)(sample / fs), us = (int64_t)((sample % fs) * 1000000 / fs);
            CHECK(us == obs::microsecond(jg, N, fs) && us >= 0 && us < 1000000, "microsecond %lld", (long long)us);
            if (sec >= n_seconds) {
                ++ref_outside[1];
                continue;
            }
            const uint64_t peak = (w >> 40) & 0xFFF, bs = (w >> 28) & 0xFFF;
            const int64_t d = (int64_t)peak - (int64_t)bs + 2048;
            const uint64_t p1 = (uint64_t)std::min<int64_t>(std::max<int64_t>(d, 0), 4095);
            const uint64_t word = layout == MKID_ROW_WIDE
                                      ? ((uint64_t)ch << 52 | peak << 40 | bs << 28 | (uint64_t)us)
                                      : ((uint64_t)ch << 56 | peak << 44 | p1 << 32 | bs << 20 | ((uint64_t)us & 0xFFFFF));
            dict[(size_t)(sec * C + ch)].push_back({word, jg});
        }
        for (size_t k = 0; k < cells; ++k) {
            ref_image[k] = (int32_t)dict[k].size();
            for (size_t s = 0; s < dict[k].size(); ++s) {
                if (s < (size_t)K)
                    ref_words[k * K + s] = dict[k][s].first, ref_stamps[k * K + s] = dict[k][s].second;
                else
                    ++ref_dropped;
            }
        }
        CHECK(image == ref_image && outside[0] == ref_outside[0] && outside[1] == ref_outside[1], "rows: image");
        CHECK(words == ref_words && stamps == ref_stamps && dropped == ref_dropped, "rows: words, stamps, dropped");
        // fill: rows made stamp-ascending with distinct stamps first, as the device's order gives them
        for (size_t k = 0; k < cells; ++k) {
            const int64_t m = obs::row_fill(image[k], K);
            CHECK(m == std::min<int64_t>((int64_t)dict[k].size(), K), "row_fill");
            std::sort(stamps.begin() + (int64_t)(k * K), stamps.begin() + (int64_t)(k * K) + m);
            for (int64_t s = 1; s < m; ++s)
                if (stamps[k * K + s] <= stamps[k * K + s - 1]) stamps[k * K + s] = stamps[k * K + s - 1] + 1;
        }
        const bool with_dt = rint_(0, 1) != 0;
        const int64_t j_defer = j0c + rint_(-10, 900);
        std::vector<float> h((size_t)n), dt((size_t)n), row_h(slots, NAN), row_dt(slots, NAN), ref_h(slots, NAN), ref_dt(slots, NAN);
        const float specials[] = {NAN, INFINITY, -INFINITY, -0.0f, 0.0f};
        for (int64_t p = 0; p < n; ++p) {
            h[(size_t)p] = rint_(0, 3) ? (float)rint_(-2000, 2000) / 100.f : specials[rint_(0, 4)];
            dt[(size_t)p] = (float)rint_(-300, 300) / 100.f;
        }
        int64_t fill[2] = {0, 0}, ref_fill[2] = {0, 0};
        CHECK(obs::fill_args_ok(ev.data(), h.data(), n, j0c, N, (double)fs, C, n_seconds, K, image.data(), stamps.data(),
                                row_h.data(), fill),
              "fill args");
        obs::fill_host(ev.data(), h.data(), with_dt ? dt.data() : nullptr, n, j0c, j_defer, N, (double)fs, C, n_seconds, K,
                       image.data(), stamps.data(), row_h.data(), row_dt.data(), fill);
        for (int64_t p = 0; p < n; ++p) {
            const int64_t ch = (int64_t)(ev[(size_t)p] >> 52), jg = jgs[(size_t)p];
            if (ch >= C || (!std::isfinite(h[(size_t)p]) && jg >= j_defer)) continue;
            const int64_t sec = (int64_t)((__int128)jg * N / fs);
            int64_t at = -1;
            if (sec < n_seconds) {
                const size_t k = (size_t)(sec * C + ch);
                for (int64_t s = 0; s < obs::row_fill(image[k], K); ++s)
                    if (stamps[k * K + s] == jg) at = (int64_t)(k * K) + s;
            }
            if (at < 0) {
                ++ref_fill[1];
                continue;
            }
            ++ref_fill[0];
            ref_h[(size_t)at] = h[(size_t)p];
            if (with_dt) ref_dt[(size_t)at] = dt[(size_t)p];
        }
        CHECK(fill[0] == ref_fill[0] && fill[1] == ref_fill[1], "fill counters");
        CHECK(memcmp(row_h.data(), ref_h.data(), slots * 4) == 0 && memcmp(row_dt.data(), ref_dt.data(), slots * 4) == 0,
              "filled heights");
    }
    int32_t i4 = 0;
    int64_t o2[2] = {0, 0}, s1 = 0;
    uint64_t w1 = 0;
    float f1 = 0.f;
    CHECK(!obs::list_args_ok(&w1, 1, 0, 128, 1e6, 64, 1, 0, 0, &i4, o2, &w1, &s1, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 1e6, 64, 1, 65537, 0, &i4, o2, &w1, &s1, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 1e6, 64, 1, 1, 2, &i4, o2, &w1, &s1, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 1e6, 255, 1, 1, MKID_ROW_REFERENCE, &i4, o2, &w1, &s1, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 8796093022209.0, 64, 1, 1, 0, &i4, o2, &w1, &s1, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 1e6, 64, 1, 1, 0, &i4, o2, nullptr, &s1, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 1e6, 64, 1, 1, 0, &i4, o2, &w1, nullptr, o2) &&
              !obs::list_args_ok(&w1, 1, 0, 128, 1e6, 64, 1, 1, 0, &i4, o2, &w1, &s1, nullptr) &&
              obs::list_args_ok(nullptr, 0, 0, 128, 1e6, 254, 1, 65536, MKID_ROW_REFERENCE, &i4, o2, &w1, &s1, o2),
          "list argument checks");
    CHECK(!obs::fill_args_ok(&w1, nullptr, 1, 0, 128, 1e6, 64, 1, 1, &i4, &s1, &f1, o2) &&
              !obs::fill_args_ok(&w1, &f1, 1, 0, 128, 1e6, 64, 1, 1, nullptr, &s1, &f1, o2) &&
              !obs::fill_args_ok(&w1, &f1, 1, 0, 128, 1e6, 64, 1, 1, &i4, nullptr, &f1, o2) &&
              !obs::fill_args_ok(&w1, &f1, 1, 0, 128, 1e6, 64, 1, 1, &i4, &s1, nullptr, o2) &&
              !obs::fill_args_ok(&w1, &f1, 1, 0, 128, 1e6, 64, 1, 1, &i4, &s1, &f1, nullptr) &&
              !obs::fill_args_ok(&w1, &f1, 1, 0, 128, 1e6, 64, 1, 0, &i4, &s1, &f1, o2) &&
              obs::fill_args_ok(nullptr, nullptr, 0, 0, 128, 1e6, 64, 1, 1, &i4, &s1, &f1, o2),
          "fill argument checks");
}

// The ring forms and the packed second (obs_common.h list_ring_host, fill_ring_host, pack_host,
// clear_host) on random lists: windows with sec0 at and around the edges of the seconds the list
// holds, K = 1, overflowing rows, cap_out below, at and above the total; every table and every
// output is a buffer of exactly the documented size, so an access outside one is an ASan report.
static void fuzz_pack(int iters) {
    namespace obs = mkid::obs;
    CHECK(obs::window_ok(obs::Window{0, 0, 1}, 1.0) && obs::window_ok(obs::Window{5, 5, 1 << 20}, 1e6) &&
              !obs::window_ok(obs::Window{0, 1, 0}, 1e6) && !obs::window_ok(obs::Window{0, 1, (1 << 20) + 1}, 1e6) &&
              !obs::window_ok(obs::Window{-1, 1, 1}, 1e6) && !obs::window_ok(obs::Window{2, 1, 1}, 1e6) &&
              obs::window_ok(obs::Window{0, INT64_MAX / 1000000 - 1, 1}, 1e6) &&
              !obs::window_ok(obs::Window{0, INT64_MAX / 1000000, 1}, 1e6) && !obs::window_ok(obs::Window{0, 1, 1}, 0.5),
          "window_ok");
    for (int it = 0; it < iters; ++it) {
        const int32_t C = (int32_t)rint_(1, 24), N = (int32_t)(1 << rint_(0, 8));
        const int32_t R = (int32_t)rint_(1, 4), K = (int32_t)(rint_(0, 2) ? rint_(1, 5) : 1);
        const int32_t layout = (int32_t)rint_(0, 1);
        const int64_t per = rint_(1, 60), fs = (int64_t)N * per;   // rows per second
        const int64_t j0 = rint_(0, 3000), first = j0 * N / fs;    // the list spans seconds first .. first + 6
        const int64_t sec0 = std::max<int64_t>(0, first + rint_(-2, 6)), sec_end = sec0 + rint_(0, 6);
        const obs::Window w{sec0, sec_end, R};
        const int64_t n = rint_(0, 300);
        std::vector<uint64_t> ev((size_t)n);
        std::vector<int64_t> jgs((size_t)n);
        for (int64_t p = 0; p < n; ++p) {
            const uint64_t ch = rint_(0, 7) ? (uint64_t)rint_(0, C - 1) : (uint64_t)rint_(0, 4095);
            jgs[(size_t)p] = j0 + rint_(0, 6 * per);
            ev[(size_t)p] = (ch << MKID_PKT_CH_SHIFT) | ((uint64_t)rint_(0, (1 << 24) - 1) << MKID_PKT_BASE_SHIFT) |
                            ((uint64_t)jgs[(size_t)p] & MKID_PKT_TS_MASK);
        }
        const size_t cells = (size_t)R * C, slots = cells * K;
        std::vector<int32_t> image(cells, 0);
        std::vector<uint64_t> words(slots, 0x5A5A);
        std::vector<int64_t> stamps(slots, -7);
        int64_t outside[4] = {0, 0, 0, 0}, ref_outside[4] = {0, 0, 0, 0}, dropped = 0, ref_dropped = 0;
        CHECK(obs::list_ring_args_ok(ev.data(), n, j0, N, (double)fs, C, w, K, layout, image.data(), outside, words.data(),
                                     stamps.data(), &dropped),
              "ring list args");
        obs::list_ring_host(ev.data(), n, j0, N, (double)fs, C, w, K, layout, image.data(), outside, words.data(),
                            stamps.data(), &dropped);
        std::vector<std::vector<std::pair<uint64_t, int64_t>>> dict(cells);
        for (int64_t p = 0; p < n; ++p) {
            const int64_t ch = (int64_t)(ev[(size_t)p] >> 52), jg = jgs[(size_t)p], sec = jg * N / fs;
            if (ch >= C)
                ++ref_outside[0];
            else if (sec >= sec_end)
                ++ref_outside[1];
            else if (sec < sec0)
                ++ref_outside[2];
            else if (sec >= sec0 + R)
                ++ref_outside[3];
            else
                dict[(size_t)(sec % R * C + ch)].push_back({obs::row_word(ev[(size_t)p], obs::microsecond(jg, N, fs), layout), jg});
        }
        CHECK(memcmp(outside, ref_outside, sizeof outside) == 0, "ring: outside");
        bool same = true;
        for (size_t k = 0; k < cells; ++k) {
            same = same && image[k] == (int32_t)dict[k].size();
            for (size_t s = 0; s < dict[k].size(); ++s) {
                if (s < (size_t)K)
                    same = same && words[k * K + s] == dict[k][s].first && stamps[k * K + s] == dict[k][s].second;
                else
                    ++ref_dropped;
            }
            for (size_t s = dict[k].size(); s < (size_t)K; ++s) same = same && words[k * K + s] == 0x5A5A && stamps[k * K + s] == -7;
        }
        CHECK(same && dropped == ref_dropped, "ring: rows");
        // fill: rows made stamp-ascending with distinct stamps, as the device's order gives them
        for (size_t k = 0; k < cells; ++k) {
            const int64_t m = obs::row_fill(image[k], K);
            std::sort(stamps.begin() + (int64_t)(k * K), stamps.begin() + (int64_t)(k * K) + m);
            for (int64_t s = 1; s < m; ++s)
                if (stamps[k * K + s] <= stamps[k * K + s - 1]) stamps[k * K + s] = stamps[k * K + s - 1] + 1;
        }
        const bool with_dt = rint_(0, 1) != 0;
        const int64_t j_defer = j0 + rint_(-5, 6 * per);
        std::vector<float> h((size_t)n), dt((size_t)n), row_h(slots, NAN), row_dt(slots, NAN), ref_h(slots, NAN), ref_dt(slots, NAN);
        for (int64_t p = 0; p < n; ++p) {
            h[(size_t)p] = rint_(0, 3) ? (float)rint_(-2000, 2000) / 100.f : NAN;
            dt[(size_t)p] = (float)rint_(-300, 300) / 100.f;
        }
        int64_t fill[2] = {0, 0}, ref_fill[2] = {0, 0};
        CHECK(obs::fill_ring_args_ok(ev.data(), h.data(), n, j0, N, (double)fs, C, w, K, image.data(), stamps.data(),
                                     row_h.data(), fill),
              "ring fill args");
        obs::fill_ring_host(ev.data(), h.data(), with_dt ? dt.data() : nullptr, n, j0, j_defer, N, (double)fs, C, w, K,
                            image.data(), stamps.data(), row_h.data(), with_dt ? row_dt.data() : nullptr, fill);
        for (int64_t p = 0; p < n; ++p) {
            const int64_t ch = (int64_t)(ev[(size_t)p] >> 52), jg = jgs[(size_t)p], sec = jg * N / fs;
            if (ch >= C || (!std::isfinite(h[(size_t)p]) && jg >= j_defer)) continue;
            int64_t at = -1;
            if (sec >= sec0 && sec < sec_end && sec < sec0 + R) {
                const size_t k = (size_t)(sec % R * C + ch);
                for (int64_t s = 0; s < obs::row_fill(image[k], K); ++s)
                    if (stamps[k * K + s] == jg) at = (int64_t)(k * K) + s;
            }
            ++ref_fill[at < 0 ? 1 : 0];
            if (at < 0) continue;
            ref_h[(size_t)at] = h[(size_t)p];
            if (with_dt) ref_dt[(size_t)at] = dt[(size_t)p];
        }
        CHECK(fill[0] == ref_fill[0] && fill[1] == ref_fill[1], "ring: fill counters");
        CHECK(memcmp(row_h.data(), ref_h.data(), slots * 4) == 0 && memcmp(row_dt.data(), ref_dt.data(), slots * 4) == 0,
              "ring: filled heights");
        // pack every slot at a cap_out below, at and above its total, then clear it
        if (rint_(0, 3) == 0) image[(size_t)rint_(0, (int64_t)cells - 1)] = (int32_t)rint_(INT32_MIN, -1);   // a wrapped count
        for (int32_t slot = 0; slot < R; ++slot) {
            const int64_t sec = slot + (int64_t)R * rint_(0, 1000);
            int64_t total = 0;
            for (int32_t c = 0; c < C; ++c) total += obs::row_fill(image[(size_t)slot * C + c], K);
            const int64_t caps[5] = {0, std::max<int64_t>(total - 1, 0), total, total + 1, rint_(0, total + 3)};
            for (const int64_t cap : caps) {
                std::vector<int32_t> counts((size_t)C, -1);
                std::vector<int64_t> offsets((size_t)C + 1, -1), ostamps((size_t)cap, -9);
                std::vector<uint64_t> owords((size_t)cap, 0xA5A5);
                std::vector<float> oh((size_t)cap, -1.f), odt((size_t)cap, -1.f);
                int64_t tot[2] = {-1, -1};
                const bool st = rint_(0, 1) != 0;
                CHECK(obs::pack_args_ok(sec, R, K, C, image.data(), words.data(), stamps.data(), row_h.data(),
                                        with_dt ? row_dt.data() : nullptr, cap, counts.data(), offsets.data(),
                                        cap ? owords.data() : nullptr, st ? ostamps.data() : nullptr,
                                        cap ? oh.data() : nullptr, with_dt ? odt.data() : nullptr, tot),
                      "pack args");
                obs::pack_host(sec, R, K, C, image.data(), words.data(), stamps.data(), row_h.data(),
                               with_dt ? row_dt.data() : nullptr, cap, counts.data(), offsets.data(), owords.data(),
                               st ? ostamps.data() : nullptr, oh.data(), with_dt ? odt.data() : nullptr, tot);
                CHECK(tot[0] == total && tot[1] == std::min(total, cap) && offsets[(size_t)C] == total, "pack: total");
                int64_t at = 0;
                bool ok = true;
                for (int32_t c = 0; c < C; ++c) {
                    const size_t k = (size_t)slot * C + c;
                    ok = ok && counts[(size_t)c] == image[k] && offsets[(size_t)c] == at;
                    for (int64_t i = 0; i < obs::row_fill(image[k], K); ++i, ++at) {
                        if (at >= cap) continue;
                        ok = ok && owords[(size_t)at] == words[k * K + i] && (!st || ostamps[(size_t)at] == stamps[k * K + i]) &&
                             memcmp(&oh[(size_t)at], &row_h[k * K + i], 4) == 0 &&
                             (!with_dt || memcmp(&odt[(size_t)at], &row_dt[k * K + i], 4) == 0);
                    }
                }
                for (int64_t i = tot[1]; i < cap; ++i) ok = ok && owords[(size_t)i] == 0xA5A5 && oh[(size_t)i] == -1.f;
                CHECK(ok, "pack: entries");
            }
            std::vector<int32_t> image0 = image;
            std::vector<float> h0 = row_h, dt0 = row_dt;
            CHECK(obs::clear_args_ok(sec, R, K, C, image.data(), row_h.data()), "clear args");
            obs::clear_host(sec, R, K, C, image.data(), row_h.data(), with_dt ? row_dt.data() : nullptr);
            bool ok = true;
            for (size_t k = 0; k < cells; ++k) {
                const bool mine = k / C == (size_t)slot;
                ok = ok && image[k] == (mine ? 0 : image0[k]);
                for (int64_t i = 0; i < K; ++i) {
                    const bool hit = mine && i < obs::row_fill(image0[k], K);
                    uint32_t a, b;
                    memcpy(&a, &row_h[k * K + i], 4), memcpy(&b, &row_dt[k * K + i], 4);
                    ok = ok && (hit ? a == obs::kNanBits : memcmp(&a, &h0[k * K + i], 4) == 0);
                    ok = ok && (hit && with_dt ? b == obs::kNanBits : memcmp(&b, &dt0[k * K + i], 4) == 0);
                }
            }
            CHECK(ok, "clear");
        }
    }
    int32_t i4 = 0;
    int64_t o2[2] = {0, 0}, s1 = 0;
    uint64_t w1 = 0;
    float f1 = 0.f;
    CHECK(!obs::pack_args_ok(-1, 1, 1, 1, &i4, &w1, &s1, &f1, &f1, 1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 0, 1, 1, &i4, &w1, &s1, &f1, &f1, 1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 1, 0, 1, &i4, &w1, &s1, &f1, &f1, 1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 1, 1, 4097, &i4, &w1, &s1, &f1, &f1, 1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 1, 1, 1, &i4, &w1, &s1, &f1, &f1, -1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 1, 1, 1, &i4, &w1, &s1, &f1, &f1, 1, &i4, o2, nullptr, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 1, 1, 1, &i4, &w1, nullptr, &f1, &f1, 1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              !obs::pack_args_ok(0, 1, 1, 1, &i4, &w1, &s1, &f1, nullptr, 1, &i4, o2, &w1, &s1, &f1, &f1, o2) &&
              obs::pack_args_ok(0, 1, 1, 1, &i4, &w1, nullptr, &f1, nullptr, 0, &i4, o2, nullptr, nullptr, nullptr, nullptr, o2),
          "pack argument checks");
}

// The laser lines, the calibration and the energy cube (wavecal_common.h lines_host, cube_host) on
// random rows (empty, single bins, plateaus, Gaussian lines, counts past 2^31), every parameter range's
// ends, and random packets, heights and calibration tables (NaN, +-inf, not usable); the rows, the
// result tables and the cube are buffers of exactly the documented sizes, so a bin, line or column
// outside them is an ASan report. Checked besides: the chosen bins ascend, keep min_sep, are local
// maxima of the smoothed row at or above min_peak, windows stay inside the row and apart, a status of
// 0 goes with finite coefficients and resolving powers and the usable flag, any other with NaN, the
// spectrum is not written, and a row's cube total is its packets that are neither deferred nor of a
// channel >= C.
static void fuzz_wavecal(int iters) {
    namespace obs = mkid::obs;
    namespace wcal = mkid::wcal;
    const double E3[3] = {1.26, 1.88, 3.06};
    const double bad1[2] = {1.0, 1.0}, bad2[1] = {-1.0}, bad3[1] = {NAN}, bad4[1] = {INFINITY}, bad5[1] = {0.0};
    CHECK(wcal::energies_ok(E3, 3) && wcal::energies_ok(E3, 1) && !wcal::energies_ok(E3, 0) && !wcal::energies_ok(E3, 4) &&
              !wcal::energies_ok(nullptr, 1) && !wcal::energies_ok(bad1, 2) && !wcal::energies_ok(bad2, 1) &&
              !wcal::energies_ok(bad3, 1) && !wcal::energies_ok(bad4, 1) && !wcal::energies_ok(bad5, 1),
          "energies_ok");
    for (int it = 0; it < iters; ++it) {
        const int32_t nbins = (int32_t)(rint_(0, 5) == 0 ? (rint_(0, 1) ? obs::kMaxBins : rint_(1, 3)) : rint_(1, 700));
        const int32_t nch = (int32_t)rint_(1, 4), P = (int32_t)rint_(1, 3);
        const int32_t w = (int32_t)(rint_(0, 3) == 0 ? (rint_(0, 1) ? 0 : wcal::kMaxSmooth) : rint_(0, 6));
        const int32_t g = (int32_t)(rint_(0, 3) == 0 ? (rint_(0, 1) ? 1 : wcal::kMaxFitHalf) : rint_(1, 20));
        const int32_t min_sep = (int32_t)(rint_(0, 4) == 0 ? rint_(1, 2 * (int64_t)nbins) : rint_(1, 40));
        const int64_t min_peak = rint_(0, 5) == 0 ? rint_(-5, 5) : rint_(1, 200);
        const int32_t cols = nbins + obs::kExtraCols;
        std::vector<int32_t> sp((size_t)nch * cols, -7);
        for (int32_t c = 0; c < nch; ++c) {
            int32_t* n = sp.data() + (size_t)c * cols + 1;
            const int kind = (int)rint_(0, 5);
            for (int32_t b = 0; b < nbins; ++b) n[b] = kind == 0 ? 0 : (kind == 1 ? (int32_t)rint_(0, 6) : 0);
            if (kind == 2) n[rint_(0, nbins - 1)] = (int32_t)rint_(1, 100000);
            if (kind == 3)
                for (int k = 0; k < 3; ++k) {
                    const int64_t b0 = rint_(0, nbins - 1), len = rint_(1, 9);
                    for (int64_t b = b0; b < std::min<int64_t>(b0 + len, nbins); ++b) n[b] = 50;
                }
            if (kind == 4)
                for (int k = 0; k < 3; ++k) {
                    const double mu = (double)rint_(0, nbins - 1), sg = (double)rint_(1, 12), amp = (double)rint_(5, 5000);
                    for (int32_t b = 0; b < nbins; ++b)
                        n[b] += (int32_t)(amp * std::exp(-0.5 * (b + 0.5 - mu) * (b + 0.5 - mu) / (sg * sg)) + (double)rint_(0, 3));
                }
            if (kind == 5)
                for (int32_t b = 0; b < nbins; ++b) n[b] = (int32_t)(uint32_t)rint_(0xFFFFF000ll, 0xFFFFFFFFll);
        }
        const std::vector<int32_t> sp0 = sp;
        std::vector<float> lo((size_t)nch), step((size_t)nch);
        for (auto& x : lo) x = (float)rint_(-300, 300) / 100.f;
        for (auto& x : step) x = rint_(0, 9) ? (float)rint_(-400, 400) / 1000.f : 0.f;
        std::vector<mkid_line_fit> lines((size_t)nch * P);
        std::vector<mkid_energy_cal> cal((size_t)nch);
        std::vector<float> cal_f((size_t)nch * 4);
        CHECK(wcal::lines_args_ok(sp.data(), lo.data(), step.data(), nch, nbins, P, E3, w, min_sep, g, lines.data(), cal.data(),
                                  cal_f.data()),
              "lines args");
        wcal::lines_host(sp.data(), lo.data(), step.data(), nch, wcal::make_params(nbins, P, E3, w, min_sep, min_peak, g),
                         lines.data(), cal.data(), cal_f.data());
        CHECK(sp == sp0, "the spectrum was written");
        for (int32_t c = 0; c < nch; ++c) {
            const int32_t* n = sp.data() + (size_t)c * cols + 1;
            const mkid_energy_cal& k = cal[(size_t)c];
            const mkid_line_fit* f = lines.data() + (size_t)c * P;
            CHECK(k.n_found >= 0 && k.n_found <= P && ((k.status & MKID_CAL_FEW_LINES) != 0) == (k.n_found < P), "n_found %d status %d",
                  k.n_found, k.status);
            int32_t bins[3] = {0, 0, 0};
            for (int32_t p = 0; p < P; ++p) {
                if (p >= k.n_found) {
                    CHECK(f[p].bin == -1 && f[p].nfit == 0 && std::isnan(f[p].mu), "a line that was not found");
                    continue;
                }
                bins[p] = f[p].bin;
                const int64_t s = wcal::smooth_at(n, nbins, w, f[p].bin);
                CHECK(f[p].bin >= 0 && f[p].bin < nbins && f[p].peak_s == s && s >= min_peak && s > wcal::smooth_at(n, nbins, w, f[p].bin - 1) &&
                          s >= wcal::smooth_at(n, nbins, w, f[p].bin + 1),
                      "line %d at bin %d is no candidate", p, f[p].bin);
                CHECK(p == 0 || f[p].bin - f[p - 1].bin >= min_sep, "lines %d and %d closer than min_sep", p - 1, p);
                CHECK(std::isnan(f[p].mu) == ((k.status & (MKID_CAL_FIT_FAILED << p)) != 0), "fit bit of line %d", p);
                CHECK(std::isnan(f[p].mu) == std::isnan(f[p].sigma) && std::isnan(f[p].mu) == std::isnan(f[p].amp), "a fit's NaNs");
                CHECK(f[p].nfit >= 0 && f[p].nfit <= 2 * g + 1 && f[p].counts >= 0, "nfit %d", f[p].nfit);
            }
            for (int32_t p = 0; p < k.n_found; ++p) {
                const wcal::Window win = wcal::window(bins, k.n_found, p, g, nbins);
                CHECK(win.b0 >= 0 && win.b1 < nbins && win.b0 <= bins[p] && bins[p] <= win.b1, "window of line %d", p);
                if (p + 1 < k.n_found) CHECK(win.b1 < wcal::window(bins, k.n_found, p + 1, g, nbins).b0, "windows overlap");
            }
            const float* cf = cal_f.data() + (size_t)c * 4;
            if (k.status == 0) {
                CHECK(std::isfinite(k.c[0]) && std::isfinite(k.c[1]) && std::isfinite(k.c[2]) && cf[3] == 1.0f, "status 0 without coefficients");
                for (int32_t p = 0; p < 3; ++p) CHECK(p < P ? k.r[p] >= 0.0 : std::isnan(k.r[p]), "resolving power %d", p);
            } else {
                CHECK(std::isnan(k.c[0]) && std::isnan(k.c[1]) && std::isnan(k.c[2]) && std::isnan(k.r[0]) && cf[3] == 0.0f &&
                          std::isnan(cf[0]),
                      "a status with coefficients");
            }
        }
        // the cube over random packets with this table (the first C of its rows) and odd ones
        const int32_t C = nch, nb = (int32_t)(rint_(0, 3) ? rint_(1, 40) : rint_(1, obs::kMaxBins));
        const int32_t mode = (int32_t)rint_(0, 1);
        const int64_t n = rint_(0, 200), j0 = rint_(0, 5000), j_defer = rint_(0, 2) ? j0 + rint_(0, 3000) : INT64_MAX;
        const float specials[] = {NAN, INFINITY, -INFINITY, -0.0f, 0.0f, 1e38f, -1e38f, 3.4e38f};
        if (rint_(0, 2) == 0)
            for (auto& x : cal_f) x = rint_(0, 3) ? (float)rint_(-300, 300) / 100.f : specials[rint_(0, 7)];
        std::vector<uint64_t> ev((size_t)n);
        std::vector<float> h((size_t)n), energy((size_t)n, -5.f);
        int64_t want = 0;
        for (int64_t p = 0; p < n; ++p) {
            const uint64_t ch = rint_(0, 5) ? (uint64_t)rint_(0, C - 1) : (uint64_t)rint_(0, 4095);
            const int64_t jg = j0 + rint_(j0 > 0 ? -1 : 0, 6000);
            ev[(size_t)p] = (ch << MKID_PKT_CH_SHIFT) | ((uint64_t)jg & MKID_PKT_TS_MASK);
            h[(size_t)p] = rint_(0, 6) ? (float)rint_(-3000, 3000) / 1000.f : specials[rint_(0, 7)];
            want += (int64_t)ch < C && !obs::deferred(h[(size_t)p], jg, j_defer);
        }
        const float hc = 1240.7f, vlo = (float)rint_(-100, 500), vinv = rint_(0, 9) ? (float)rint_(1, 400) / 100.f : specials[rint_(0, 7)];
        std::vector<int32_t> cube((size_t)C * (nb + obs::kExtraCols), 0);
        CHECK(wcal::cube_args_ok(ev.data(), h.data(), n, j0, C, cal_f.data(), mode, nb, cube.data()), "cube args");
        const wcal::CubeRule rule{j0, j_defer, C, nb, mode, hc, vlo, vinv};
        wcal::cube_host(ev.data(), h.data(), n / 2, cal_f.data(), rule, cube.data(), energy.data());
        wcal::cube_host(ev.data() + n / 2, h.data() + n / 2, n - n / 2, cal_f.data(), rule, cube.data(), energy.data() + n / 2);
        int64_t got = 0;
        for (int32_t v : cube) got += v;
        CHECK(got == want, "cube total %lld of %lld packets", (long long)got, (long long)want);
        for (int64_t p = 0; p < n; ++p) {
            const bool pixel = (int64_t)(ev[(size_t)p] >> MKID_PKT_CH_SHIFT) < C;
            uint32_t bits;
            memcpy(&bits, &energy[(size_t)p], 4);
            CHECK(pixel ? (!std::isnan(energy[(size_t)p]) || bits == obs::kNanBits) : energy[(size_t)p] == -5.f, "energy of packet %lld",
                  (long long)p);
        }
    }
    int32_t i4 = 0;
    float f1 = 0.f;
    uint64_t w1 = 0;
    mkid_line_fit l1{};
    mkid_energy_cal c1{};
    CHECK(!wcal::lines_args_ok(&i4, &f1, &f1, 0, 4, 1, E3, 0, 1, 1, &l1, &c1, &f1) && !wcal::lines_args_ok(&i4, &f1, &f1, 1, 0, 1, E3, 0, 1, 1, &l1, &c1, &f1) &&
              !wcal::lines_args_ok(&i4, &f1, &f1, 1, 16385, 1, E3, 0, 1, 1, &l1, &c1, &f1) && !wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 1, E3, 65, 1, 1, &l1, &c1, &f1) &&
              !wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 1, E3, -1, 1, 1, &l1, &c1, &f1) && !wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 1, E3, 0, 0, 1, &l1, &c1, &f1) &&
              !wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 1, E3, 0, 1, 0, &l1, &c1, &f1) && !wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 1, E3, 0, 1, 65, &l1, &c1, &f1) &&
              !wcal::lines_args_ok(nullptr, &f1, &f1, 1, 4, 1, E3, 0, 1, 1, &l1, &c1, &f1) && !wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 1, E3, 0, 1, 1, &l1, &c1, nullptr) &&
              wcal::lines_args_ok(&i4, &f1, &f1, 1, 4, 3, E3, 64, 1, 64, &l1, &c1, &f1),
          "lines argument checks");
    CHECK(!wcal::cube_args_ok(&w1, &f1, 1, 0, 64, &f1, 2, 4, &i4) && !wcal::cube_args_ok(&w1, &f1, 1, 0, 64, &f1, 0, 0, &i4) &&
              !wcal::cube_args_ok(&w1, &f1, 1, 0, 64, &f1, 0, 16385, &i4) && !wcal::cube_args_ok(&w1, &f1, -1, 0, 64, &f1, 0, 4, &i4) &&
              !wcal::cube_args_ok(&w1, &f1, 1, -1, 64, &f1, 0, 4, &i4) && !wcal::cube_args_ok(nullptr, &f1, 1, 0, 64, &f1, 0, 4, &i4) &&
              !wcal::cube_args_ok(&w1, &f1, 1, 0, 64, nullptr, 0, 4, &i4) && !wcal::cube_args_ok(&w1, &f1, 1, 0, 4097, &f1, 0, 4, &i4) &&
              wcal::cube_args_ok(nullptr, nullptr, 0, 0, 64, &f1, 1, 4, &i4),
          "cube argument checks");
}

// The resonator loop fits (loopfit_common.h fit_host) over random and degenerate sweeps: resonator
// loops with noise, constant sweeps, straight lines, zero frequencies, NaN, +-inf and huge samples,
// zero, negative and non-finite standard deviations, draws far outside their ranges, every shape's
// ends (fsteps 12 and 1024, S 1 and 16, max_iter 1). All arrays are buffers of exactly the documented
// sizes, so a point, start or channel outside them is an ASan report. Checked besides: the window
// lies inside the sweep around cidx with at most 2 (fsteps / 4) points, a failure status goes with
// NaN floats, best_start -1 and evals 0, any other with finite parameters inside their bounds, a
// finite chi^2 that is the lowest of chisq_all with ties to the lower start, and 1 <= evals <=
// max_iter with the max_iter bit only when evals == max_iter; the inputs are not written.
static void fuzz_loopfit(int iters) {
    namespace lfit = mkid::lfit;
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const double odd[] = {NAN, INFINITY, -INFINITY, 0.0, -0.0, 1e300, -1e300, 1e-300};
    for (int it = 0; it < iters; ++it) {
        const int32_t nch = (int32_t)rint_(1, 3);
        const int32_t fsteps = (int32_t)(rint_(0, 7) == 0 ? (rint_(0, 1) ? lfit::kMinSteps : lfit::kMaxSteps) : rint_(12, 140));
        const int32_t S = (int32_t)(rint_(0, 5) == 0 ? (rint_(0, 1) ? 1 : lfit::kMaxStarts) : rint_(1, 6));
        const int32_t max_iter = (int32_t)(rint_(0, 5) == 0 ? 1 : rint_(2, 25));
        const bool sd = rint_(0, 1) != 0, qg = rint_(0, 2) == 0;
        const size_t np = (size_t)nch * fsteps;
        std::vector<double> x(np), I(np), Q(np), isd(sd ? np : 0), qsd(sd ? np : 0), draws((size_t)nch * S * 5), qguess(qg ? nch : 0);
        for (int32_t c = 0; c < nch; ++c) {
            const int kind = (int)rint_(0, 6);
            const double Qr = 15e3 + 65e3 * U(rng), f0 = 4e9 + 2e9 * U(rng), R = 2e3 + 2e4 * U(rng);
            const double span = (4.0 + 4.0 * U(rng)) * f0 / Qr, off = (U(rng) - 0.5) * span;
            const double ci = (2.0 + 3.0 * U(rng)) * R * (rint_(0, 1) ? 1.0 : -1.0), cq = (2.0 + 3.0 * U(rng)) * R * (rint_(0, 1) ? 1.0 : -1.0);
            const double ang = 6.0 * U(rng) - 3.0;
            for (int32_t i = 0; i < fsteps; ++i) {
                const size_t k = (size_t)c * fsteps + i;
                x[k] = kind == 3 ? 0.0 : f0 + off + span * ((double)i / (fsteps - 1) - 0.5);
                const double t = 2.0 * Qr * (x[k] - f0) / f0, den = 1.0 + t * t;
                const double re = (t * t / den - 0.5) * 2.0 * R, im = t / den * 2.0 * R;
                I[k] = re * std::cos(ang) + im * std::sin(ang) + ci + 0.01 * R * N(rng);
                Q[k] = -re * std::sin(ang) + im * std::cos(ang) + cq + 0.01 * R * N(rng);
                if (kind == 1) I[k] = 12.0, Q[k] = -3.0;                     // a constant sweep
                if (kind == 2) I[k] = (double)i, Q[k] = 5.0;                 // a straight line, flat in Q
                if (kind == 4 && rint_(0, 9) == 0) (rint_(0, 1) ? I[k] : Q[k]) = odd[rint_(0, 7)];
                if (kind == 5 && rint_(0, 9) == 0) x[k] = odd[rint_(0, 7)];
                if (kind == 6) I[k] = std::rint(I[k]) - std::rint(ci), Q[k] = std::rint(Q[k]);   // centres near an axis
                if (sd) {
                    isd[k] = rint_(0, 30) ? 0.01 * R * (0.5 + U(rng)) : odd[rint_(0, 7)];
                    qsd[k] = rint_(0, 30) ? 0.01 * R * (0.5 + U(rng)) : -1.0;
                }
            }
            if (qg) qguess[(size_t)c] = rint_(0, 5) ? Qr * (0.5 + U(rng)) : odd[rint_(0, 7)];
        }
        for (auto& d : draws) d = rint_(0, 40) ? 2.0 * U(rng) - 1.0 : (rint_(0, 1) ? odd[rint_(0, 7)] : 50.0 * N(rng));
        const std::vector<double> x0 = x, I0 = I, Q0 = Q;
        std::vector<mkid_loop_fit> fits((size_t)nch);
        std::vector<double> call((size_t)nch * S, -7.0);
        const double ftol = rint_(0, 3) ? 1e-8 : 1e-2;
        const bool want_all = rint_(0, 3) != 0;
        CHECK(lfit::args_ok(x.data(), I.data(), Q.data(), sd ? isd.data() : nullptr, sd ? qsd.data() : nullptr, draws.data(), nch,
                            fsteps, S, max_iter, ftol, fits.data()),
              "loop fit args");
        lfit::fit_host(x.data(), I.data(), Q.data(), sd ? isd.data() : nullptr, sd ? qsd.data() : nullptr, draws.data(),
                       qg ? qguess.data() : nullptr, nch, fsteps, S, max_iter, ftol, fits.data(), want_all ? call.data() : nullptr);
        CHECK(memcmp(x.data(), x0.data(), np * 8) == 0 && memcmp(I.data(), I0.data(), np * 8) == 0 &&
                  memcmp(Q.data(), Q0.data(), np * 8) == 0,
              "the sweep was written");
        for (int32_t c = 0; c < nch; ++c) {
            const mkid_loop_fit& f = fits[(size_t)c];
            const int32_t q = fsteps / 4;
            CHECK(f.cidx >= 0 && f.cidx <= fsteps - 3 && f.low == std::max(f.cidx - q, 0) && f.high == std::min(f.cidx + q, fsteps) &&
                      f.n == f.high - f.low && f.n >= 3 && f.n <= 2 * q && f.n <= lfit::kMaxWindow && f.pad == 0,
                  "window %d %d %d %d of %d", f.cidx, f.low, f.high, f.n, fsteps);
            const int32_t fail = MKID_LOOP_NONFINITE | MKID_LOOP_FLAT | MKID_LOOP_NO_FIT;
            CHECK((f.status & ~(fail | MKID_LOOP_MAX_ITER)) == 0, "status %d", f.status);
            if (f.status & fail) {
                bool nan = std::isnan(f.chisq) && std::isnan(f.qc) && std::isnan(f.qi) && std::isnan(f.dipdb);
                for (int i = 0; i < lfit::kNP; ++i) nan = nan && std::isnan(f.p[i]);
                CHECK(nan && f.best_start == -1 && f.evals == 0 && (f.status & MKID_LOOP_MAX_ITER) == 0, "a failed fit with results");
                if (want_all)
                    for (int32_t s = 0; s < S; ++s) CHECK(!std::isfinite(call[(size_t)c * S + s]), "a failed fit with a finite start");
                continue;
            }
            CHECK(f.best_start >= 0 && f.best_start < S && f.evals >= 1 && f.evals <= max_iter &&
                      (((f.status & MKID_LOOP_MAX_ITER) != 0) ? f.evals == max_iter : true) && std::isfinite(f.chisq) && f.chisq >= 0.0,
                  "start %d evals %d status %d", f.best_start, f.evals, f.status);
            const double* xw = x.data() + (size_t)c * fsteps;
            const double xlo = *std::min_element(xw + f.low, xw + f.high), xhi = *std::max_element(xw + f.low, xw + f.high);
            CHECK(f.p[0] >= 5e3 && f.p[0] <= 1e6 && f.p[1] >= xlo && f.p[1] <= xhi && f.p[2] >= 1e-4 &&
                      f.p[2] <= 1e2 && f.p[3] >= 1.0 && f.p[3] <= 4e4 && std::fabs(f.p[4]) <= 5e3 && std::fabs(f.p[5]) <= 1.1 * lfit::kPi + 1e-12 &&
                      f.p[6] > 0.0 && f.p[7] > 0.0 && std::isfinite(f.p[8]) && std::isfinite(f.p[9]),
                  "parameters outside their bounds");
            if (want_all)
                for (int32_t s = 0; s < S; ++s) {
                    const double v = call[(size_t)c * S + s];
                    CHECK(!std::isfinite(v) || v > f.chisq || (v == f.chisq && s >= f.best_start), "start %d beats the best", s);
                    if (s == f.best_start) CHECK(v == f.chisq, "chisq_all of the best start");
                }
        }
    }
    double d1 = 1.0, w[lfit::kWin], sum = 0.0;
    mkid_loop_fit f1{};
    lfit::window_weights(w);
    for (double v : w) sum += v;
    CHECK(w[0] == w[9] && std::fabs(w[0]) < 1e-16 && std::fabs(sum - 1.0) < 1e-15, "window weights");
    CHECK(!lfit::args_ok(nullptr, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, &d1, nullptr, &d1, 1, 12, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, &d1, &d1, 1, 12, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, nullptr, 1, 12, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 1, 1, 1e-6, nullptr) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 0, 12, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 11, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 1025, 1, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 0, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 17, 1, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 1, 0, 1e-6, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 1, 1, 0.0, &f1) &&
              !lfit::args_ok(&d1, &d1, &d1, nullptr, nullptr, &d1, 1, 12, 1, 1, NAN, &f1) &&
              lfit::args_ok(&d1, &d1, &d1, &d1, &d1, &d1, 1, 1024, 16, 1, 1e-6, &f1),
          "loop fit argument checks");
}

// The resonator magnitude fits (magfit_common.h fit_host) over random and degenerate sweeps: dips with
// noise, all-zero and constant sweeps, zero and equal frequencies, NaN, +-inf and huge samples, draws
// far outside a normal's range, every shape's ends. All arrays are buffers of exactly the documented
// sizes, so a point, start or channel outside them is an ASan report. Checked besides: cidx lies
// inside the velocities, norm is the largest magnitude, a failure status goes with NaN parameters,
// best_start -1, evals 0 and a d_qout of 50000, any other with finite parameters inside their bounds,
// a d_qout of p[0], a finite chi^2 that is the lowest of chisq_all with ties to the lower start, and
// 1 <= evals <= max_iter with the max_iter bit only when evals == max_iter; the inputs are not written.
static void fuzz_magfit(int iters) {
    namespace mfit = mkid::mfit;
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const double odd[] = {NAN, INFINITY, -INFINITY, 0.0, -0.0, 1e300, -1e300, 1e-300};
    for (int it = 0; it < iters; ++it) {
        const int32_t nch = (int32_t)rint_(1, 3);
        const int32_t fsteps = (int32_t)(rint_(0, 7) == 0 ? (rint_(0, 1) ? mfit::kMinSteps : mfit::kMaxSteps) : rint_(12, 140));
        const int32_t S = (int32_t)(rint_(0, 5) == 0 ? (rint_(0, 1) ? 1 : mfit::kMaxStarts) : rint_(1, 6));
        const int32_t max_iter = (int32_t)(rint_(0, 5) == 0 ? 1 : rint_(2, 25));
        const size_t np = (size_t)nch * fsteps;
        std::vector<double> x(np), I(np), Q(np), draws((size_t)nch * S);
        for (int32_t c = 0; c < nch; ++c) {
            const int kind = (int)rint_(0, 6);
            const double Qr = 15e3 + 65e3 * U(rng), f0 = 4e9 + 2e9 * U(rng), R = 2e3 + 2e4 * U(rng);
            const double span = (4.0 + 4.0 * U(rng)) * f0 / Qr, off = (U(rng) - 0.5) * span, ang = 6.0 * U(rng);
            for (int32_t i = 0; i < fsteps; ++i) {
                const size_t k = (size_t)c * fsteps + i;
                x[k] = kind == 3 ? 0.0 : (kind == 6 ? f0 : f0 + off + span * ((double)i / (fsteps - 1) - 0.5));
                const double t = 2.0 * Qr * (f0 + off + span * ((double)i / (fsteps - 1) - 0.5) - f0) / f0;
                const double m = R * (1.0 - 0.7 * (1.0 - std::fabs(t) / std::sqrt(1.0 + t * t))) * (1.0 + 1e-3 * N(rng));
                I[k] = m * std::cos(ang), Q[k] = m * std::sin(ang);
                if (kind == 1) I[k] = 0.0, Q[k] = 0.0;                       // an all-zero sweep
                if (kind == 2) I[k] = 12.0, Q[k] = -3.0;                     // a constant sweep
                if (kind == 4 && rint_(0, 9) == 0) (rint_(0, 1) ? I[k] : Q[k]) = odd[rint_(0, 7)];
                if (kind == 5 && rint_(0, 9) == 0) x[k] = odd[rint_(0, 7)];
            }
        }
        for (auto& d : draws) d = rint_(0, 40) ? N(rng) : (rint_(0, 1) ? odd[rint_(0, 7)] : 50.0 * N(rng));
        const std::vector<double> x0 = x, I0 = I, Q0 = Q;
        std::vector<mkid_mag_fit> fits((size_t)nch);
        std::vector<double> call((size_t)nch * S, -7.0), qout((size_t)nch, -7.0);
        const double ftol = rint_(0, 3) ? 1e-8 : 1e-2;
        const bool want_all = rint_(0, 3) != 0, want_q = rint_(0, 3) != 0;
        CHECK(mfit::args_ok(x.data(), I.data(), Q.data(), draws.data(), nch, fsteps, S, max_iter, ftol, fits.data()), "mag fit args");
        mfit::fit_host(x.data(), I.data(), Q.data(), draws.data(), nch, fsteps, S, max_iter, ftol, fits.data(),
                       want_q ? qout.data() : nullptr, want_all ? call.data() : nullptr);
        CHECK(memcmp(x.data(), x0.data(), np * 8) == 0 && memcmp(I.data(), I0.data(), np * 8) == 0 &&
                  memcmp(Q.data(), Q0.data(), np * 8) == 0,
              "the sweep was written");
        for (int32_t c = 0; c < nch; ++c) {
            const mkid_mag_fit& f = fits[(size_t)c];
            const double *xw = x.data() + (size_t)c * fsteps, *Iw = I.data() + (size_t)c * fsteps, *Qw = Q.data() + (size_t)c * fsteps;
            CHECK(f.cidx >= 0 && f.cidx <= fsteps - 3, "cidx %d of %d", f.cidx, fsteps);
            bool finite = true, top = true;
            for (int32_t i = 0; i < fsteps; ++i) {
                finite = finite && std::isfinite(xw[i]) && std::isfinite(Iw[i]) && std::isfinite(Qw[i]);
                top = top && !(std::sqrt(Iw[i] * Iw[i] + Qw[i] * Qw[i]) > f.norm);
            }
            const int32_t fail = MKID_LOOP_NONFINITE | MKID_LOOP_FLAT | MKID_LOOP_NO_FIT;
            CHECK((f.status & ~(fail | MKID_LOOP_MAX_ITER)) == 0 && finite == ((f.status & MKID_LOOP_NONFINITE) == 0), "status %d", f.status);
            if (finite) CHECK(top && f.norm >= 0.0 && ((f.status & MKID_LOOP_FLAT) != 0) == (f.norm == 0.0), "norm %g status %d", f.norm, f.status);
            if (f.status & fail) {
                bool nan = std::isnan(f.chisq);
                for (int i = 0; i < mfit::kNP; ++i) nan = nan && std::isnan(f.p[i]);
                CHECK(nan && f.best_start == -1 && f.evals == 0 && (f.status & MKID_LOOP_MAX_ITER) == 0, "a failed fit with results");
                if (want_q) CHECK(qout[(size_t)c] == 50000.0, "qout of a failed fit %g", qout[(size_t)c]);
                if (want_all)
                    for (int32_t s = 0; s < S; ++s) CHECK(!std::isfinite(call[(size_t)c * S + s]), "a failed fit with a finite start");
                continue;
            }
            CHECK(f.best_start >= 0 && f.best_start < S && f.evals >= 1 && f.evals <= max_iter &&
                      (((f.status & MKID_LOOP_MAX_ITER) != 0) ? f.evals == max_iter : true) && std::isfinite(f.chisq) && f.chisq >= 0.0,
                  "start %d evals %d status %d", f.best_start, f.evals, f.status);
            const double xlo = *std::min_element(xw, xw + fsteps), xhi = *std::max_element(xw, xw + fsteps);
            CHECK(f.p[0] >= 5e3 && f.p[0] <= 1e6 && f.p[1] >= xlo && f.p[1] <= xhi && f.p[2] >= 1e-4 && f.p[2] <= 1e2 &&
                      f.p[3] >= 0.01 && f.p[3] <= 10.0 && std::fabs(f.p[4]) <= 5e3 && std::fabs(f.p[5]) <= 1e8,
                  "parameters outside their bounds");
            if (want_q) CHECK(qout[(size_t)c] == f.p[0], "qout %g of Q %g", qout[(size_t)c], f.p[0]);
            if (want_all)
                for (int32_t s = 0; s < S; ++s) {
                    const double v = call[(size_t)c * S + s];
                    CHECK(!std::isfinite(v) || v > f.chisq || (v == f.chisq && s >= f.best_start), "start %d beats the best", s);
                    if (s == f.best_start) CHECK(v == f.chisq, "chisq_all of the best start");
                }
        }
    }
    double d1 = 1.0;
    mkid_mag_fit f1{};
    CHECK(!mfit::args_ok(nullptr, &d1, &d1, &d1, 1, 12, 1, 1, 1e-6, &f1) && !mfit::args_ok(&d1, nullptr, &d1, &d1, 1, 12, 1, 1, 1e-6, &f1) &&
              !mfit::args_ok(&d1, &d1, nullptr, &d1, 1, 12, 1, 1, 1e-6, &f1) && !mfit::args_ok(&d1, &d1, &d1, nullptr, 1, 12, 1, 1, 1e-6, &f1) &&
              !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 12, 1, 1, 1e-6, nullptr) && !mfit::args_ok(&d1, &d1, &d1, &d1, 0, 12, 1, 1, 1e-6, &f1) &&
              !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 11, 1, 1, 1e-6, &f1) && !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 1025, 1, 1, 1e-6, &f1) &&
              !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 12, 0, 1, 1e-6, &f1) && !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 12, 17, 1, 1e-6, &f1) &&
              !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 12, 1, 0, 1e-6, &f1) && !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 12, 1, 1, 0.0, &f1) &&
              !mfit::args_ok(&d1, &d1, &d1, &d1, 1, 12, 1, 1, NAN, &f1) && mfit::args_ok(&d1, &d1, &d1, &d1, 1, 1024, 16, 1, 1e-6, &f1) &&
              sizeof(mkid_mag_fit) == 80,
          "mag fit argument checks");
}

// Welch spectra and the IQ noise analysis (welch_common.h): pos_of_bin is a permutation for every
// length a pass sequence serves, the four-step split multiplies back to nfft with both factors inside
// the LDS limit, and the host twin's loops (which the kernels' index maps restate) run on buffers of
// exactly the stated sizes: an index outside a segment, a table or a stitched row is an ASan error.
static void fuzz_welch(int iters) {
    namespace wl = mkid::welch;
    for (int32_t n = 2; n <= wl::kLdsMaxN; n *= 2) {
        const wl::Plan p = wl::make_plan(n);
        std::vector<char> seen((size_t)n, 0);
        int32_t prod = 1;
        for (int32_t s = 0; s < p.npass; ++s) prod *= wl::radix(p, s);
        CHECK(prod == n && p.npass >= 1, "welch plan of %d", n);
        for (int32_t k = 0; k < n; ++k) {
            const int32_t pos = wl::pos_of_bin(p, k);
            CHECK(pos >= 0 && pos < n && !seen[(size_t)pos], "welch pos_of_bin(%d) of %d", k, n);
            if (pos >= 0 && pos < n) seen[(size_t)pos] = 1;
        }
    }
    for (int32_t nfft = 2 * wl::kLdsMaxN; nfft <= wl::kMaxN; nfft *= 2) {
        int32_t n1, n2;
        wl::split(nfft, n1, n2);
        CHECK(n1 * n2 == nfft && n1 >= 8 && n1 <= n2 && n2 <= wl::kLdsMaxN && 4096 % n1 == 0 && n2 % (4096 / n1) == 0,
              "welch split of %d: %d x %d", nfft, n1, n2);
    }
    std::normal_distribution<double> nd;
    for (int it = 0; it < iters; ++it) {
        const int m = (int)(rint_(0, 11) == 0 ? rint_(13, 16) : rint_(3, 12));
        const int32_t nfft = 1 << m;
        const int64_t n = nfft + rint_(0, m > 12 ? nfft : 40 * (int64_t)nfft / (m > 8 ? 16 : 1));
        std::vector<double> a((size_t)n), b((size_t)n), pa((size_t)nfft / 2 + 1), pb(pa.size());
        for (auto& x : a) x = nd(rng);
        for (auto& x : b) x = 1.0 + 1e-3 * nd(rng);
        const bool two = rint_(0, 3) != 0;
        CHECK(wl::psd_args_ok(a.data(), n, n, 1, nfft, 1.0, 0, pa.data()) &&
                  !wl::psd_args_ok(a.data(), nfft - 1, n, 1, nfft, 1.0, 0, pa.data()) &&
                  !wl::psd_args_ok(a.data(), n, n - 1, 1, nfft, 1.0, 0, pa.data()) &&
                  !wl::psd_args_ok(a.data(), n, n, 1, nfft + 1, 1.0, 0, pa.data()),
              "welch args at %d", nfft);
        wl::Tables t;
        wl::make_tables(nfft, t);
        wl::channel_host(nfft, t, wl::RowLoader{a.data(), two ? b.data() : nullptr}, n, 2e5,
                         wl::Sink{pa.data(), two ? pb.data() : nullptr, 0, nfft / 2 + 1, 0});
        double sum = 0.0;
        bool ok = true;
        for (double v : pa) ok = ok && std::isfinite(v) && v >= 0.0, sum += v;
        // Parseval: sum of the one-sided density x (fs / nfft) is the windowed mean square (about 1)
        CHECK(ok && sum * (2e5 / nfft) > 0.05 && sum * (2e5 / nfft) < 20.0, "welch density at %d: %g", nfft, sum);
    }
    for (int it = 0; it < iters / 4 + 1; ++it) {
        mkid_iqnoise_cfg c{};
        c.nfft_high = 1 << rint_(3, 8), c.nfft_low = c.nfft_high << rint_(1, 14 - wl::log2i(c.nfft_high));
        c.k_join = (int32_t)rint_(1, c.nfft_high / 2 - 1);
        const int32_t nout = wl::iq_nout(c);
        c.fit_count = (int32_t)rint_(2, std::min(nout, 9)), c.fit_first = (int32_t)rint_(0, nout - c.fit_count);
        c.samprate = 2e5, c.f_eval = 1e3, c.gain = 0.2, c.full_scale = 32767.0;
        CHECK(wl::iq_cfg_ok(&c), "iq cfg %d/%d/%d", c.nfft_low, c.nfft_high, c.k_join);
        mkid_iqnoise_cfg bad = c;
        bad.fit_first = nout - c.fit_count + 1;
        CHECK(!wl::iq_cfg_ok(&bad), "iq cfg fit range");
        const int64_t n = c.nfft_low + rint_(0, c.nfft_low);
        std::vector<int16_t> I((size_t)n), Q((size_t)n);
        const bool centred = rint_(0, 5) == 0;   // a record whose mean is the centre: rad == 0
        for (int64_t j = 0; j < n; ++j) {
            I[(size_t)j] = centred ? (int16_t)((j & 1) ? 7 : -7) : (int16_t)(3000 + 30 * nd(rng));
            Q[(size_t)j] = centred ? (int16_t)((j & 1) ? -3 : 3) : (int16_t)(-2000 + 30 * nd(rng));
        }
        if (centred && (n & 1)) I[(size_t)n - 1] = 0, Q[(size_t)n - 1] = 0;
        int64_t si = 0, sq = 0;
        for (int64_t j = 0; j < n; ++j) si += I[(size_t)j], sq += Q[(size_t)j];
        mkid_iqnoise_result r;
        const double icen = centred ? 0.0 : 6e-3, qcen = centred ? 0.0 : -3e-3;
        wl::iq_means(si, sq, n, c, 0.0, 0.0, icen, qcen, 2e4, &r);
        CHECK(centred == ((r.status & MKID_IQN_BAD_RAD) != 0) && r.sum_i == si && r.pad == 0, "iq status %d", r.status);
        std::vector<double> pn((size_t)nout), an((size_t)nout);
        wl::Tables tl, th;
        wl::make_tables(c.nfft_low, tl), wl::make_tables(c.nfft_high, th);
        const wl::IqLoader ld(I.data(), Q.data(), c, 0.0, 0.0, icen, qcen, r);
        wl::channel_host(c.nfft_low, tl, ld, n, c.samprate, wl::iq_sink_low(c, pn.data(), an.data()));
        wl::channel_host(c.nfft_high, th, ld, n, c.samprate, wl::iq_sink_high(c, pn.data(), an.data()));
        const double fn = wl::iq_fn1k(c, pn.data(), 2e4, r.status);
        CHECK(centred ? std::isnan(fn) : std::isfinite(fn), "iq fn1k %g", fn);
        for (int32_t b2 = 1; b2 < nout; ++b2)
            CHECK(wl::iq_freq(c, b2) > wl::iq_freq(c, b2 - 1), "iq freq axis at %d", b2);
    }
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 300;
    rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
    fuzz_plans(iters);
    fuzz_sizing(iters / 2 + 1);
    fuzz_capacity(iters / 3 + 1);
    fuzz_slot_order(iters / 10 + 2);
    fuzz_quantize(iters / 3 + 1);
    fuzz_merge_pack(iters);
    fuzz_pkt(iters);
    fuzz_carry(iters);
    fuzz_bank(iters);
    fuzz_thresholds(iters / 2 + 1);
    fuzz_noise(iters / 10 + 1);
    fuzz_fit(iters);
    fuzz_observe(iters);
    fuzz_photons(iters);
    fuzz_pack(iters);
    fuzz_wavecal(iters / 3 + 1);
    fuzz_loopfit(iters / 3 + 1);
    fuzz_magfit(iters / 3 + 1);
    fuzz_welch(iters / 10 + 2);
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("plan_fuzz ok: %d iterations\n", iters);
    return 0;
}
