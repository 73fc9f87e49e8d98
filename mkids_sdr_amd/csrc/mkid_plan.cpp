// Host-side planning (mkid_plan.h): plain C++, no HIP, built into libmkidgpu.so and, with
// -fsanitize=address,undefined, into the CPU fuzz driver tools/plan_fuzz.cpp.
#include <array>
#include "mkid_plan.h"
#include "pkt_common.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace mkid {
namespace plan {

int64_t seg_capacity(int64_t L, int dead) { return L / (dead + 3) + 2; }

int64_t seg_length(int64_t J, int C, int64_t wave_slots) {
    const int64_t nt = std::max<int64_t>(1, wave_slots * 64 / C);
    return std::max<int64_t>(kSegL, (J + nt - 1) / nt);
}

const char* size_workspace(const mkid_cfg& cfg, int64_t trig_slots, int64_t svf_lanes, int64_t svf_w,
                           Workspace& ws) {
    const int C = cfg.n_channels, N = cfg.fft_len;
    if (C <= 0 || N != 2 * C || cfg.max_chunk < N || cfg.max_chunk % N != 0 || cfg.dead_time < 0)
        return "unsupported geometry";
    if (trig_slots < 1 || svf_lanes < 1 || svf_w < kFirTaps || svf_w % kFirTaps != 0) return "bad tuning values";
    ws = Workspace{};
    ws.max_chunk = cfg.max_chunk;
    ws.Kmax = cfg.max_chunk / (N / 2);
    ws.Jmax = cfg.max_chunk / N;
    ws.trig_slots = trig_slots;
    ws.svf_lanes = svf_lanes;
    ws.svf_w = svf_w;
    // packet capacities are hard bounds (seg_capacity): no per-channel/segment overflow can occur
    const int64_t cap_bound = seg_capacity(ws.Jmax, cfg.dead_time);   // whole call, one segment
    ws.capc = std::min<int64_t>(cfg.max_events_per_ch > 0 ? cfg.max_events_per_ch : cap_bound, INT_MAX / 2);
    // plan_trigger rounds segment lengths UP to the 26-sample ring: every segment of a call of
    // J <= Jmax rows is at most round26(Jmax) long (EMA: round26(max(kSegL, ceil(J / nt))), and a
    // multi-segment plan needs J > kSegL; SVF: round26(ceil(J / nseg)) or J), and the EMA segments of
    // a full call at most Lmax = round26(seg_length(Jmax)) (found by tools/plan_fuzz.cpp: sizing
    // from the unrounded lengths left some legal calls one packet short of the scratch)
    auto round26 = [](int64_t L) { return (L + kFirTaps - 1) / kFirTaps * kFirTaps; };
    const int64_t Lmax = round26(seg_length(ws.Jmax, C, trig_slots));
    // for J <= Jmax: L(J) <= Lmax and ceil(J / L(J)) <= max(slots * 64 / C, ceil(Jmax / kSegL))
    ws.nseg_max = std::max<int64_t>(std::max<int64_t>(1, trig_slots * 64 / C), (ws.Jmax + kSegL - 1) / kSegL);
    const int64_t capseg = seg_capacity(Lmax, cfg.dead_time);
    const int64_t capseg_any = seg_capacity(round26(ws.Jmax), cfg.dead_time);   // any one segment
    // one [C][nseg][capseg] table per call
    ws.slot_cap = (int64_t)C * std::max<int64_t>(std::max<int64_t>(ws.nseg_max * capseg, ws.capc), capseg_any);
    // the fix-up re-runs one segment per channel into [C][capseg]: any plan's capseg, including an
    // SVF segment as long as the whole call (plan_trigger), whatever max_events_per_ch says
    ws.scratch_cap = std::max<int64_t>(std::max<int64_t>(capseg, ws.capc), capseg_any);
    return nullptr;
}

static TrigPlan plan_trigger(const Workspace& ws, int C, int mode, int dead, int64_t J) {
    TrigPlan p;
    p.J = J;
    if (mode == MKID_BASE_SVF) {
        // svf_lanes segments over all channels (the per-lane walk is latency bound), each
        // >= kSvfLmin rows; short calls run as one exact segment
        const int64_t want = std::max<int64_t>(1, ws.svf_lanes / C);
        const int64_t nseg = std::min<int64_t>(std::min<int64_t>(want, J / kSvfLmin), ws.nseg_max);
        p.W = 0;
        p.L = (int32_t)J;
        p.nseg = 1;
        if (nseg > 1 && J > 2 * kSvfLmin) {
            int64_t L = (J + nseg - 1) / nseg;
            L = (L + kFirTaps - 1) / kFirTaps * kFirTaps;
            p.L = (int32_t)L;
            p.W = (int32_t)ws.svf_w;
            p.nseg = (int32_t)((J + L - 1) / L);
        }
        p.capseg = (int32_t)seg_capacity(p.L, dead);
        return p;
    }
    const bool serial = J <= kSegL;
    // segment starts at multiples of 26 (the trigger's window ring is group-aligned)
    const int64_t Ls = serial ? J : (seg_length(J, C, ws.trig_slots) + kFirTaps - 1) / kFirTaps * kFirTaps;
    p.L = (int32_t)Ls;
    p.W = serial ? 0 : (int32_t)kSegW;
    p.nseg = (int32_t)((J + Ls - 1) / Ls);
    p.capseg = (int32_t)seg_capacity(Ls, dead);
    return p;
}

const char* plan_call(const Workspace& ws, int C, int N, int mode, int dead, int64_t n, TrigPlan& p) {
    // the per-call buffers (raw rows, IQ tap, slot table) hold max_chunk samples
    if (n <= 0 || n % N != 0 || n > ws.max_chunk) return "call size outside the workspace";
    p = plan_trigger(ws, C, mode, dead, n / N);
    if (p.nseg > ws.nseg_max) return "trigger plan exceeds the segment tables";
    if ((int64_t)C * p.nseg * p.capseg > ws.slot_cap) return "trigger plan exceeds the packet slot table";
    if (p.capseg > ws.scratch_cap) return "trigger plan exceeds the fix-up scratch";
    return nullptr;
}

// Select-slot order (mkid_slot_order). A select thread reads, per channel and frame, the Y entry
// `key` of its bin in each region; a ds_read_b64 costs one LDS cycle per distinct address on the
// busiest bank pair of each 32-lane half (MI355X_MICROARCH.md §LDS), and entry e sits on pair
// e mod 32 (regions and frames are 0 mod 32 entries apart). Each select wave's channels are
// spread over its read groups (one per half-wave and read instruction) so that a group's 32
// channels fall on distinct pairs where the bins allow, each wave keeping its own channels (its
// stores and LO loads stay within the same lines). Greedy per wave: channels by pair-class size,
// each into the group whose cost rises least, then whose new cost is lowest, then the emptiest
// (tools/lds_assign.py holds the same algorithm and its model).
//   k_front3, C = 1024 (N = 2048): key yswz(bin & 511); wave w owns channels 128 w .. 128 w + 127,
//     slot st + 512 q (st = 64 w + 32 h + l) is lane 32 h + l of wave w in read instruction q:
//     random bins ~3.4 cycles per group in channel order, ~1.9 ordered (PMC 287 M -> 156 M).
//   k_front5 layout, C = 2048 (N = 4096): key yswz(bin & 511) + 4 REG s (the pre-combined region
//     P^s, s = bit 9 of the bin: same pair, another address); select wave sw < 8 owns channels
//     64 sw + l + 512 q (q < 3, 6 groups), wave 8 + v owns 1536 + 64 v + l + 256 q (q < 2, 4 groups).
//     Computed for the model and tests only: applied in k_front5 (round 6) it cut the PMC LDS
//     conflict cycles 390.5 M -> 152.9 M per launch but took 2.5 % (plain stores) to 6 %
//     (non-temporal) more time, the scattered stores and the channel decoding costing more than
//     the conflicts, which sit off the transform waves' critical chain.
namespace {
void assign_groups(const std::vector<int>& yo, int ng, std::vector<std::vector<int>>& member) {
    constexpr int GS = 32;
    const int B = (int)yo.size();
    int cnt[32] = {0};
    for (int i = 0; i < B; ++i) ++cnt[yo[i] & 31];
    std::vector<int> order(B);
    for (int i = 0; i < B; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        const int ka = yo[a] & 31, kb = yo[b] & 31;
        if (cnt[ka] != cnt[kb]) return cnt[ka] > cnt[kb];
        if (ka != kb) return ka < kb;
        return yo[a] < yo[b];
    });
    std::vector<int> size(ng, 0), gmax(ng, 0);
    std::vector<std::array<int, 32>> mult(ng);
    for (auto& m : mult) m.fill(0);
    std::vector<std::vector<int>> seen(ng);
    member.assign(ng, {});
    for (int i : order) {
        const int k = yo[i] & 31;
        int bg = -1, bk0 = 0, bk1 = 0, bk2 = 0;
        bool bsame = false;
        for (int g = 0; g < ng; ++g) {
            if (size[g] >= GS) continue;
            const bool same = std::find(seen[g].begin(), seen[g].end(), yo[i]) != seen[g].end();
            const int m = mult[g][k] + (same ? 0 : 1);
            const int nm = std::max(gmax[g], m);
            const int k0 = nm - gmax[g], k1 = nm, k2 = size[g];
            if (bg < 0 || k0 < bk0 || (k0 == bk0 && (k1 < bk1 || (k1 == bk1 && k2 < bk2)))) {
                bg = g; bk0 = k0; bk1 = k1; bk2 = k2; bsame = same;
            }
        }
        member[bg].push_back(i);
        ++size[bg];
        if (!bsame) {
            seen[bg].push_back(yo[i]);
            ++mult[bg][k];
        }
        gmax[bg] = std::max(gmax[bg], mult[bg][k]);
    }
}

int yswz_entry(int b) {
    const int k = b & 511;
    return k ^ ((k >> 2) & 14);
}
}  // namespace

void slot_order(const std::vector<int32_t>& bins, int C, std::vector<int16_t>& out) {
    out.resize(C);
    for (int i = 0; i < C; ++i) out[i] = (int16_t)i;
    if ((C != 1024 && C != 2048) || (int)bins.size() < C) return;
    // per wave: the slots of its read groups (group j = read instruction j >> 1, half j & 1)
    struct Wave { int base, stride, nq; };
    std::vector<Wave> waves;
    if (C == 1024) {
        for (int w = 0; w < 8; ++w) waves.push_back({64 * w, 512, 2});
    } else {
        for (int w = 0; w < 8; ++w) waves.push_back({64 * w, 512, 3});
        for (int v = 0; v < 4; ++v) waves.push_back({1536 + 64 * v, 256, 2});
    }
    constexpr int kRegion4 = 4 * 576;   // k_front5: P^1 regions start 4 REG entries after P^0
    for (const Wave& wv : waves) {
        const int ng = 2 * wv.nq;
        // the wave's channels: k_front3 owns 128 consecutive channels (its slot order predates the
        // k_front5 one and is kept bit-identical); k_front5 the natural channels of its slots
        std::vector<int> chans;
        if (C == 1024) {
            const int w = wv.base / 64;
            for (int i = 0; i < 128; ++i) chans.push_back(128 * w + i);
        } else {
            for (int q = 0; q < wv.nq; ++q)
                for (int l = 0; l < 64; ++l) chans.push_back(wv.base + l + wv.stride * q);
        }
        std::vector<int> yo(chans.size());
        for (size_t i = 0; i < chans.size(); ++i) {
            const int b = bins[chans[i]];
            yo[i] = yswz_entry(b) + (C == 2048 ? kRegion4 * ((b >> 9) & 1) : 0);
        }
        std::vector<std::vector<int>> member;
        assign_groups(yo, ng, member);
        for (int g = 0; g < ng; ++g)
            for (int l = 0; l < 32; ++l)
                out[wv.base + 32 * (g & 1) + l + wv.stride * (g >> 1)] = (int16_t)chans[member[g][l]];
    }
}

// mkid_pulse_fit: the LDS region of one wave and how many a workgroup holds (mkid_plan.h)
FitPlan plan_fit(int32_t ncoeff, int32_t L, int ncu) {
    FitPlan p;
    p.nl = 2 * L + 1;
    p.G = 64 / p.nl;
    p.W = ncoeff + 2 * L;
    p.off_w = 0;
    p.off_cf = p.W;
    p.off_part = p.off_cf + ncoeff;
    p.off_h = p.off_part + 64;
    p.wave_floats = p.off_h + 64;
    p.waves = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kFitWaves, kFitLdsBytes / (4ll * p.wave_floats)));
    p.lds_bytes = 4ll * p.wave_floats * p.waves;
    p.grid_cap = std::max<int64_t>(1, (int64_t)std::max(ncu, 1) * 32 / p.waves);
    return p;
}

// K1 taps as the device applies them (include/mkidgpu.h, mkid_set_pfb): h_q = rint(h 2^S) int16
// with the largest S such that every point's four |h_q| sum to <= 65535 and every |h_q| <= 32767
// (so the fused kernels' int16 dot products never overflow int32 on int16 samples).
int quantize_pfb(const float* h, int T, int N, std::vector<int16_t>& hq) {
    double ms = 0.0, ma = 0.0;
    for (int p = 0; p < N; ++p) {
        double sp = 0.0;
        for (int t = 0; t < T; ++t) {
            const double a = std::fabs((double)h[t * N + p]);
            sp += a;
            ma = std::max(ma, a);
        }
        ms = std::max(ms, sp);
    }
    int S = 0;
    if (ms > 0.0) {
        S = -64;
        while (S < 64 && std::ldexp(ms, S + 1) <= 65535.0 && std::ldexp(ma, S + 1) <= 32767.0) ++S;
    }
    hq.resize((size_t)T * N);
    // rounding can push a point's sum of |h_q| past 65535 (and a dot product of full-scale
    // samples past INT32_MAX): step S down until the ROUNDED taps obey both bounds
    for (;; --S) {
        bool ok = true;
        for (size_t i = 0; i < hq.size(); ++i) {
            const double r = std::rint(std::ldexp((double)h[i], S));
            if (std::fabs(r) > 32767.0) ok = false;
            hq[i] = ok ? (int16_t)r : 0;
        }
        for (int p = 0; p < N && ok; ++p) {
            int64_t sp = 0;
            for (int t = 0; t < T; ++t) sp += std::abs((int64_t)hq[(size_t)t * N + p]);
            if (sp > 65535) ok = false;
        }
        if (ok || S <= -64) break;
    }
    return S;
}

void merge_channel_major(uint64_t* ev, int64_t n) {
    if (n > 1)
        std::stable_sort(ev, ev + n, [](uint64_t a, uint64_t b) {
            return (a >> MKID_PKT_CH_SHIFT) < (b >> MKID_PKT_CH_SHIFT);
        });
}

int pack_reference(const uint64_t* wide, int64_t n, uint64_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t w = wide[i];
        const int32_t ch = pkt::channel(w);
        if (ch >= 255) return -1;  // 8-bit channel field, 255 = end-of-second marker
        out[i] = pkt::reference_word((uint64_t)ch, pkt::peak(w), pkt::base(w), w);   // the stamp's low 20 bits
    }
    return 0;
}

int32_t rearm_level(int32_t thr, int32_t q8) {
    const int64_t p = (int64_t)thr * q8;
    const int64_t fl = p >= 0 ? p / 256 : -((-p + 255) / 256);   // floor(p / 256), no shift of a negative
    return (int32_t)((int64_t)thr - fl);
}

BankWs plan_bank(int64_t Cb, int64_t R, int64_t budget, int64_t want) {
    // bytes per channel of each table, in the order of BankWs's offsets
    const int64_t per[15] = {R * 2000 * 8, R * 800 * 8, R * 8,  (2 * R + 8) * 8, 2000 * 8, 2000 * 8, 800 * 8, 8 * 8,
                             3 * 800 * 8,  800 * 8,     2 * 4,  R * 4,           R * 4,    4,        4};
    BankWs w;
    for (int64_t p : per) w.channel_bytes += p;
    const int64_t slack = 15 * (kBankAlign - 1);   // at most this much padding, whatever the group
    int64_t g = budget > slack ? (budget - slack) / w.channel_bytes : 0;
    g = std::min(g, std::min(Cb, kBankMaxGroup));
    if (want > 0) g = std::min(g, want);
    w.group = std::max<int64_t>(g, 1);
    int64_t* off[15] = {&w.rows, &w.nrows, &w.peaks, &w.scratch, &w.tP,       &w.tPf,    &w.noise, &w.stats,
                        &w.work, &w.coeff, &w.refmed, &w.accept, &w.appended, &w.status, &w.nready};
    for (int i = 0; i < 15; ++i) {
        *off[i] = w.bytes;
        w.bytes += (w.group * per[i] + kBankAlign - 1) / kBankAlign * kBankAlign;
    }
    return w;
}

ThrPlan plan_thresholds(int64_t rows, int64_t ld, int32_t nch, bool aligned16, int ncu) {
    ThrPlan p;
    p.vec = (aligned16 && ld % 8 == 0) ? 8 : 1;
    p.nch_vec = p.vec == 8 ? (nch / 8) * 8 : 0;
    p.strips_vec = (p.nch_vec + kThrStrip - 1) / kThrStrip;
    p.strips_tail = ((int64_t)nch - p.nch_vec + kThrStrip - 1) / kThrStrip;
    const int64_t strips = p.strips_vec + p.strips_tail;
    const int64_t target = 2 * (int64_t)std::max(ncu, 1);
    // rows per block so that strips x row blocks is about the target: rows strips / target, rounded up
    // (rows < 2^31 and strips < 2^26: the product fits)
    int64_t B = (rows * strips + target - 1) / target;
    B = (B + kThrRowStep - 1) / kThrRowStep * kThrRowStep;
    p.B = std::min(std::max(B, kThrMinB), kThrMaxB);
    p.row_blocks = (rows + p.B - 1) / p.B;
    p.grid_vec = std::min(p.strips_vec * p.row_blocks, kThrMaxGrid);
    p.grid_tail = std::min(p.strips_tail * p.row_blocks, kThrMaxGrid);
    p.grid_init = std::min(((int64_t)nch * 100 + kThrThreads - 1) / kThrThreads, kThrMaxInitGrid);
    p.grid_finish = ((int64_t)nch + kThrFinishCh - 1) / kThrFinishCh;
    p.off_lo = 0;
    p.off_hi = (int64_t)nch * 4;
    p.off_counts = (int64_t)nch * 8;
    p.bytes = p.off_counts + (int64_t)nch * 400;
    return p;
}

// exp(-2 pi i k / m), exact at the quarter turns: radix-2 and radix-4 butterflies then add and
// subtract only, and the bins of an integer piece that are sums and differences stay exact
static noise::Cx<double> unit_root(int64_t k, int64_t m) {
    if (4 * k % m == 0) {
        const noise::Cx<double> q[4] = {{1.0, 0.0}, {0.0, -1.0}, {-1.0, 0.0}, {0.0, 1.0}};
        return q[4 * k / m];
    }
    const double a = -6.283185307179586476925286766559 * (double)k / (double)m;
    return {std::cos(a), std::sin(a)};
}

bool plan_noise(int32_t n, NoisePlan& p) {
    p = NoisePlan{};
    if (n < 1 || n > MKID_NOISE_MAX_N) return false;
    static_assert(MKID_NOISE_MAX_N <= 65536 && MKID_NOISE_MAX_N <= kNoiseThreadsLarge * kNoisePerLarge, "uint16 index tables");
    p.n = n;
    std::vector<int32_t> radix;
    int32_t m = n, twos = 0;
    while (m % 2 == 0) m /= 2, ++twos;
    for (int i = 0; i < twos / 2; ++i) radix.push_back(4);
    if (twos % 2) radix.push_back(2);
    for (int32_t f = 3; m > 1; f += 2) {
        if ((int64_t)f * f > m) f = m;
        while (m % f == 0) m /= f, radix.push_back(f);
    }
    std::sort(radix.begin(), radix.end(), [](int32_t a, int32_t b) { return a > b; });
    int32_t L = n, tw = 0;
    for (int32_t r : radix) {
        p.passes.push_back(noise::Pass{r, L, L / r, n / L, tw});
        for (int32_t i = 0; i < r; ++i) p.wr.push_back(unit_root(i, r));
        L /= r, tw += r;
    }
    p.wn.resize((size_t)n);
    for (int32_t i = 0; i < n; ++i) p.wn[(size_t)i] = unit_root(i, n);
    // position p = t_0 M_0 + t_1 M_1 + ... holds bin t_0 + r_0 (t_1 + r_1 (t_2 + ...))
    p.bin_of_pos.resize((size_t)n);
    std::vector<uint16_t> pos_of_bin((size_t)n);
    for (int32_t pos = 0; pos < n; ++pos) {
        int32_t rem = pos, k = 0, w = 1;
        for (const noise::Pass& ps : p.passes) k += (rem / ps.M) * w, rem %= ps.M, w *= ps.r;
        p.bin_of_pos[(size_t)pos] = (uint16_t)k;
        pos_of_bin[(size_t)k] = (uint16_t)pos;
    }
    p.partner.resize((size_t)n);
    for (int32_t pos = 0; pos < n; ++pos)
        p.partner[(size_t)pos] = pos_of_bin[(size_t)((n - p.bin_of_pos[(size_t)pos]) % n)];
    const bool large = n > kNoiseThreadsSmall * kNoisePerSmall;
    p.threads = large ? kNoiseThreadsLarge : kNoiseThreadsSmall;
    p.per_thread = large ? kNoisePerLarge : kNoisePerSmall;
    p.lds_bytes = 8ll * n + 8ll * kNoiseStageR + 16ll * (p.threads / 64);
    const auto up = [](int64_t v) { return (v + 15) / 16 * 16; };
    p.off_wn = 0;
    p.off_wr = up(8ll * n);
    p.off_bin = up(p.off_wr + 8ll * tw);
    p.off_partner = up(p.off_bin + 2ll * n);
    p.bytes = up(p.off_partner + 2ll * n);
    return true;
}

void noise_pack_tables(const NoisePlan& p, char* out) {
    std::fill(out, out + p.bytes, 0);
    float* wn = (float*)(out + p.off_wn);
    for (size_t i = 0; i < p.wn.size(); ++i) wn[2 * i] = (float)p.wn[i].re, wn[2 * i + 1] = (float)p.wn[i].im;
    float* wr = (float*)(out + p.off_wr);
    for (size_t i = 0; i < p.wr.size(); ++i) wr[2 * i] = (float)p.wr[i].re, wr[2 * i + 1] = (float)p.wr[i].im;
    std::copy(p.bin_of_pos.begin(), p.bin_of_pos.end(), (uint16_t*)(out + p.off_bin));
    std::copy(p.partner.begin(), p.partner.end(), (uint16_t*)(out + p.off_partner));
}

}  // namespace plan
}  // namespace mkid
