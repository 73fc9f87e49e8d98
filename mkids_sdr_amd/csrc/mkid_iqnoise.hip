// C ABI of libmkidgpu.so (include/mkidgpu.h): Welch spectra and the IQ noise analysis
// (IQsweep.AnalyzeNoise) — mkid_welch_psd, mkid_iq_noise, their host twins and the stitched
// frequency axis. The rules are welch_common.h's; the kernels are k_welch.hip's.
// The workspace and the per-nfft tables belong to the context: new buffers are allocated into locals
// and moved in only once every allocation has succeeded.
#include <cmath>

#include "mkid_ctx.h"
#include "welch_common.h"

using namespace mkid;

namespace {

#define WELCH_ARGS_MSG                                                                                           \
    "need pointers, nch >= 1, nfft a power of two in 8 .. 262144, nfft <= n < 2^31, ld >= n, group >= 0, finite " \
    "fs > 0"
#define IQN_ARGS_MSG                                                                                               \
    "need pointers, nch >= 1, nfft_low <= n < 2^31, ld >= n, powers of two 8 <= nfft_high <= 4096 < .. nfft_low " \
    "<= 262144 with nfft_high < nfft_low, 1 <= k_join < nfft_high / 2, r k_join <= nfft_low / 2, fit_count >= "  \
    "2, the fit range inside the stitched bins, group >= 0, finite samprate > 0, f_eval, gain and full_scale "    \
    "(the last two not zero)"

constexpr int64_t kWsAlign = 256;
int64_t align_up(int64_t v) { return (v + kWsAlign - 1) / kWsAlign * kWsAlign; }

// How a call at one nfft carves the workspace: per channel the strip sums [nstrips][2][nfft / 2 + 1]
// and, for the four-step transform, a segment of every strip [nstrips][nfft] complex. group = max(1,
// min(nch, 65535, the channels the budget holds, want if want > 0)).
struct WelchWs {
    int64_t nseg, nstrips, part_ch, y_ch, group, y_off, bytes;
};
WelchWs plan_welch(int64_t n, int32_t nfft, int32_t nch, int32_t want) {
    WelchWs w{};
    w.nseg = welch::segments(n, nfft);
    w.nstrips = welch::strips(w.nseg);
    w.part_ch = w.nstrips * 2 * (nfft / 2 + 1) * 8;
    w.y_ch = welch::four_step(nfft) ? w.nstrips * (int64_t)nfft * 16 : 0;
    const int64_t fit = plan::kBankBudget / (w.part_ch + w.y_ch + 2 * kWsAlign);
    w.group = std::max<int64_t>(1, std::min<int64_t>({(int64_t)nch, 65535, fit, want > 0 ? want : INT64_MAX}));
    w.y_off = align_up(w.group * w.part_ch);
    w.bytes = w.y_off + align_up(w.group * w.y_ch);
    return w;
}

// the context's tables for nfft, made and uploaded when a call first brings that length
int tables_for(mkid_ctx* c, int32_t nfft, const mkid_ctx::WelchTab** out) {
    for (const auto& t : c->welch_tabs)
        if (t.nfft == nfft) {
            *out = &t;
            return MKID_OK;
        }
    welch::Tables h;
    welch::make_tables(nfft, h);
    mkid_ctx::WelchTab t;
    HIPCHK(c, t.w.alloc((size_t)nfft));
    HIPCHK(c, t.tw.alloc(2 * (size_t)nfft));
    HIPCHK(c, hipMemcpyAsync(t.w.get(), h.w.data(), (size_t)nfft * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(t.tw.get(), h.tw.data(), (size_t)nfft * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the uploads have left `h`
    t.nfft = nfft, t.S2 = h.S2;
    c->welch_tabs.push_back(std::move(t));
    *out = &c->welch_tabs.back();
    return MKID_OK;
}

// every group of one nfft; `a` holds the source and the sink
int run_groups(mkid_ctx* c, WelchArgs a, const WelchWs& w, const mkid_ctx::WelchTab& t, int32_t nfft, double fs,
               int32_t nch) {
    a.nfft = nfft, a.nseg = w.nseg, a.nstrips = w.nstrips;
    a.w = t.w.get(), a.tw = t.tw.get();
    a.den = fs * t.S2;
    a.part = (double*)c->welchws.get();
    a.y = w.y_ch ? (double*)(c->welchws.get() + w.y_off) : nullptr;
    for (int64_t c0 = 0; c0 < nch; c0 += w.group) {   // the stream orders the groups' use of the workspace
        a.c0 = (int32_t)c0;
        a.g = (int32_t)std::min<int64_t>(w.group, nch - c0);
        HIPCHK(c, launch_welch_group(a, c->stream));
    }
    return MKID_OK;
}

}  // namespace

extern "C" {

int mkid_welch_psd(mkid_ctx* c, const double* d_a, const double* d_b, int64_t n, int64_t ld, int32_t nch,
                   int32_t nfft, double fs, int32_t group, double* d_pa, double* d_pb) {
    if (!c) return MKID_E_ARG;
    if (!welch::psd_args_ok(d_a, n, ld, nch, nfft, fs, group, d_pa)) FAIL(c, MKID_E_ARG, "welch_psd: " WELCH_ARGS_MSG);
    HIPCHK(c, hipSetDevice(c->device));
    const WelchWs w = plan_welch(n, nfft, nch, group);
    if (int rc = c->welchws.reserve(c, (size_t)w.bytes)) return rc;
    const mkid_ctx::WelchTab* t = nullptr;
    if (int rc = tables_for(c, nfft, &t)) return rc;
    WelchArgs a{};
    a.a = d_a, a.b = d_b, a.ld = ld;
    a.out_a = d_pa, a.out_b = d_pb, a.ldo = nfft / 2 + 1, a.off = 0, a.k_lo = 0, a.k_hi = nfft / 2 + 1;
    return run_groups(c, a, w, *t, nfft, fs, nch);
}

int mkid_welch_psd_host(const double* a, const double* b, int64_t n, int64_t ld, int32_t nch, int32_t nfft, double fs,
                        int32_t group, double* pa, double* pb) {
    if (!welch::psd_args_ok(a, n, ld, nch, nfft, fs, group, pa)) return MKID_E_ARG;
    welch::Tables t;
    welch::make_tables(nfft, t);
    const int64_t nb = nfft / 2 + 1;
    for (int64_t ch = 0; ch < nch; ++ch)   // a channel's result does not depend on the grouping
        welch::channel_host(nfft, t, welch::RowLoader{a + ch * ld, b ? b + ch * ld : nullptr}, n, fs,
                            welch::Sink{pa + ch * nb, pb ? pb + ch * nb : nullptr, 0, (int32_t)nb, 0});
    return MKID_OK;
}

int mkid_iq_noise(mkid_ctx* c, const int16_t* d_i, const int16_t* d_q, int64_t n, int64_t ld, int32_t nch,
                  const double* d_i0, const double* d_q0, const double* d_icen, const double* d_qcen,
                  const double* d_qfit, const mkid_iqnoise_cfg* cfg, double* d_pn, double* d_an,
                  mkid_iqnoise_result* d_result) {
    if (!c) return MKID_E_ARG;
    if (!welch::iq_args_ok(d_i, d_q, n, ld, nch, d_i0, d_q0, d_icen, d_qcen, d_qfit, cfg, d_pn, d_an, d_result))
        FAIL(c, MKID_E_ARG, "iq_noise: " IQN_ARGS_MSG);
    HIPCHK(c, hipSetDevice(c->device));
    const WelchWs wl = plan_welch(n, cfg->nfft_low, nch, cfg->group), wh = plan_welch(n, cfg->nfft_high, nch, cfg->group);
    if (int rc = c->welchws.reserve(c, (size_t)std::max(wl.bytes, wh.bytes))) return rc;
    const mkid_ctx::WelchTab *tl = nullptr, *th = nullptr;
    if (int rc = tables_for(c, cfg->nfft_low, &tl)) return rc;
    if (int rc = tables_for(c, cfg->nfft_high, &th)) return rc;
    for (const auto& t : c->welch_tabs)   // the second may have moved the first
        if (t.nfft == cfg->nfft_low) tl = &t;
    IqNoiseArgs q{};
    q.xi = d_i, q.xq = d_q, q.i0 = d_i0, q.q0 = d_q0, q.icen = d_icen, q.qcen = d_qcen, q.qfit = d_qfit;
    q.res = d_result, q.pn = d_pn, q.an = d_an, q.cfg = *cfg, q.n = n, q.ld = ld, q.nch = nch;
    HIPCHK(c, launch_iq_means(q, c->stream));
    WelchArgs a{};
    a.xi = d_i, a.xq = d_q, a.i0 = d_i0, a.q0 = d_q0, a.icen = d_icen, a.qcen = d_qcen, a.res = d_result;
    a.cfg = *cfg, a.ld = ld, a.out_a = d_pn, a.out_b = d_an, a.ldo = welch::iq_nout(*cfg);
    const welch::Sink lo = welch::iq_sink_low(*cfg, nullptr, nullptr), hi = welch::iq_sink_high(*cfg, nullptr, nullptr);
    a.k_lo = lo.k_lo, a.k_hi = lo.k_hi, a.off = lo.off;
    if (int rc = run_groups(c, a, wl, *tl, cfg->nfft_low, cfg->samprate, nch)) return rc;
    a.k_lo = hi.k_lo, a.k_hi = hi.k_hi, a.off = hi.off;
    if (int rc = run_groups(c, a, wh, *th, cfg->nfft_high, cfg->samprate, nch)) return rc;
    HIPCHK(c, launch_iq_fn1k(q, c->stream));
    return MKID_OK;
}

int mkid_iq_noise_host(const int16_t* i, const int16_t* q, int64_t n, int64_t ld, int32_t nch, const double* i0,
                       const double* q0, const double* icen, const double* qcen, const double* qfit,
                       const mkid_iqnoise_cfg* cfg, double* pn, double* an, mkid_iqnoise_result* result) {
    if (!welch::iq_args_ok(i, q, n, ld, nch, i0, q0, icen, qcen, qfit, cfg, pn, an, result)) return MKID_E_ARG;
    welch::Tables tl, th;
    welch::make_tables(cfg->nfft_low, tl);
    welch::make_tables(cfg->nfft_high, th);
    const int32_t nout = welch::iq_nout(*cfg);
    for (int64_t ch = 0; ch < nch; ++ch) {
        const int16_t *xi = i + ch * ld, *xq = q + ch * ld;
        int64_t si = 0, sq = 0;
        for (int64_t j = 0; j < n; ++j) si += xi[j], sq += xq[j];
        mkid_iqnoise_result& r = result[ch];
        welch::iq_means(si, sq, n, *cfg, i0[ch], q0[ch], icen[ch], qcen[ch], qfit[ch], &r);
        double *p = pn + ch * nout, *a = an + ch * nout;
        const welch::IqLoader ld_(xi, xq, *cfg, i0[ch], q0[ch], icen[ch], qcen[ch], r);
        welch::channel_host(cfg->nfft_low, tl, ld_, n, cfg->samprate, welch::iq_sink_low(*cfg, p, a));
        welch::channel_host(cfg->nfft_high, th, ld_, n, cfg->samprate, welch::iq_sink_high(*cfg, p, a));
        if (r.status & MKID_IQN_BAD_RAD)
            for (int32_t b = 0; b < nout; ++b) p[b] = welch::nan64(), a[b] = welch::nan64();
        r.fn1k = welch::iq_fn1k(*cfg, p, qfit[ch], r.status);
    }
    return MKID_OK;
}

int mkid_iq_noise_freqs(const mkid_iqnoise_cfg* cfg, double* freqs) {
    if (!freqs || !welch::iq_cfg_ok(cfg)) return MKID_E_ARG;
    for (int32_t b = 0; b < welch::iq_nout(*cfg); ++b) freqs[b] = welch::iq_freq(*cfg, b);
    return MKID_OK;
}

}  // extern "C"
