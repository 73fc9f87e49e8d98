// C ABI of libmkidgpu.so (include/mkidgpu.h): calibration and pulse analysis — replay trigger,
// template, optimal filter, bank filters, pulse heights, the pulse-height fit, pulse capture, phase thresholds, phase-noise
// spectra, the laser lines of the pulse-height spectra with the energy calibration, the resonator loop
// fits, the synthetic ADC stream, stream copy.
// Every entry point that replaces buffers of the context allocates the new ones into locals and
// moves them in, with the scalars that describe them, only once every allocation has succeeded.
#include <cmath>

#include "fit_common.h"
#include "loopfit_common.h"
#include "magfit_common.h"
#include "mkid_ctx.h"
#include "noise_common.h"
#include "thr_common.h"
#include "wavecal_common.h"

using namespace mkid;

extern "C" {

int mkid_replay_trigger(mkid_ctx* c, const int16_t* d_raw, int64_t n, int64_t ld, int32_t nch,
                        const mkid_replay_cfg* rc, int32_t* d_hits, int32_t cap, int32_t* d_counts) {
    if (!c || !d_raw || !rc || !d_counts || (cap > 0 && !d_hits)) return MKID_E_ARG;
    if (n <= 0 || nch <= 0 || ld < nch || cap < 0) FAIL(c, MKID_E_ARG, "replay: bad shape");
    if (rc->mode != MKID_REPLAY_ROLLING && rc->mode != MKID_REPLAY_BLOCK) FAIL(c, MKID_E_ARG, "replay: bad mode");
    if (rc->length <= 0 || rc->start < 0 || rc->need < 0 || rc->skip <= 0)
        FAIL(c, MKID_E_ARG, "replay: length/start/need/skip out of range");
    if (rc->mode == MKID_REPLAY_ROLLING && rc->start < rc->length)
        FAIL(c, MKID_E_ARG, "replay: rolling start must be >= meanlength");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nf = (size_t)nch * (size_t)((n + 31) / 32);
    const size_t nm = rc->mode == MKID_REPLAY_BLOCK ? (size_t)nch * (size_t)(n / rc->length) : 0;
    if (int err = c->rflags.reserve(c, nf)) return err;
    if (int err = c->rmeans.reserve(c, nm)) return err;
    HIPCHK(c, launch_replay(d_raw, n, ld, nch, rc->mode, rc->length, rc->start, rc->need, rc->skip,
                            rc->wrap_negative, rc->threshold_deg, c->rflags.get(), c->rmeans.get(), d_hits, cap,
                            d_counts, c->stream));
    return MKID_OK;
}

// The workspace tables of `a` for one group of the plan `w`, in the context's bank workspace (grown
// first where it is smaller).
static int bank_tables(mkid_ctx* c, const plan::BankWs& w, BankArgs& a) {
    if (int rc = c->bankws.reserve(c, (size_t)w.bytes)) return rc;
    char* p = c->bankws.get();
    a.rows = (double*)(p + w.rows), a.nrows = (double*)(p + w.nrows), a.peaks = (double*)(p + w.peaks);
    a.scratch = (double*)(p + w.scratch), a.tP = (double*)(p + w.tP), a.tPf = (double*)(p + w.tPf);
    a.noise = (double*)(p + w.noise), a.stats = (double*)(p + w.stats), a.work = (double*)(p + w.work);
    a.coeff = (double*)(p + w.coeff), a.refmed = (float*)(p + w.refmed), a.accept = (int32_t*)(p + w.accept);
    a.appended = (int32_t*)(p + w.appended), a.status = (int32_t*)(p + w.status);
    a.nready = (int32_t*)(p + w.nready);
    return MKID_OK;
}

// The bank kernels on one channel whose P records are all ready, without the filter; the finish
// kernel writes the caller's template and noise at status 0 only.
int mkid_make_template(mkid_ctx* c, const float* d_I, const float* d_Q, int64_t P, double* d_template,
                       double* d_noise, mkid_template_info* info) {
    if (!c || !d_I || !d_Q || !d_template || !d_noise || !info) return MKID_E_ARG;
    if (P <= 0) FAIL(c, MKID_E_ARG, "make_template: need pulses");
    if (P > INT32_MAX) FAIL(c, MKID_E_ARG, "make_template: more than 2^31 - 1 pulses");
    HIPCHK(c, hipSetDevice(c->device));
    BankArgs a{};
    if (int rc = bank_tables(c, plan::plan_bank(1, P, plan::kBankBudget), a)) return rc;
    if (!c->d_tplslot.get()) HIPCHK(c, c->d_tplslot.alloc(1));
    mkid_ctx::TplSlot* slot = c->d_tplslot.get();
    a.I = d_I, a.Q = d_Q, a.ready = &slot->ready;
    a.out_tpl = d_template, a.out_noise = d_noise, a.result = &slot->result;
    a.g = 1, a.R = (int32_t)P, a.ready_stride = 1;
    const int32_t ready = (int32_t)P;
    mkid_bank_result r{};
    hipStream_t s = c->stream;
    hipError_t e = hipMemcpyAsync(&slot->ready, &ready, sizeof ready, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_bank_filters(a, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&r, &slot->result, sizeof r, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);   // whatever was enqueued: both copies use this frame
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        c->err = std::string("make_template: ") + hipGetErrorString(e);
        return MKID_E_HIP;
    }
    if (r.status == 2) FAIL(c, MKID_E_STATE, "make_template: no pulse passed the first pass");
    // nothing accepted in pass 2: the column means are 0 / 0
    if (r.status != 0) FAIL(c, MKID_E_STATE, "make_template: no pulse passed the second pass");
    info->count = r.count;
    info->count1 = r.count1;
    info->pm = r.pm;
    info->pdev = r.pdev;
    info->flag = r.flag;
    info->pstart = r.pstart;
    return MKID_OK;
}

int mkid_optimal_filter(mkid_ctx* c, const double* d_template, const double* d_noise, int32_t pre, int32_t ncoeff,
                        double* d_coeff) {
    if (!c || !d_template || !d_noise || !d_coeff) return MKID_E_ARG;
    if (pre < 10 || pre > 2000 || ncoeff <= 0 || ncoeff > 800) FAIL(c, MKID_E_ARG, "optimal_filter: bad pre/ncoeff");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> work;
    HIPCHK(c, work.alloc(3 * 800));
    HIPCHK(c, launch_optimal_filter(d_template, d_noise, pre, ncoeff, d_coeff, work.get(), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MKID_OK;
}

int mkid_bank_filters(mkid_ctx* c, const float* d_I, const float* d_Q, const int32_t* d_ready,
                      const mkid_bank_cfg* bc, double* d_templates, double* d_noise, float* d_coeff,
                      mkid_bank_result* d_result) {
    if (!c || !d_I || !d_ready || !bc || !d_coeff || !d_result) return MKID_E_ARG;
    if (bc->length != 2000) FAIL(c, MKID_E_ARG, "bank_filters: records must be 2000 rows long");
    if (bc->n_channels < 1 || bc->max_per_ch < 1) FAIL(c, MKID_E_ARG, "bank_filters: need channels and records");
    if (bc->pre < 10 || bc->pre > 2000 || bc->ncoeff <= 0 || bc->ncoeff > 800)
        FAIL(c, MKID_E_ARG, "bank_filters: bad pre/ncoeff");
    if (bc->ready_stride < 1 || bc->group < 0) FAIL(c, MKID_E_ARG, "bank_filters: bad ready_stride/group");
    if (!d_Q && !(std::isfinite(bc->sign) && bc->sign != 0.0f))
        FAIL(c, MKID_E_ARG, "bank_filters: phase mode needs a finite, non-zero sign");
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t Cb = bc->n_channels;
    const plan::BankWs w = plan::plan_bank(Cb, bc->max_per_ch, plan::kBankBudget, bc->group);
    BankArgs a{};
    if (int rc = bank_tables(c, w, a)) return rc;
    a.I = d_I, a.Q = d_Q, a.ready = d_ready;
    a.out_tpl = d_templates, a.out_noise = d_noise, a.out_coeff = d_coeff, a.result = d_result;
    a.R = bc->max_per_ch, a.ready_stride = bc->ready_stride, a.min_records = bc->min_records;
    a.pre = bc->pre, a.ncoeff = bc->ncoeff, a.sign = bc->sign;
    for (int64_t c0 = 0; c0 < Cb; c0 += w.group) {   // the stream orders the groups' use of the tables
        a.c0 = (int32_t)c0;
        a.g = (int32_t)std::min<int64_t>(w.group, Cb - c0);
        HIPCHK(c, launch_bank_filters(a, c->stream));
    }
    return MKID_OK;
}

// mkid_set_pulse_filter and mkid_set_pulse_filter_device: the table comes from host or device memory
static int set_pulse_filter(mkid_ctx* c, const float* coeff, int32_t nch, int32_t ncoeff, int32_t pre,
                            hipMemcpyKind kind) {
    if (!c || !coeff) return MKID_E_ARG;
    if (nch != c->C) FAIL(c, MKID_E_ARG, "pulse filter: need one filter per channel");
    if (ncoeff < 1 || ncoeff > 4096 || pre < 0) FAIL(c, MKID_E_ARG, "pulse filter: bad ncoeff/pre");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> co;
    RollBuf<float> hist, fhist;
    const int64_t fit_rows = ncoeff + 2 * (int64_t)std::max(c->fit_L, 0);
    HIPCHK(c, co.alloc((size_t)nch * ncoeff));
    HIPCHK(c, hist.alloc(ncoeff, (int64_t)nch * 4));
    if (c->fit_L >= 0) HIPCHK(c, fhist.alloc(fit_rows, (int64_t)nch * 4));
    // the copy drains the stream: no kernel still reads the filter and the rows replaced below
    HIPCHK(c, hipMemcpyAsync(co.get(), coeff, (size_t)nch * ncoeff * 4, kind, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->d_hcoeff = std::move(co);
    c->phist = std::move(hist);
    c->pcarry = plan::Carry{ncoeff};   // the rows carried for the old filter are forgotten
    if (c->fit_L >= 0) {
        c->fhist = std::move(fhist);
        c->fcarry = plan::Carry{fit_rows};
    }
    c->h_ncoeff = ncoeff;
    c->h_pre = pre;
    return MKID_OK;
}

int mkid_set_pulse_filter(mkid_ctx* c, const float* coeff, int32_t nch, int32_t ncoeff, int32_t pre) {
    return set_pulse_filter(c, coeff, nch, ncoeff, pre, hipMemcpyHostToDevice);
}

int mkid_set_pulse_filter_device(mkid_ctx* c, const float* d_coeff, int32_t nch, int32_t ncoeff, int32_t pre) {
    return set_pulse_filter(c, d_coeff, nch, ncoeff, pre, hipMemcpyDeviceToDevice);
}

static int pulse_heights(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events,
                         const int64_t* d_n, int64_t n, float* d_heights) {
    if (!c || (n > 0 && (!d_phase || !d_events || !d_heights))) return MKID_E_ARG;
    if (rows < 0 || j0 < 0 || n < 0) FAIL(c, MKID_E_ARG, "pulse heights: negative rows/j0/n");
    if (!c->d_hcoeff.get()) FAIL(c, MKID_E_STATE, "pulse heights: no filter set (mkid_set_pulse_filter)");
    HIPCHK(c, hipSetDevice(c->device));
    // the carried rows precede this call's rows only if the calls are contiguous in j
    const plan::Carry& k = c->pcarry;
    HeightArgs a{d_phase, d_events, c->d_hcoeff.get(), d_heights, rows, j0, n, c->C, c->h_ncoeff, c->h_pre, d_n,
                 c->phist.get() + k.offset(j0) * c->C, k.before(j0), c->ncu, 0};
    KTime kt;
    tstart(c, MKID_K_HEIGHTS, &kt, c->stream);
    HIPCHK(c, launch_pulse_heights(a, c->stream));
    tstop(c, &kt, c->stream);
    // keep the last h_ncoeff rows of (history, these rows) for the next call's early windows
    if (rows > 0) {
        HIPCHK(c, c->phist.roll(d_phase, rows, c->stream));
        c->pcarry.advance(j0, rows);
    }
    return MKID_OK;
}

int mkid_pulse_heights(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events,
                       int64_t n, float* d_heights) {
    return pulse_heights(c, d_phase, rows, j0, d_events, nullptr, n, d_heights);
}

int mkid_pulse_heights_counted(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0,
                               const uint64_t* d_events, const int64_t* d_count, int64_t cap, float* d_heights) {
    if (!d_count) return MKID_E_ARG;
    return pulse_heights(c, d_phase, rows, j0, d_events, d_count, cap, d_heights);
}

// ---- pulse heights with a lag search and a parabolic vertex (fit_common.h) ------------------------
int mkid_set_pulse_fit(mkid_ctx* c, int32_t search, int32_t polarity) {
    if (!c) return MKID_E_ARG;
    if (!fit::params_ok(search, polarity)) FAIL(c, MKID_E_ARG, "pulse fit: need 0 <= search <= 31, polarity +1 or -1");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->h_ncoeff > 0) {   // else mkid_set_pulse_filter allocates the rows
        const int64_t fit_rows = c->h_ncoeff + 2 * (int64_t)search;
        RollBuf<float> fhist;
        HIPCHK(c, fhist.alloc(fit_rows, (int64_t)c->C * 4));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // an earlier fit may still read the old rows
        c->fhist = std::move(fhist);
        c->fcarry = plan::Carry{fit_rows};
    }
    c->fit_L = search;
    c->fit_s = polarity;
    return MKID_OK;
}

static int pulse_fit(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events,
                     const int64_t* d_n, int64_t n, float* d_heights, float* d_dt, int32_t* d_lag, float* d_h0) {
    if (!c || (rows > 0 && !d_phase) || (n > 0 && (!d_events || !d_heights))) return MKID_E_ARG;
    if (rows < 0 || j0 < 0 || n < 0) FAIL(c, MKID_E_ARG, "pulse fit: negative rows/j0/n");
    if (!c->d_hcoeff.get()) FAIL(c, MKID_E_STATE, "pulse fit: no filter set (mkid_set_pulse_filter)");
    if (c->fit_L < 0) FAIL(c, MKID_E_STATE, "pulse fit: not configured (mkid_set_pulse_fit)");
    HIPCHK(c, hipSetDevice(c->device));
    const plan::Carry& k = c->fcarry;
    const plan::FitPlan p = plan::plan_fit(c->h_ncoeff, c->fit_L, c->ncu);
    FitArgs a{};
    a.phase = d_phase, a.hist = c->fhist.get() + k.offset(j0) * c->C, a.events = d_events;
    a.coeff = c->d_hcoeff.get(), a.d_n = d_n;
    a.heights = d_heights, a.dt = d_dt, a.lag = d_lag, a.h0 = d_h0;
    a.rows = rows, a.j0 = j0, a.n = n, a.hrows = k.before(j0);
    a.C = c->C, a.ncoeff = c->h_ncoeff, a.pre = c->h_pre, a.L = c->fit_L, a.s = c->fit_s;
    HIPCHK(c, launch_pulse_fit(a, p, c->stream));
    // keep the last rows of (carried rows, these rows) for the next call's early windows
    if (rows > 0) {
        HIPCHK(c, c->fhist.roll(d_phase, rows, c->stream));
        c->fcarry.advance(j0, rows);
    }
    return MKID_OK;
}

int mkid_pulse_fit(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events, int64_t n,
                   float* d_heights, float* d_dt, int32_t* d_lag, float* d_h0) {
    return pulse_fit(c, d_phase, rows, j0, d_events, nullptr, n, d_heights, d_dt, d_lag, d_h0);
}

int mkid_pulse_fit_counted(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events,
                           const int64_t* d_count, int64_t cap, float* d_heights, float* d_dt, int32_t* d_lag,
                           float* d_h0) {
    if (!d_count) return MKID_E_ARG;
    return pulse_fit(c, d_phase, rows, j0, d_events, d_count, cap, d_heights, d_dt, d_lag, d_h0);
}

// The CPU statement of the device call: the same decode, window test and selection (fit_common.h)
// on lag values accumulated in float64; no carried rows.
int mkid_pulse_fit_host(const float* phase, int64_t rows, int32_t C, int64_t j0, const uint64_t* events, int64_t n,
                        const float* coeff, int32_t ncoeff, int32_t pre, int32_t search, int32_t polarity,
                        double* heights, double* dt, int32_t* lag, double* h0) {
    if (!coeff || (rows > 0 && !phase) || (n > 0 && (!events || !heights))) return MKID_E_ARG;
    if (rows < 0 || j0 < 0 || n < 0 || C < 1 || C > 4096 || ncoeff < 1 || ncoeff > fit::kMaxCoeff || pre < 0 ||
        !fit::params_ok(search, polarity))
        return MKID_E_ARG;
    double H[2 * fit::kMaxSearch + 1];
    for (int64_t p = 0; p < n; ++p) {
        const pkt::Stamp st = pkt::decode(events[p], j0);
        const int64_t r0 = st.jg - j0 - pre;
        fit::Result<double> r{NAN, NAN, NAN, INT32_MIN};
        if (fit::inside(st.ch, C, r0, search, ncoeff, 0, rows)) {
            const float* cf = coeff + (size_t)st.ch * ncoeff;
            for (int32_t d = -search; d <= search; ++d) {
                double acc = 0.0;
                for (int32_t i = 0; i < ncoeff; ++i) acc += (double)cf[i] * (double)phase[(r0 + d + i) * C + st.ch];
                H[d + search] = acc;
            }
            r = fit::select<double>(H, search, polarity);
        }
        heights[p] = r.height;
        if (dt) dt[p] = r.dt;
        if (lag) lag[p] = r.lag;
        if (h0) h0[p] = r.h0;
    }
    return MKID_OK;
}

int mkid_set_capture(mkid_ctx* c, int32_t length, int32_t pre, int32_t max_per_ch) {
    if (!c) return MKID_E_ARG;
    if (length < 1 || length > 4096 || pre < 0 || pre >= length || max_per_ch < 1)
        FAIL(c, MKID_E_ARG, "capture: need 1 <= length <= 4096, 0 <= pre < length, max_per_ch >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t H = std::max<int64_t>(length - 1, pre + 1);   // rows carried
    // windows still open after a call have stamps in (j_end - (length - pre), j_end): packets at
    // least max(dead_time, 1) rows apart (trig_common.h) never outnumber this
    const int32_t PC = (length - pre) / std::max(c->cfg.dead_time, 1) + 2;
    const size_t C = (size_t)c->C;
    RollBuf<float> hist;
    DevBuf<int64_t> pend[2];
    DevBuf<int32_t> pend_n[2], work;
    hipError_t e = hist.alloc(H, (int64_t)C * 4);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = pend[b].alloc(C * PC);
        if (e == hipSuccess) e = pend_n[b].alloc(C);
    }
    if (e == hipSuccess) e = work.alloc(2 * C);
    if (e != hipSuccess) {   // the context keeps the capture it had (or none)
        c->err = std::string("capture: hipMalloc: ") + hipGetErrorString(e);
        return MKID_E_HIP;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // an earlier capture may still read the old buffers
    c->chist = std::move(hist);
    for (int b = 0; b < 2; ++b) c->d_cpend[b] = std::move(pend[b]), c->d_cpend_n[b] = std::move(pend_n[b]);
    c->d_cwork = std::move(work);
    c->cap_L = length; c->cap_pre = pre; c->cap_R = max_per_ch; c->cap_PC = PC;
    c->cpend_cur = 0;
    c->ccarry = plan::Carry{H};   // no segment
    return MKID_OK;
}

static int capture_pulses(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events,
                          const int64_t* d_n, int64_t n, float* d_records, int64_t* d_stamps, int32_t* d_info) {
    if (!c || (rows > 0 && !d_phase) || (n > 0 && !d_events) || !d_records || !d_stamps || !d_info)
        return MKID_E_ARG;
    if (rows < 0 || j0 < 0 || n < 0) FAIL(c, MKID_E_ARG, "capture: negative rows/j0/n");
    if (c->cap_L <= 0) FAIL(c, MKID_E_STATE, "capture: not configured (mkid_set_capture)");
    HIPCHK(c, hipSetDevice(c->device));
    const int cur = c->cpend_cur;
    plan::Carry& k = c->ccarry;
    if (k.end != j0) {   // a new segment: no carried rows, no pending packets
        k.drop();        // until this call's launches are in, no segment stands
        HIPCHK(c, hipMemsetAsync(c->d_cpend_n[cur].get(), 0, (size_t)c->C * 4, c->stream));
    }
    CaptureArgs a{d_phase, c->chist.get() + k.offset(j0) * c->C, d_events, d_n, d_records, d_stamps, d_info,
                  c->d_cpend[cur].get(), c->d_cpend_n[cur].get(), c->d_cpend[cur ^ 1].get(),
                  c->d_cpend_n[cur ^ 1].get(), c->d_cwork.get(),
                  rows, j0, n, k.before(j0), c->C, c->cap_L, c->cap_pre, c->cap_R, c->cap_PC, 0};
    KTime kt;
    tstart(c, MKID_K_CAPTURE, &kt, c->stream);
    hipError_t e = launch_capture(a, c->stream);
    tstop(c, &kt, c->stream);
    if (e == hipSuccess && rows > 0)   // keep the last rows of (carried rows, these rows)
        e = c->chist.roll(d_phase, rows, c->stream);
    if (e != hipSuccess) {   // partly enqueued: the segment ends here
        k.drop();
        c->err = std::string("capture launch: ") + hipGetErrorString(e);
        return MKID_E_HIP;
    }
    c->cpend_cur = cur ^ 1;
    k.advance(j0, rows);
    return MKID_OK;
}

int mkid_capture_pulses(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0, const uint64_t* d_events,
                        int64_t n, float* d_records, int64_t* d_stamps, int32_t* d_info) {
    return capture_pulses(c, d_phase, rows, j0, d_events, nullptr, n, d_records, d_stamps, d_info);
}

int mkid_capture_pulses_counted(mkid_ctx* c, const float* d_phase, int64_t rows, int64_t j0,
                                const uint64_t* d_events, const int64_t* d_count, int64_t cap, float* d_records,
                                int64_t* d_stamps, int32_t* d_info) {
    if (!d_count) return MKID_E_ARG;
    return capture_pulses(c, d_phase, rows, j0, d_events, d_count, cap, d_records, d_stamps, d_info);
}

// ---- thresholds from a phase block (loadThresholds) ----------------------------------------------
static bool thr_args_ok(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, double nsigma, const int32_t* thr) {
    return raw && thr && rows >= 1 && rows <= INT32_MAX && nch >= 1 && ld >= nch && std::isfinite(nsigma) &&
           nsigma >= 0.0;
}

int mkid_phase_thresholds(mkid_ctx* c, const int16_t* d_raw, int64_t rows, int64_t ld, int32_t nch, double nsigma,
                          int32_t* d_thr, mkid_thr_stats* d_stats) {
    if (!c) return MKID_E_ARG;
    if (!thr_args_ok(d_raw, rows, ld, nch, nsigma, d_thr))
        FAIL(c, MKID_E_ARG, "phase_thresholds: need pointers, 1 <= rows < 2^31, 1 <= nch <= ld, finite nsigma >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    const plan::ThrPlan p = plan::plan_thresholds(rows, ld, nch, ((uintptr_t)d_raw & 15) == 0, c->ncu);
    if (int rc = c->thrws.reserve(c, (size_t)p.bytes)) return rc;
    HIPCHK(c, launch_thresholds(d_raw, rows, ld, nch, nsigma, p, c->thrws.get(), d_thr, d_stats, c->stream));
    return MKID_OK;
}

int mkid_phase_thresholds_block_rows(const mkid_ctx* c, int64_t rows, int64_t ld, int32_t nch, int32_t aligned16,
                                     int64_t* block_rows) {
    if (!c || !block_rows || rows < 1 || rows > INT32_MAX || nch < 1 || ld < nch) return MKID_E_ARG;
    *block_rows = plan::plan_thresholds(rows, ld, nch, aligned16 != 0, c->ncu).B;
    return MKID_OK;
}

// The CPU statement of the device call: the same cut tables, bin rule, prefix sums and finish
// (thr_common.h), one channel at a time.
int mkid_phase_thresholds_host(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, double nsigma,
                               int32_t* thr_out, mkid_thr_stats* stats) {
    if (!thr_args_ok(raw, rows, ld, nch, nsigma, thr_out)) return MKID_E_ARG;
    for (int32_t ch = 0; ch < nch; ++ch) {
        const int16_t* x = raw + ch;
        int32_t lo = x[0], hi = x[0];
        for (int64_t r = 1; r < rows; ++r) lo = std::min<int32_t>(lo, x[r * ld]), hi = std::max<int32_t>(hi, x[r * ld]);
        const thr::Range rg = thr::make_range(lo, hi);
        int32_t ct[thr::kBins + 1];
        ct[0] = INT32_MIN, ct[thr::kBins] = INT32_MAX;
        for (int i = 1; i < thr::kBins; ++i) ct[i] = thr::cut(rg, i);
        uint32_t count[thr::kBins] = {0};
        int b = 0;   // the estimate: the previous sample's bin
        for (int64_t r = 0; r < rows; ++r) {
            b = thr::bin_of(x[r * ld], ct, b);
            ++count[b];
        }
        double n[thr::kBins];
        for (int i = 0; i < thr::kBins; ++i) n[i] = thr::fraction(count[i], rows);
        const thr::Pick p = thr::pick_scan([&n](int i) { return n[i]; }, 0, 1);
        thr_out[ch] = thr::finish(lo, hi, p, nsigma, stats ? &stats[ch] : nullptr);
    }
    return MKID_OK;
}

// ---- phase-noise spectra from a phase block (longsnapshot's noise FFT) ----------------------------
static bool noise_args_ok(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, int32_t n_averages, double scale,
                          double norm1, const double* spec) {
    return raw && spec && rows >= 1 && rows <= INT32_MAX && nch >= 1 && ld >= nch && n_averages >= 1 &&
           n_averages <= rows && rows / n_averages <= MKID_NOISE_MAX_N && std::isfinite(scale) && scale > 0.0 &&
           std::isfinite(norm1) && norm1 > 0.0;
}
#define NOISE_ARGS_MSG \
    "need pointers, 1 <= rows < 2^31, 1 <= nch <= ld, 1 <= n_averages <= rows, rows / n_averages <= 16384, finite scale, norm1 > 0"

// spec = mul * (sum over the pieces of log2 |X|^2) + add
static void noise_constants(int32_t n_averages, double scale, double norm1, double& mul, double& add) {
    mul = 10.0 * std::log10(2.0) / (double)n_averages;
    add = 20.0 * std::log10(scale / norm1 / 1e-6);
}

int mkid_phase_noise_spectra(mkid_ctx* c, const int16_t* d_raw, int64_t rows, int64_t ld, int32_t nch,
                             int32_t n_averages, double scale, double norm1, double* d_spec) {
    if (!c) return MKID_E_ARG;
    if (!noise_args_ok(d_raw, rows, ld, nch, n_averages, scale, norm1, d_spec))
        FAIL(c, MKID_E_ARG, "phase_noise_spectra: " NOISE_ARGS_MSG);
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t n = (int32_t)(rows / n_averages);
    if (c->noise_plan.n != n) {   // another n: make its tables, then replace the old ones
        plan::NoisePlan p;
        if (!plan::plan_noise(n, p)) FAIL(c, MKID_E_ARG, "phase_noise_spectra: no plan for this n");
        std::vector<char> image((size_t)p.bytes);
        plan::noise_pack_tables(p, image.data());
        DevBuf<char> tab;
        HIPCHK(c, tab.alloc((size_t)p.bytes));
        HIPCHK(c, hipMemcpyAsync(tab.get(), image.data(), (size_t)p.bytes, hipMemcpyHostToDevice, c->stream));
        // the upload has left `image`, and an earlier call may still use the old tables
        HIPCHK(c, hipStreamSynchronize(c->stream));
        p.wn = {}, p.wr = {}, p.bin_of_pos = {}, p.partner = {};   // the context keeps passes and offsets
        c->d_noisetab = std::move(tab), c->noise_plan = std::move(p);
    }
    double mul, add;
    noise_constants(n_averages, scale, norm1, mul, add);
    HIPCHK(c, launch_noise(d_raw, ld, nch, n_averages, mul, add, c->noise_plan, c->d_noisetab.get(), d_spec, c->stream));
    return MKID_OK;
}

// The CPU statement of the device call: the same plan, passes, unpacking and finish
// (noise_common.h) in float64, one channel at a time.
int mkid_phase_noise_spectra_host(const int16_t* raw, int64_t rows, int64_t ld, int32_t nch, int32_t n_averages,
                                  double scale, double norm1, double* spec) {
    if (!noise_args_ok(raw, rows, ld, nch, n_averages, scale, norm1, spec)) return MKID_E_ARG;
    const int32_t n = (int32_t)(rows / n_averages);
    plan::NoisePlan p;
    if (!plan::plan_noise(n, p)) return MKID_E_ARG;
    const noise::View<double> v{n, (int32_t)p.passes.size(), p.passes.data(), p.wn.data(), p.wr.data(),
                                p.bin_of_pos.data(), p.partner.data()};
    double mul, add;
    noise_constants(n_averages, scale, norm1, mul, add);
    std::vector<noise::Cx<double>> z((size_t)n), y((size_t)n);
    std::vector<double> acc((size_t)n);
    for (int32_t ch = 0; ch < nch; ++ch) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int32_t a = 0; a < n_averages; a += 2) {
            const int16_t* colA = raw + (int64_t)a * n * ld + ch;
            const int16_t* colB = a + 1 < n_averages ? colA + (int64_t)n * ld : nullptr;
            noise::pair_host<double>(v, colA, colB, ld, z.data(), y.data(), acc.data(),
                                     [](double x) { return std::log2(x); });
        }
        for (int32_t pos = 0; pos < n; ++pos)
            spec[(int64_t)ch * n + p.bin_of_pos[(size_t)pos]] = noise::finish(acc[(size_t)pos], mul, add);
    }
    return MKID_OK;
}

// ---- laser lines and the energy calibration from the pulse-height spectra (wavecal_common.h) -----
#define LINES_ARGS_MSG                                                                                               \
    "need pointers, nch >= 1, 1 <= nbins <= 16384, 1 <= n_lines <= 3, finite, positive, distinct energies, "        \
    "0 <= smooth <= 64, min_sep >= 1, 1 <= fit_half <= 64"

int mkid_spectrum_lines(mkid_ctx* c, const int32_t* d_spectra, const float* d_lo, const float* d_step, int32_t nch,
                        int32_t nbins, int32_t n_lines, const double* energies, int32_t smooth, int32_t min_sep,
                        int64_t min_peak, int32_t fit_half, mkid_line_fit* d_lines, mkid_energy_cal* d_cal,
                        float* d_cal_f) {
    if (!c) return MKID_E_ARG;
    if (!wcal::lines_args_ok(d_spectra, d_lo, d_step, nch, nbins, n_lines, energies, smooth, min_sep, fit_half, d_lines,
                             d_cal, d_cal_f))
        FAIL(c, MKID_E_ARG, "spectrum_lines: " LINES_ARGS_MSG);
    HIPCHK(c, hipSetDevice(c->device));
    WcalLinesArgs a{};
    a.spectra = d_spectra, a.lo = d_lo, a.step = d_step, a.lines = d_lines, a.cal = d_cal, a.cal_f = d_cal_f;
    a.min_peak = min_peak, a.nbins = nbins, a.P = n_lines, a.w = smooth, a.min_sep = min_sep, a.g = fit_half;
    for (int32_t p = 0; p < MKID_CAL_MAX_LINES; ++p) a.E[p] = p < n_lines ? energies[p] : NAN;
    HIPCHK(c, launch_spectrum_lines(a, nch, c->stream));
    return MKID_OK;
}

// The CPU statement of the device call: the loops of wavecal_common.h.
int mkid_spectrum_lines_host(const int32_t* spectra, const float* lo, const float* step, int32_t nch, int32_t nbins,
                             int32_t n_lines, const double* energies, int32_t smooth, int32_t min_sep,
                             int64_t min_peak, int32_t fit_half, mkid_line_fit* lines, mkid_energy_cal* cal,
                             float* cal_f) {
    if (!wcal::lines_args_ok(spectra, lo, step, nch, nbins, n_lines, energies, smooth, min_sep, fit_half, lines, cal,
                             cal_f))
        return MKID_E_ARG;
    wcal::lines_host(spectra, lo, step, nch, wcal::make_params(nbins, n_lines, energies, smooth, min_sep, min_peak, fit_half),
                     lines, cal, cal_f);
    return MKID_OK;
}

// ---- resonator loop fits (loopfit_common.h) ----------------------------------------------------------
#define LOOPS_ARGS_MSG                                                                                             \
    "need pointers (d_isd and d_qsd both or neither), nch >= 1, 12 <= fsteps <= 1024, 1 <= n_starts <= 16, "      \
    "max_iter >= 1, ftol > 0"

int mkid_fit_loops(mkid_ctx* c, const double* d_freq, const double* d_i, const double* d_q, const double* d_isd,
                   const double* d_qsd, const double* d_draws, const double* d_qguess, int32_t nch, int32_t fsteps,
                   int32_t n_starts, int32_t max_iter, double ftol, mkid_loop_fit* d_fits, double* d_chisq_all) {
    if (!c) return MKID_E_ARG;
    if (!lfit::args_ok(d_freq, d_i, d_q, d_isd, d_qsd, d_draws, nch, fsteps, n_starts, max_iter, ftol, d_fits))
        FAIL(c, MKID_E_ARG, "fit_loops: " LOOPS_ARGS_MSG);
    HIPCHK(c, hipSetDevice(c->device));
    LoopfitArgs a{};
    a.freq = d_freq, a.i = d_i, a.q = d_q, a.isd = d_isd, a.qsd = d_qsd, a.draws = d_draws, a.qguess = d_qguess;
    a.fits = d_fits, a.chisq_all = d_chisq_all, a.ftol = ftol, a.fsteps = fsteps, a.S = n_starts, a.max_iter = max_iter;
    lfit::window_weights(a.wn);
    HIPCHK(c, launch_fit_loops(a, nch, c->stream));
    return MKID_OK;
}

// The CPU statement of the device call: the loops of loopfit_common.h.
int mkid_fit_loops_host(const double* freq, const double* i, const double* q, const double* isd, const double* qsd,
                        const double* draws, const double* qguess, int32_t nch, int32_t fsteps, int32_t n_starts,
                        int32_t max_iter, double ftol, mkid_loop_fit* fits, double* chisq_all) {
    if (!lfit::args_ok(freq, i, q, isd, qsd, draws, nch, fsteps, n_starts, max_iter, ftol, fits)) return MKID_E_ARG;
    lfit::fit_host(freq, i, q, isd, qsd, draws, qguess, nch, fsteps, n_starts, max_iter, ftol, fits, chisq_all);
    return MKID_OK;
}

// ---- resonator magnitude fits (magfit_common.h) ------------------------------------------------------
#define MAGS_ARGS_MSG \
    "need pointers, nch >= 1, 12 <= fsteps <= 1024, 1 <= n_starts <= 16, max_iter >= 1, ftol > 0"

int mkid_fit_mags(mkid_ctx* c, const double* d_freq, const double* d_i, const double* d_q, const double* d_draws,
                  int32_t nch, int32_t fsteps, int32_t n_starts, int32_t max_iter, double ftol, mkid_mag_fit* d_fits,
                  double* d_qout, double* d_chisq_all) {
    if (!c) return MKID_E_ARG;
    if (!mfit::args_ok(d_freq, d_i, d_q, d_draws, nch, fsteps, n_starts, max_iter, ftol, d_fits))
        FAIL(c, MKID_E_ARG, "fit_mags: " MAGS_ARGS_MSG);
    HIPCHK(c, hipSetDevice(c->device));
    MagfitArgs a{};
    a.freq = d_freq, a.i = d_i, a.q = d_q, a.draws = d_draws, a.fits = d_fits, a.qout = d_qout, a.chisq_all = d_chisq_all;
    a.ftol = ftol, a.fsteps = fsteps, a.S = n_starts, a.max_iter = max_iter;
    lfit::window_weights(a.wn);
    HIPCHK(c, launch_fit_mags(a, nch, c->stream));
    return MKID_OK;
}

// The CPU statement of the device call: the loops of magfit_common.h.
int mkid_fit_mags_host(const double* freq, const double* i, const double* q, const double* draws, int32_t nch,
                       int32_t fsteps, int32_t n_starts, int32_t max_iter, double ftol, mkid_mag_fit* fits, double* qout,
                       double* chisq_all) {
    if (!mfit::args_ok(freq, i, q, draws, nch, fsteps, n_starts, max_iter, ftol, fits)) return MKID_E_ARG;
    mfit::fit_host(freq, i, q, draws, nch, fsteps, n_starts, max_iter, ftol, fits, qout, chisq_all);
    return MKID_OK;
}

int mkid_stream_copy(mkid_ctx* c, void* d_dst, const void* d_src, int64_t bytes) {
    if (!c || !d_dst || !d_src || bytes < 0) return MKID_E_ARG;
    if (bytes % 16 != 0 || ((uintptr_t)d_dst & 15) != 0 || ((uintptr_t)d_src & 15) != 0)
        FAIL(c, MKID_E_ARG, "stream copy: 16-byte aligned pointers and sizes only");
    HIPCHK(c, hipSetDevice(c->device));
    KTime kt;
    tstart(c, MKID_K_COPY, &kt, c->stream);
    HIPCHK(c, launch_stream_copy(d_dst, d_src, bytes, c->stream));
    tstop(c, &kt, c->stream);
    return MKID_OK;
}
int mkid_synth_adc(mkid_ctx* c, int16_t* d_out, int64_t n, int64_t n0, const int16_t* d_base,
                   const mkid_synth_tone* d_tones, const mkid_pulse* d_pulses, int64_t npulses, float tr,
                   float tf, int32_t window, float sigma, uint32_t seed) {
    if (!c || !d_out || !d_base || n < 0 || (npulses > 0 && (!d_pulses || !d_tones))) return MKID_E_ARG;
    if (tr <= 0.f || tf <= 0.f || window < 0) FAIL(c, MKID_E_ARG, "bad pulse shape");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_synth(d_out, n, n0, d_base, d_tones, d_pulses, npulses, tr, tf, window, sigma, seed,
                           c->stream));
    return MKID_OK;
}

}  // extern "C"
