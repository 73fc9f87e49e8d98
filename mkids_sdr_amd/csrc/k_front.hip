// Fused front end for N = 128 / 256 (configs[0]'s 64-channel geometry; N >= 512 runs the
// wave-specialised k_front3 / k_front5, launch_fused below).
// K1-K6 in one pass over the ADC stream: polyphase filter bank + N-point FFT
// (2x oversampled, hop M = N/2) + bin select + DDC + 26-tap IQ low-pass decimating by 2 +
// IQ-centre subtraction + atan2 + Fix16_13. The complex baseband z never leaves the CU: HBM sees
// 4 B/sample of int16 I/Q in and 1 B/sample of raw phase (+2 B/sample float phase) out.
//
// A workgroup of BT = N/2 = C threads owns a contiguous run of frames [k_b, k_e) and walks it
// FPB = 4 frames per iteration (NT = N/8 threads per frame, 8 points per thread):
//   input  LDS ring of RS = 2T-1+FPB hops of M int16 I/Q samples; each iteration brings 4 new
//          hops with ONE 16-byte global load per thread, issued one iteration ahead.
//   PFB    u[p] = sum_tau h_q[tau N + p] x[(k+1)M - TN + tau N + p]: exact int16 dot products
//          (taps h_q = rint(h 2^S), mkid_set_pfb; the 2^-S rides in the LO table)
//   FFT    Stockham radix-8/4 passes through a padded per-frame LDS buffer (fft_common.h); the
//          last pass is fused into the select: thread c evaluates only the radix-4 butterfly
//          output X[bin_c] (4 LDS reads, 3 complex MACs with per-channel constant twiddles).
//   DDC    thread c = channel c: z_k = X_k[bin_c] (-1)^(bin_c (k+1)) conj(LUT_c[k mod P]) / 2^15
//          for the 4 frames of the iteration (LO table [P][C]: one contiguous row per frame; the
//          bin-parity sign is folded into the table on the host, P being even).
//   LPF    transposed form, 13 complex accumulators per thread: frame 2j adds g_{2m+1} z to
//          output j+m, frame 2j+1 adds g_{2m} z and completes output j:
//          y_j = sum_i g_i z_{2j+1-i}      (taps int(lpf*(2**11-1))/2^11, ROACH_Pulses.py:69,88)
//   phase  phi_j = atan2(Im y - qc, Re y - ic)     (pulse_triggering_IQ.py:152), accumulated
//          centred: y - c = sum_i g_i (z_i - c') + r  (mkid_internal.h Centring)
//          raw_j = fix16_13(phi_j): clamp(rint(phi_j 2^13), +-pi 2^13) (front_common.h)
// Each run starts kLpfHist = 24 frames early (warm-up: the low-pass history is recomputed from
// the ADC samples instead of being stored), so frames before the chunk come from an ADC history
// of (2T-1+24) hops carried between calls. Reference geometry: ROACH_Setup.py:507-550.
#include "front_common.h"

// a workgroup barrier, stamped before and after in the timing build (FRONT_STAMP; tools/stamps.py
// reads iterations 8..15 of the kernel's counter it_)
#define FSYNC(id)                            \
    do {                                     \
        FRONT_STAMP(it_, 8, 2 * (id));       \
        __syncthreads();                     \
        FRONT_STAMP(it_, 8, 2 * (id) + 1);   \
    } while (0)

// Streaming traffic is non-temporal: the ADC stream is read once and the phase rows are written
// once, so neither should evict the LO table (512 KB at 1024 channels, re-read by every
// workgroup every iteration) from L2. With default-policy streams the LO rows miss L2 on some
// boxes and their loads stall the select stage: same-box A/B -15 % k_front, -11 % k_trigger
// (profiles/r01/r01_v29_kbench_nt.json).

namespace mkid {

// Radix sequence: Plan8<N> (fft_common.h), three passes at N = 128 / 256. The last pass is not run
// through LDS: its radix-RL butterfly is evaluated only for the selected bin, by the channel's thread.
template <int N>
struct FGeo {
    using PL = Plan8<N>;
    static_assert(PL::NP == 3, "k_front runs the three-pass plans (N = 128 / 256)");
    static constexpr int PTS = 8, NT = N / PTS, FPB = 4;
    static constexpr int BT = NT * FPB;                 // == C: one channel per thread
    static constexpr int M = N / 2, C = N / 2, T = kPfbTaps;
    static constexpr int RS = 2 * T - 1 + FPB;          // ring slots (hops)
    // float2 per frame of the exchange buffer (Pad16 layout). A wave spans 4 (N = 128) or 2
    // (N = 256) frames, so this stride sets the banks its accesses fall on: it stays the one the
    // kernel was tuned and measured with (the size of an LPad<5, 4> layout, rounded up to even)
    static constexpr int LDSF = (LPad<5, 4>::size(N) + 1) & ~1;
    static_assert(LDSF >= Pad16::size(N), "frame buffer");
    static constexpr int SPT = FPB * M / BT;            // new samples per thread per iteration
    static_assert(SPT == 4, "one 16-byte load per thread per iteration");
    static_assert(BT == C, "one channel per thread");
    static constexpr int NS2 = PL::R[0], NS3 = NS2 * PL::R[1];
    static constexpr int RL = PL::R[2];                       // radix of the fused last pass
    static constexpr int NSL = N / RL;                        // its butterfly count / stride
    static_assert(NSL % 16 == 0, "pad-linear offsets in the fused last pass");
    using TW2 = TwiddleLds<N, PTS, PL::R[1], NS2>;
    static constexpr size_t tw_offset = (size_t)RS * M * 4 + (size_t)FPB * LDSF * 8 + (size_t)N * 8;
    // the pass-2 twiddle table; the NS3 float2 after it are not used (room a fourth pass's table
    // once took) and keep the launch's LDS footprint at the measured one
    static constexpr size_t lds_bytes = tw_offset + (size_t)(TW2::ENTRIES + NS3) * 8;
    static_assert(lds_bytes == (N == 128 ? 8832 : 17792), "LDS footprint of the measured kernels");
    // register budget sized for 4 waves per SIMD (16 per CU, <= 128 VGPRs): HIP's second
    // launch-bounds argument is the minimum waves per execution unit
    static constexpr int MINW = 4;
};

template <int N>
__global__ __launch_bounds__(FGeo<N>::BT, FGeo<N>::MINW) void k_front(FrontArgs a) {
    using G = FGeo<N>;
    using PL = typename G::PL;
    constexpr int PTS = G::PTS, NT = G::NT, M = G::M, C = G::C, T = G::T, RS = G::RS, FPB = G::FPB;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* ring = reinterpret_cast<uint32_t*>(smem);
    float2* fbuf = reinterpret_cast<float2*>(smem + (size_t)RS * M * 4);

    const int tid = threadIdx.x;
    // frame of the iteration this thread transforms: wave-uniform when a wave lies within one
    // frame (NT >= 64), so the ring-slot arithmetic below runs on the scalar unit
    const int slot = NT % 64 == 0 ? __builtin_amdgcn_readfirstlane(tid / NT) : tid / NT;
    const int t = tid % NT;
    float2* buf = fbuf + slot * G::LDSF;
    // PFB taps of point p as int16 pairs {h0|h1, h2|h3} in LDS (8 B per point): the PFB is an
    // exact int16 x int16 dot product per I/Q component (pfb_dot), the tap scale 2^-S
    // rides in the LO table
    uint2* hl = reinterpret_cast<uint2*>(smem + (size_t)RS * M * 4 + (size_t)FPB * G::LDSF * 8);
    static_assert(T == 4, "two int16 tap pairs per point");
    for (int p = tid; p < N; p += G::BT) hl[p] = a.pfbq[p];

    // pass-2 twiddle table in LDS (filled once; published by the prologue barrier)
    float2* twt = reinterpret_cast<float2*>(smem + G::tw_offset);
    typename G::TW2 tw2{twt};
    G::TW2::fill(twt, tid, G::BT);

    const int c = tid;  // channel of the select / low-pass / phase stage
    const int32_t bin = a.bins[c];
    const float2 ncen = a.cen.ncen[c], cor = a.cen.cor[c];   // centred low-pass (mkid_internal.h)
    // fused last pass for X[bin]: bin = jl + NSL s,
    //   X[bin] = sum_r W_RL^{r s} W_N^{jl r} Y[jl + r NSL]   (Stockham last pass, NS = NSL)
    constexpr int RL = G::RL, NSL = G::NSL;
    const int jl = bin % NSL, sl = bin / NSL;
    float2 tl[RL - 1];
#pragma unroll
    for (int r = 1; r < RL; ++r) {
        double sn, cs;
        sincospi(-2.0 * ((double)(jl * r) / N + (double)((r * sl) % RL) / RL), &sn, &cs);
        tl[r - 1] = make_float2((float)cs, (float)sn);
    }
    const int yoff = lpad(jl);

    const FrontRun run(a);
    if (run.empty()) return;
    const int64_t k_b = run.k_b, k_start = run.k_start;  // warm-up frames rebuild the low-pass history
    const int nrun = run.nrun;
    // outputs of this run: rows j = k_b/2 .. ; 32-bit offsets from per-run bases
    int16_t* const raw_run = a.raw + (k_b >> 1) * C;
    [[maybe_unused]] float* const phase_run = a.phase ? a.phase + (k_b >> 1) * C : nullptr;

    // prologue: hops k_start-2T+1 .. k_start+FPB-1 -> ring (slot = hop mod RS)
    {
        const int64_t h0 = k_start - 2 * T + 1;
        for (int g = 0; g < RS; g += FPB) {
            const int64_t hop = h0 + g + (tid * G::SPT) / M;
            if (hop > h0 + RS - 1) continue;
            const Hop<1> v = front_load<M, 1>(a, h0 + g, tid);
            *reinterpret_cast<uint4*>(ring + (int)(((hop % RS) + RS) % RS) * M + (tid * G::SPT) % M) = v.v[0];
        }
    }
    Hop<1> pre = front_load<M, 1>(a, k_start + FPB, tid);
    __syncthreads();

    // static issue priority by dispatch order (MI355X_MICROARCH.md "two waves per SIMD" item 4):
    // the later-dispatched waves of a SIMD lose every age-based arbitration and reach each barrier
    // last; raising them once before the loop trims that skew (-0.7..-1 % k_front, same-box A/B
    // profiles/r01/r01_v28_kbench_prio.json)
    {
        const int w = __builtin_amdgcn_readfirstlane(tid) / 64, nw = G::BT / 64;
        const int pr = nw >= 4 ? w * 4 / nw : 0;  // 0..3 by quarter of the workgroup
        if (pr == 1) __builtin_amdgcn_s_setprio(1);
        if (pr == 2) __builtin_amdgcn_s_setprio(2);
        if (pr == 3) __builtin_amdgcn_s_setprio(3);
    }
    uint64_t gp[13];
#pragma unroll
    for (int m = 0; m < 13; ++m) gp[m] = tap_pair(a.taps.g[2 * m], a.taps.g[2 * m + 1]);
    float2 acc[13];
#pragma unroll
    for (int m = 0; m < 13; ++m) acc[m] = make_float2(0.f, 0.f);
    float2 ys = make_float2(0.f, 0.f);

    // 32-bit stream counters, advanced by FPB per iteration (no 64-bit modulo in the loop):
    //   rb  = ring slot of hop kb + 1 - 2T (the oldest hop frame kb reads); the FPB hops loaded
    //         for the next iteration, kb + FPB + q = (kb + 1 - 2T) + RS + q, go to slot rb + q
    //   lrow = LO-table row of frame kb;  kr = kb - k_b (frame index relative to the run)
    int rb = (int)((((k_start + 1 - 2 * T) % RS) + RS) % RS);
    int lrow = (int)((a.k0 + k_start) & (int64_t)(a.P - 1));
    const int qh = (tid * G::SPT) / M, qoff = (tid * G::SPT) % M;  // this thread's ring write

#ifdef MKID_XP_STAMPS
    int it_ = 0;
#endif
    for (int kr = -kLpfHist; kr < nrun; kr += FPB) {
        const int64_t kb = k_b + kr;
#ifdef MKID_XP_STAMPS
        ++it_;
        FRONT_STAMP(it_, 8, 14);
#endif
        // LO rows of this iteration's frames (latency hidden behind the FFT)
        float2 lov[FPB];
#pragma unroll
        for (int f = 0; f < FPB; ++f) lov[f] = (a.lo + ((lrow + f) & (a.P - 1)) * C)[c];

        // ---- PFB of frame kb + slot from the LDS ring ----
        int sb = rb + slot;
        sb -= sb >= RS ? RS : 0;
        float2 v[PTS];
#pragma unroll
        for (int r = 0; r < PTS; ++r) {
            const int p = t + r * NT;
            const int hi = p / M, off = p % M;
            // one 8-byte LDS read (a uint2 load is split into two 4-byte halves)
            const uint64_t h64 = reinterpret_cast<const uint64_t*>(hl)[p];
            const uint2 hp = make_uint2((uint32_t)h64, (uint32_t)(h64 >> 32));
            uint32_t w[T];
#pragma unroll
            for (int tau = 0; tau < T; ++tau) {
                int sl = sb + 2 * tau + hi;
                sl -= sl >= RS ? RS : 0;  // sb + 2 tau + hi < 2 RS
                w[tau] = ring[sl * M + off];
            }
            v[r] = pfb_dot(hp, w);
            // keep the point order: stops the scheduler from hoisting all 32 ring loads at once
            // (register pressure) ...
            if ((r & 3) == 3)  // ... but let four points' loads overlap
                asm volatile("" : "+v"(v[r].x), "+v"(v[r].y), "+v"(v[r - 1].x), "+v"(v[r - 1].y),
                             "+v"(v[r - 2].x), "+v"(v[r - 2].y), "+v"(v[r - 3].x), "+v"(v[r - 3].y));
        }
        st_dft<PTS, PL::R[0]>(v);
        FSYNC(0);  // ring reads of this iteration and last iteration's select are done
        {
            int ws = rb + qh;
            ws -= ws >= RS ? RS : 0;
            *reinterpret_cast<uint4*>(ring + ws * M + qoff) = pre.v[0];
            pre = front_load<M, 1>(a, kb + 2 * FPB, tid);
            rb += FPB;
            rb -= rb >= RS ? RS : 0;
            lrow += FPB;
        }
        st_write<N, PTS, PL::R[0], 1>(buf, v, t);
        FSYNC(1);
        st_read<N, PTS, PL::R[1]>(buf, v, t);
        FSYNC(2);
        tw2.apply(v, t);
        st_dft<PTS, PL::R[1]>(v);
        st_write<N, PTS, PL::R[1], G::NS2>(buf, v, t);
        FSYNC(6);

        // ---- select + DDC + low-pass + phase for channel c over the FPB frames ----
#pragma unroll
        for (int f = 0; f < FPB; ++f) {
            const int kf = kr + f;  // frame kb + f relative to k_b
            const float2* yf = fbuf + f * G::LDSF + yoff;
            float2 X = yf[0];
#pragma unroll
            for (int r = 1; r < RL; ++r) X = cmac(X, tl[r - 1], yf[r * NSL / 16 * 17]);
            const float2 z = cmul_add_pk(X, lov[f], ncen);   // z - c'
#ifdef MKID_XP_STAMPS
            if (f == 0) {
                asm volatile("" ::"v"(z.x), "v"(z.y));
                FRONT_STAMP(it_, 8, 12);  // frame 0 selected (its LDS reads and LO load have landed)
            }
            if (f == 2) FRONT_STAMP(it_, 8, 13);  // output 0 written
#endif
            if ((f & 1) == 0) {  // frame 2j: taps 1,3,..,25 into outputs j..j+12
                lpf_even(gp, z, acc);
            } else {  // frame 2j+1: taps 0,2,..,24; output j complete
                const float2 y = lpf_odd(gp, z, acc);
                if (kf > 0 && kf < nrun) {
                    const int jr = (kf - 1) >> 1;  // row within the run
                    ys.x += y.x;
                    ys.y += y.y;
                    const float ph = phase_atan2(y.y + cor.y, y.x + cor.x);
#ifndef MKID_XP_STAMPS
                    if (phase_run) __builtin_nontemporal_store(ph, phase_run + jr * C + c);
#endif
                    __builtin_nontemporal_store(fix16_13(ph), raw_run + jr * C + c);
                    if (c == a.iq_ch && a.iqtap)
                        *reinterpret_cast<uint32_t*>(a.iqtap + 2 * ((k_b >> 1) + jr)) = iq_tap_word(a.cen, y);
                }
            }
        }
    }
    if (a.ysum) {
        ysum_add(a.ysum, c, ys.x, ys.y);
    }
}

bool fused_supported(int N) { return N == 128 || N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096; }

int64_t front_hist_samples(int N) { return front_hist(N / 2); }

template <int N>
static hipError_t launch_front(const FrontArgs& a0, hipStream_t s) {
    using G = FGeo<N>;
    static std::atomic<uint64_t> attr_mask{0};
    hipError_t e = ensure_lds_attr(attr_mask, (const void*)k_front<N>, (int)G::lds_bytes);
    if (e != hipSuccess) return e;
    FrontArgs a = a0;
    if (a.K <= 0) return hipSuccess;
    // frame runs: long enough to amortise the 24-frame warm-up, enough of them to fill the CUs
    const int64_t blocks = front_grid(a, 1024, 1024, G::FPB);
    hipLaunchKernelGGL(k_front<N>, dim3((unsigned)blocks), dim3(G::BT), G::lds_bytes, s, a);
    return hipGetLastError();
}

// the fused front end of each FFT length: k_front (this file) at N = 128 / 256, the
// wave-specialised k_front3 at 512 / 1024 / 2048 and k_front5 at 4096
hipError_t launch_fused(int N, const FrontArgs& a, hipStream_t s) {
    switch (N) {
        case 128: return launch_front<128>(a, s);
        case 256: return launch_front<256>(a, s);
        case 512: return launch_front3<512>(a, s);
        case 1024: return launch_front3<1024>(a, s);
        case 2048: return launch_front3<2048>(a, s);
        case 4096: return launch_front5(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mkid
