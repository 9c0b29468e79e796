// trk_persist.hip — the closed DLL/PLL loop with one workgroup per channel for a whole run.
//
// dll_pll_veml_tracking::general_work (dll_pll_veml_tracking.cc:1728-2094) runs one epoch per call:
// do_correlation_step (:1037-1062) → Cpu_Multicorrelator_Real_Codes (cpu_multicorrelator_real_codes.cc:
// 103-126) → the loop update (trk_loop.h).  Epoch k+1's NCO depends on epoch k's correlations, so a
// channel is a strictly serial chain of epochs, while channels are independent.  This kernel gives
// every channel its own 256-thread workgroup that runs ALL of the channel's epochs in the IF buffer
// inside one launch: no kernel boundary, no host round trip and no grid-wide synchronisation
// between epochs.  Per epoch:
//   1. thread 0 derives the correlator arguments from the channel state (do_correlation_step);
//   2. the epoch is correlated in the reference's own order of operations, per rotator variant (below): every
//      sum is formed in the same order on every run (the results are bit-reproducible, independent of wave
//      scheduling and of the other channels in the launch) and equals the reference's bit for bit;
//   3. thread 0 runs the loop update on the channel state, which lives in LDS for the whole run, and
//      writes the epoch's record.
//
// Rotator variants (include/gnsship.h GNSSHIP_ROTATOR_*):
//  * generic (volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn.h:66-98): one phasor, N dependent
//    products per epoch, renormalised every 256 samples, and ONE serial float sum per tap component
//    (result[t] += (x·phase)·a_t[n], n = 0..N−1).  Reproduced bit for bit as a three-stage pipeline
//    through LDS rings of 64-sample chunks: wave 0's lane 0 replays the phasor chain and stores the
//    phase of every sample; waves 1-2 (alternate chunks, one lane per sample) form x·phase and its
//    products with every tap's chip; wave 3's lane j < 2·taps (+2 for the data prompt) adds tap
//    component j's products serially in sample order — the reference's own float sum.
//  * AVX (…:155-316, what volk_gnsssdr dispatches on AVX hosts): 16 phasors z_l advanced by
//    dz = normalise(inc^16), renormalised every 64 iterations, sixteen accumulators per tap.  Sixteen lanes
//    of one wave ARE those sixteen chains, serial sums and all (chains_avx): one dependent chain of N/16
//    iterations per epoch, the reference's own single-core latency.  This is the fallback behind trk_fast.hip
//    and trk_lane.hip (GNSSHIP_TRK_FAST=0, codes that are not ±1, no trk_fast plan).  An earlier form cut the
//    epoch into tasks spread over three waves and summed them as a tree: faster, and one ulp off the
//    reference's taps in every epoch; it was removed when every engine was held to bit equality, and what
//    the chains cost against it has not been measured.
//
// High-dynamics tracking and epochs too long for LDS stay on the round-based path (trk_kernel.hip).
#include <cstdlib>

#include "corr_device.h"
#include "serial_rotator.h"
#include "trk_engine.h"

// Epoch phase timestamps for the profiling build only (make prof → scripts/libgnsship_prof.so,
// scripts/trk_wg_profile.py): slot [(channel·kProfEpochs + epoch)·16 + k] = wall_clock64() at phase
// k (0-6 and 16-21 in the kernel, 8-12 inside the loop update — trk_loop.h GNSSHIP_TRK_LOOP_STAMP —
// 13-15 and 7 unused).
#ifdef GNSSHIP_CORR_PROFILE
namespace gnsship {
constexpr int kProfEpochs = 64;
constexpr int kProfSlots = 32;
__device__ unsigned long long* g_trk_prof = nullptr;
__shared__ int g_prof_epoch;
__device__ __forceinline__ void trk_prof_stamp(int e, int k)
{
    if (g_trk_prof && e < kProfEpochs) g_trk_prof[(static_cast<size_t>(blockIdx.x) * kProfEpochs + e) * kProfSlots + k] = wall_clock64();
}
}  // namespace gnsship
#define GNSSHIP_TRK_STAMP(e, k) gnsship::trk_prof_stamp((e), (k))
#define GNSSHIP_TRK_LOOP_STAMP(k) gnsship::trk_prof_stamp(gnsship::g_prof_epoch, (k))
#else
#define GNSSHIP_TRK_STAMP(e, k) \
    do {                        \
    } while (0)
#endif

#include "trk_loop.h"
#include "trk_glo_loop.h"

#pragma clang fp contract(off)

namespace gnsship {
namespace {

constexpr int kPThreads = 256;
constexpr int kPWaves = kPThreads / kWave;
constexpr int kAvxSeg = 64;    // the AVX rotator's renormalisation period in 16-sample iterations (:265-272)

// The epoch being correlated (LDS): the reference's call arguments as a DevJob plus the AVX step.
struct PEpoch {
    DevJob job;
    float dz_re, dz_im;  // normalise(inc^16) (AVX)
    int32_t runnable;
    int32_t in_margin;   // every chip index of the epoch lies in the padded LDS replica
    SerialSync sync;     // generic: the serial pipeline's ring counters
    int32_t locked;      // lock_status outcome (wave 1) for the loop update (wave 0)
    double coh;          // epoch_pre's coherent integration time (0: no lock test this epoch)
    float trace_rem_carr, trace_step;  // the carrier arguments as passed (IF folded in)
    float taps[2 * kMaxTaps + 2];  // the epoch's tap sums (+ the data prompt), as epoch_update reads them
    gnsship_trk_epoch rec;
    gnsship_trk_dump_record dump;
};

// ---- the generic rotator: serial pipeline (serial_rotator.h) ---------------------------------------
// Ring of RC chunks in the dynamic LDS after the codes: phases, then 2·(taps + data prompt) product
// rows per chunk.  The accumulator's lane j stores component j where the loop update reads it.
template <int FMT, int NT, bool DATA>
__device__ void serial_epoch(PEpoch& ep, float* anc, int RC, i4v span, int N, const float* c0, const float* c1, int L, int lane, int wave)
{
    constexpr int TM = NT + (DATA ? 1 : 0);
    SerialSync& sy = ep.sync;
    f2* Zr = reinterpret_cast<f2*>(anc);
    float* P = anc + 2 * kSChunk * RC;
    if (wave == 0) {
        if (lane == 0) serial_replay(sy, Zr, RC, N, f2{ep.job.p0_re, ep.job.p0_im}, f2{ep.job.inc_re, ep.job.inc_im});
    } else if (wave < kPWaves - 1) {
        const float* code[TM];
        float shift[TM];
#pragma unroll
        for (int t = 0; t < TM; t++) {
            code[t] = t < NT ? c0 : c1;
            shift[t] = t < NT ? ep.job.shifts[t] : 0.0f;
        }
        if (ep.in_margin)
            serial_produce<FMT, TM, true>(sy, Zr, P, RC, span, N, TM, code, shift, L, ep.job.code_step, ep.job.rem_code, lane, wave - 1);
        else
            serial_produce<FMT, TM, false>(sy, Zr, P, RC, span, N, TM, code, shift, L, ep.job.code_step, ep.job.rem_code, lane, wave - 1);
    } else {
        const float acc = serial_accumulate(sy, P, RC, N, TM, lane);
        // the taps' components, then the data prompt at 2·kMaxTaps (the other entries were zeroed)
        if (lane < 2 * TM) ep.taps[lane < 2 * NT ? lane : 2 * kMaxTaps + lane - 2 * NT] = acc;
    }
}

// ---- correlation (AVX, u_avx's own accumulation order) -------------------------------------------
// The sixteen lanes of one wave ARE u_avx's sixteen chains (trk_lane.hip's scheme with float replicas).  Lane l
// starts at phase·inc^l, takes the samples 16m + l, forms a = x·z_l (_mm256_complexmul_ps rounding), advances
// z_l·dz (renormalised after iteration m ≡ 0 mod 64, :266-272) and adds a·code to its own accumulators
// in iteration order (_mm256_mul_ps, _mm256_add_ps, :252-260); the chains combine as :279-291, the
// N mod 16 tail runs on lane 0 (:294-308).  One dependent chain of N/16 iterations per epoch: the
// reference's own single-core latency — this engine is the fallback behind trk_fast and trk_lane.

// ((d_k + d_{k+4}) + d_{k+8}) + d_{k+12} for k = 0..3, then (((0 + s_0) + s_1) + s_2) + s_3, valid at
// lane 0 of the 16-lane row (as trk_lane.hip's avx_chain_sum_row)
__device__ __forceinline__ float chain_sum_row(float d)
{
    float s = d + dpp_mov<0x12C>(d);  // row_ror:12 — lane k reads lane k + 4
    s = s + dpp_mov<0x128>(d);        // row_ror:8  — lane k + 8
    s = s + dpp_mov<0x124>(d);        // row_ror:4  — lane k + 12
    float r = 0.0f + s;
    r = r + dpp_mov<0x101>(s);  // row_shl:1 — lane 0 reads lane 1
    r = r + dpp_mov<0x102>(s);  // row_shl:2
    r = r + dpp_mov<0x103>(s);  // row_shl:3
    return r;
}

__device__ __forceinline__ f2 mul_add(f2 acc, f2 a, float c)  // acc + fl(a·c), no fusion
{
    return f2{__fadd_rn(acc.x, __fmul_rn(a.x, c)), __fadd_rn(acc.y, __fmul_rn(a.y, c))};
}

// Lanes 0..15 of one wave (l = lane); the tap sums land in ep.taps as the loop update reads them.
template <int FMT, int NT, bool DATA, bool IN_MARGIN>
__device__ void chains_avx(PEpoch& ep, i4v span, int N, const float* code0, const float* code1, int L, int l)
{
    constexpr int SB = sample_bytes<FMT>();
    constexpr int NTT = NT + (DATA ? 1 : 0);
    constexpr int kB = 8;  // iterations whose samples are loaded together
    const DevJob& job = ep.job;
    const int M = N / kAvxLanes, tail = N - kAvxLanes * M;
    const f2 inc = f2{job.inc_re, job.inc_im}, dz = f2{ep.dz_re, ep.dz_im};
    const float step = job.code_step, rem = job.rem_code;
    float shifts[NTT];
#pragma unroll
    for (int t = 0; t < NTT; t++) shifts[t] = t < NT ? job.shifts[t] : 0.0f;
    f2 z = f2{job.p0_re, job.p0_im};  // phase_vec[l] = phase·inc^l (:204-208)
    for (int i = 0; i < kAvxLanes - 1; i++)
        if (i < l) z = cmul_exact(z, inc);
    f2 acc[NTT];
#pragma unroll
    for (int t = 0; t < NTT; t++) acc[t] = f2{0.0f, 0.0f};
    for (int m0 = 0; m0 < M; m0 += kB) {
        f2 x[kB];
#pragma unroll
        for (int u = 0; u < kB; u++) x[u] = m0 + u < M ? load_sample<FMT>(span, (kAvxLanes * (m0 + u) + l) * SB, 0) : f2{0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < kB; u++) {
            const int m = m0 + u;
            if (m >= M) break;
            const f2 a = cmul_exact_pk(x[u], z);
            z = cmul_exact_pk(z, dz);
            if ((m & (kAvxSeg - 1)) == 0) z = normalise_avx(z);
            const float sn = __fmul_rn(step, static_cast<float>(kAvxLanes * m + l));
#pragma unroll
            for (int t = 0; t < NTT; t++) acc[t] = mul_add(acc[t], a, code_at<IN_MARGIN>(t < NT ? code0 : code1, L, sn, shifts[t], rem));
        }
    }
#pragma unroll
    for (int t = 0; t < NTT; t++) acc[t] = f2{chain_sum_row(acc[t].x), chain_sum_row(acc[t].y)};
    if (l != 0) return;
    f2 ph = normalise_avx(z);  // _phase = normalise(z_0), then sample by sample
    for (int q = 0; q < tail; q++) {
        const int n = kAvxLanes * M + q;
        const f2 wo = cmul_exact(load_sample<FMT>(span, n * SB, 0), ph);
        ph = cmul_exact(ph, inc);
        const float sn = __fmul_rn(step, static_cast<float>(n));
#pragma unroll
        for (int t = 0; t < NTT; t++) acc[t] = mul_add(acc[t], wo, code_at<false>(t < NT ? code0 : code1, L, sn, shifts[t], rem));
    }
    for (int i = 0; i < 2 * kMaxTaps + 2; i++) ep.taps[i] = 0.0f;
#pragma unroll
    for (int t = 0; t < NTT; t++) {
        const int o = (DATA && t == NT) ? 2 * kMaxTaps : 2 * t;
        ep.taps[o] = acc[t].x;
        ep.taps[o + 1] = acc[t].y;
    }
}

// do_correlation_step's arguments for the epoch at c.nitems_read (derive_job on the device; the
// generic lane factor needs arg/|inc| in double, the AVX path needs dz instead).
// p0 / inc: (cos rem, −sin rem) and (cos −step, sin −step), evaluated by two lanes of wave 0 at once.
template <bool AVX>
__device__ void derive_epoch(PEpoch& ep, const TrkParams& k, const TrkChannel& c, int64_t off, int L, f2 p0, f2 inc, int32_t n_samples)
{
    const int NT = k.n_taps;
    const float* sh = c.narrow ? k.shifts_n : k.shifts;
    DevJob& j = ep.job;
    const float spcf = static_cast<float>(k.code_samples_per_chip);
    j.sample_offset = off;
    j.n_samples = n_samples;
    j.code_id = c.code_id;
    j.n_taps = NT;
    j.rot_avx = 0;  // (the batch path's flag: this kernel has its own replays)
    j.p0_re = p0.x;
    j.p0_im = p0.y;
    j.inc_re = inc.x;
    j.inc_im = inc.y;
    j.rem_code = __fmul_rn(static_cast<float>(c.rem_code_phase_chips), spcf);
    j.code_step = __fmul_rn(static_cast<float>(c.code_phase_step_chips), spcf);
    for (int t = 0; t < kMaxTaps; t++) j.shifts[t] = t < NT ? sh[t] : 0.0f;
    if constexpr (AVX) {
        f2 d = f2{j.inc_re, j.inc_im};
        for (int q = 0; q < 4; q++) d = cmul_exact(d, d);  // dz *= dz four times (:221-225)
        d = normalise_avx(d);
        ep.dz_re = d.x;
        ep.dz_im = d.y;
    }
    // chip-index range (monotone in n): inside the padded replica the modulo is skipped (the data
    // prompt's shift 0 lies inside the taps' range)
    float smin = 0.0f, smax = 0.0f;
    for (int t = 0; t < NT; t++) {
        smin = fminf(smin, j.shifts[t]);
        smax = fmaxf(smax, j.shifts[t]);
    }
    const double span = static_cast<double>(j.code_step) * static_cast<double>(j.n_samples > 0 ? j.n_samples - 1 : 0);
    const double lo = fmin(0.0, span) + smin - j.rem_code - 2.0;
    const double hi = fmax(0.0, span) + smax - j.rem_code + 2.0;
    ep.in_margin = (isfinite(lo) && isfinite(hi) && lo >= -kCodeMargin && hi < static_cast<double>(L + kCodeMargin)) ? 1 : 0;
}

// Stage a padded code replica (engine.h padded_code_quads) in LDS.
__device__ void stage_code(float* dst, const CodeDesc& cd)
{
    const int nq = padded_code_quads(cd.len);
    const float4* src = reinterpret_cast<const float4*>(cd.ptr - kCodeMargin);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int q = threadIdx.x; q < nq; q += kPThreads) d4[q] = src[q];
}

// THRU: the throughput variant for more channels than CUs — ≤ 128 VGPRs (4 workgroups per CU) and
// a 4-deep sample prefetch; otherwise one workgroup per CU may use every register for a 16-deep one.
template <bool THRU>
constexpr int persist_waves_per_simd() { return THRU ? 4 : 1; }

// GLO: the GLONASS L1 / L2 C/A block (trk_glo_loop.h) on the generic serial pipeline — the epoch is correlated over the
// channel's current block length (not vector_length) and thread 0 runs glo_epoch_update in place of the five phases.
// Every GLO branch is `if constexpr`: the other instantiations compile to what they were.
template <int FMT, int NT, bool DATA, bool AVX, bool THRU, bool GLO = false>
__global__ __launch_bounds__(kPThreads, persist_waves_per_simd<THRU>()) void trk_persist_kernel(const TrkParams* __restrict__ pk, TrkChannel* __restrict__ chans,
    const CodeDesc* __restrict__ codes, int n_codes, const void* __restrict__ samples, uint64_t buf_first, int64_t buf_len, int max_rounds,
    int n_chans, int code_cap_floats, int ring_chunks, gnsship_trk_epoch* __restrict__ rec, gnsship_trk_dump_record* __restrict__ dump,
    gnsship_trk_corr_trace* __restrict__ trace, int* __restrict__ ran_count)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ TrkChannel sc;
    __shared__ PEpoch ep;
    __shared__ int32_t skip;
    const int ch = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TrkParams& k = *pk;
    {
        const int* src = reinterpret_cast<const int*>(chans + ch);
        int* dst = reinterpret_cast<int*>(&sc);
        for (int i = tid; i < static_cast<int>(sizeof(TrkChannel) / 4); i += kPThreads) dst[i] = src[i];
    }
    __syncthreads();
    if (tid == 0) {
        const bool tracking = sc.state == 2 || sc.state == 3 || sc.state == 4;
        const bool codes_ok = sc.code_id >= 0 && sc.code_id < n_codes && codes[sc.code_id].ptr && codes[sc.code_id].len > 0 &&
                              padded_code_quads(codes[sc.code_id].len) * 4 <= code_cap_floats &&
                              (!DATA || (sc.data_code_id >= 0 && sc.data_code_id < n_codes && codes[sc.data_code_id].ptr &&
                                            codes[sc.data_code_id].len == codes[sc.code_id].len));
        skip = (tracking && codes_ok) ? 0 : 1;
    }
    __syncthreads();
    if (skip) return;  // idle channel: its state is untouched
    float* code0 = lds;
    float* code1 = lds + code_cap_floats;
    float* anc = lds + (DATA ? 2 : 1) * code_cap_floats;
    stage_code(code0, codes[sc.code_id]);
    if constexpr (DATA) stage_code(code1, codes[sc.data_code_id]);
    const int L = codes[sc.code_id].len;
    const float* c0 = code0 + kCodeMargin;
    const float* c1 = code1 + kCodeMargin;
    const int N = static_cast<int>(k.conf.vector_length);
    for (int e = 0; e < max_rounds; e++) {
        if (wave == 0) {
            if (lane == 0) GNSSHIP_TRK_STAMP(e, 0);
#ifdef GNSSHIP_CORR_PROFILE
            if (lane == 0) g_prof_epoch = e;
#endif
            // the epoch's two phasors (cpu_multicorrelator_real_codes.cc:115,123), lane 0: rem_carr,
            // lane 1: −step, each glibc's cosf / sinf (glibc_sincosf.h)
            const float a = lane == 0 ? corr_rem_carr(k, sc) : -corr_phase_step(k, sc);
            if (lane == 0) {
                ep.trace_rem_carr = corr_rem_carr(k, sc);
                ep.trace_step = corr_phase_step(k, sc);
            }
            float sf, cf;
            glibc_sincosf(a, &sf, &cf);
            const f2 p0 = f2{__shfl(cf, 0, kWave), -__shfl(sf, 0, kWave)};
            const f2 inc = f2{__shfl(cf, 1, kWave), __shfl(sf, 1, kWave)};
            if (lane == 0) {
                const uint64_t vl = GLO ? static_cast<uint64_t>(sc.current_prn_length_samples > 0 ? sc.current_prn_length_samples : 0) : k.conf.vector_length;
                const bool runnable = (sc.state == 2 || sc.state == 3 || sc.state == 4) && sc.nitems_read >= buf_first &&
                                      sc.nitems_read + vl <= buf_first + static_cast<uint64_t>(buf_len) && (!GLO || vl > 0);
                ep.runnable = runnable ? 1 : 0;
                if (runnable) {
                    derive_epoch<AVX>(ep, k, sc, static_cast<int64_t>(sc.nitems_read - buf_first), L, p0, inc, static_cast<int32_t>(vl));
                    sc.epoch_start = sc.nitems_read;
                }
                ep.sync = SerialSync{};
                if constexpr (!AVX)
                    for (int i = 0; i < 2 * kMaxTaps + 2; i++) ep.taps[i] = 0.0f;
                GNSSHIP_TRK_STAMP(e, 1);
            }
        }
        __syncthreads();  // also: the code replicas are staged (first epoch)
        if (!ep.runnable) break;
        // the epoch's first sample as a wave-uniform value: read from LDS it is per-lane, and a per-lane
        // buffer resource turns every sample load into a waterfall loop
        const uint64_t off64 = static_cast<uint64_t>(ep.job.sample_offset);
        const int64_t off_u = static_cast<int64_t>((static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(off64 >> 32)))) << 32) |
                                                   static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(off64 & 0xffffffffu))));
        // the epoch's length: vector_length, or (GLO) the block length the previous epoch left, wave-uniform
        const int Ne = GLO ? __builtin_amdgcn_readfirstlane(ep.job.n_samples) : N;
        const i4v span = sample_span<FMT>(samples, off_u, Ne);
        if constexpr (AVX) {
            if (wave == 1 && lane < kAvxLanes) {
                if (ep.in_margin) chains_avx<FMT, NT, DATA, true>(ep, span, N, c0, c1, L, lane);
                else chains_avx<FMT, NT, DATA, false>(ep, span, N, c0, c1, L, lane);
            }
            if (tid == 0) GNSSHIP_TRK_STAMP(e, 2);
        } else {
            serial_epoch<FMT, NT, DATA>(ep, anc, ring_chunks, span, Ne, c0, c1, L, lane, wave);
            if (tid == 0) GNSSHIP_TRK_STAMP(e, 2);
        }
        if (lane == 0) GNSSHIP_TRK_STAMP(e, wave <= 1 ? 3 + wave : 14 + wave);  // waves 2, 3: slots 16, 17
        __syncthreads();
        const float* taps = ep.taps;
        const float* pdata = DATA ? ep.taps + 2 * kMaxTaps : ep.taps;
        gnsship_trk_dump_record* dr = dump ? &ep.dump : nullptr;
        if (tid == 0) {
            GNSSHIP_TRK_STAMP(e, 5);
            ep.rec = gnsship_trk_epoch{};
            ep.rec.flags = 8;
            if constexpr (GLO) {
                ep.coh = 0.0;  // no phases: the block's whole epoch, record and consume_each included
                glo_epoch_update(k, sc, taps, ep.rec, dr);
            } else {
                ep.coh = epoch_pre(k, sc, taps, pdata, ep.rec, nullptr, dr);
            }
        }
        __syncthreads();
        // the lock detectors (wave 1) beside the loop filters and NCO update (wave 0), which run
        // speculatively on a register copy of their members, stored only when the lock test passes
        // (trk_loop.h epoch phases)
        const double coh = ep.coh;
        LoopRegs lr;
        if (coh > 0.0) {
            if (tid == kWave) {
                GNSSHIP_TRK_LOOP_STAMP(8);
                ep.locked = lock_status(k, sc, coh) ? 1 : 0;
            } else if (tid == 0) {
                load_regs(k, sc, lr);
                epoch_loop(k, lr, nullptr);
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (coh > 0.0) {
                const bool locked = ep.locked != 0;
                if (locked) store_regs(lr, sc);
                epoch_post(k, sc, taps, pdata, ep.rec, locked, dr);
            }
            if constexpr (!GLO) epoch_finish(k, sc, ep.rec);
            const size_t slot = static_cast<size_t>(e) * n_chans + ch;
            if (rec) rec[slot] = ep.rec;
            if (dump && (ep.rec.flags & 16)) dump[slot] = ep.dump;
            if (trace) {
                gnsship_trk_corr_trace tr{};
                tr.sample_counter = sc.epoch_start;
                tr.n_samples = Ne;
                tr.n_taps = NT;
                tr.rem_carrier_phase_rad = ep.trace_rem_carr;
                tr.phase_step_rad = ep.trace_step;
                tr.rem_code_phase_samples = ep.job.rem_code;
                tr.code_phase_step_samples = ep.job.code_step;
                for (int t = 0; t < 5; t++) tr.shifts[t] = ep.job.shifts[t];
                for (int t = 0; t < 10; t++) tr.taps[t] = t < 2 * NT ? taps[t] : 0.0f;
                tr.data_prompt[0] = DATA ? pdata[0] : 0.0f;
                tr.data_prompt[1] = DATA ? pdata[1] : 0.0f;
                trace[slot] = tr;
            }
            atomicAdd(ran_count + e, 1);
            GNSSHIP_TRK_STAMP(e, 6);
        }
        __syncthreads();
    }
    if (tid == 0) sc.ran = 0;
    __syncthreads();
    {
        const int* src = reinterpret_cast<const int*>(&sc);
        int* dst = reinterpret_cast<int*>(chans + ch);
        for (int i = tid; i < static_cast<int>(sizeof(TrkChannel) / 4); i += kPThreads) dst[i] = src[i];
    }
}

}  // namespace

#ifdef GNSSHIP_CORR_PROFILE
}  // namespace gnsship
extern "C" int gnsship_debug_trk_profile(void* dev_buf)
{
    return hipMemcpyToSymbol(HIP_SYMBOL(gnsship::g_trk_prof), &dev_buf, sizeof(void*)) == hipSuccess ? 0 : -3;
}
namespace gnsship {
#endif

// LDS bytes of the persistent kernel's dynamic region: the code replica(s) and, for the generic rotator, the serial
// pipeline's rings — 16 chunks where they fit, else 8 or 4 (g_out = RC).  The AVX form (chains_avx) keeps its
// chains in registers: the replicas alone.
static size_t persist_lds(const TrkParams& p, int code_cap_floats, bool avx, int* g_out)
{
    const size_t codes = static_cast<size_t>(p.jobs_per_channel > 1 ? 2 : 1) * code_cap_floats * sizeof(float);
    if (g_out) *g_out = 0;
    if (avx) return codes;
    const int na = 2 * (p.n_taps + (p.jobs_per_channel > 1 ? 1 : 0));
    size_t bytes = 0;
    for (int rc = 16; rc >= 4; rc /= 2) {
        bytes = codes + serial_ring_bytes(rc, na);
        if (g_out) *g_out = rc;
        if (bytes <= kTrkPersistMaxLds) break;
    }
    return bytes;
}

size_t trk_persist_lds_bytes(const TrkParams& p, int code_cap_floats, bool avx) { return persist_lds(p, code_cap_floats, avx, nullptr); }

hipError_t launch_trk_persist(const TrkRun& r, bool avx, gnsship_trk_plan* plan)
{
    int ring_chunks = 0;  // the generic rotator's ring (0 for the AVX form)
    const size_t lds = persist_lds(r.params, r.code_cap_floats, avx, &ring_chunks);
    const bool data = r.params.jobs_per_channel > 1;
    const bool glo = r.params.conf.system == GNSSHIP_SYS_GLO_L1CA || r.params.conf.system == GNSSHIP_SYS_GLO_L2CA;
    if (glo && (avx || data || r.params.n_taps != 3)) return hipErrorInvalidValue;
    // more channels than CUs: the throughput variant (GNSSHIP_TRK_THRU=0/1 overrides, for A/B runs)
    bool thru = r.n_chans > 256;
    if (const char* env = std::getenv("GNSSHIP_TRK_THRU")) thru = env[0] == '1';
    const int nt = r.params.n_taps;
    dim3 grid(r.n_chans), block(kPThreads);
#define GNSSHIP_PERSIST(F, NTV, DV, AV)                                                                                                  \
    do {                                                                                                                                       \
        auto kfn = thru ? trk_persist_kernel<F, NTV, DV, AV, true> : trk_persist_kernel<F, NTV, DV, AV, false>;                             \
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)); \
        if (e0 != hipSuccess) return e0;                                                                                                       \
        hipLaunchKernelGGL(kfn, grid, block, lds, r.stream, r.params_dev, r.chans, r.codes, r.n_codes, r.samples, r.buf_first, r.buf_len,      \
            r.max_rounds, r.n_chans, r.code_cap_floats, ring_chunks, r.rec, r.dump, r.trace, r.ran_count);                                     \
    } while (0)
#define GNSSHIP_PERSIST_GLO(F)                                                                                                                \
    do {                                                                                                                                      \
        auto kfn = thru ? trk_persist_kernel<F, 3, false, false, true, true> : trk_persist_kernel<F, 3, false, false, false, true>;               \
        hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)); \
        if (e0 != hipSuccess) return e0;                                                                                                      \
        hipLaunchKernelGGL(kfn, grid, block, lds, r.stream, r.params_dev, r.chans, r.codes, r.n_codes, r.samples, r.buf_first, r.buf_len,     \
            r.max_rounds, r.n_chans, r.code_cap_floats, ring_chunks, r.rec, r.dump, r.trace, r.ran_count);                                    \
    } while (0)
#define GNSSHIP_PERSIST_F(F)                                                      \
    do {                                                                          \
        if (glo) {                                                                \
            GNSSHIP_PERSIST_GLO(F);                                               \
        } else if (nt == 3 && !data) {                                            \
            if (avx) GNSSHIP_PERSIST(F, 3, false, true);                          \
            else GNSSHIP_PERSIST(F, 3, false, false);                             \
        } else if (nt == 3 && data) { /* GPS L5: pilot taps + the L5I prompt */    \
            if (avx) GNSSHIP_PERSIST(F, 3, true, true);                           \
            else GNSSHIP_PERSIST(F, 3, true, false);                              \
        } else if (nt == 5 && !data) {                                            \
            if (avx) GNSSHIP_PERSIST(F, 5, false, true);                          \
            else GNSSHIP_PERSIST(F, 5, false, false);                             \
        } else if (nt == 5 && data) {                                             \
            if (avx) GNSSHIP_PERSIST(F, 5, true, true);                           \
            else GNSSHIP_PERSIST(F, 5, true, false);                              \
        } else {                                                                  \
            return hipErrorInvalidValue;                                          \
        }                                                                         \
    } while (0)
    switch (r.fmt) {
    case GNSSHIP_FMT_CF32: GNSSHIP_PERSIST_F(GNSSHIP_FMT_CF32); break;
    case GNSSHIP_FMT_CI16: GNSSHIP_PERSIST_F(GNSSHIP_FMT_CI16); break;
    case GNSSHIP_FMT_CI8: GNSSHIP_PERSIST_F(GNSSHIP_FMT_CI8); break;
    default: return hipErrorInvalidValue;
    }
#undef GNSSHIP_PERSIST_F
#undef GNSSHIP_PERSIST_GLO
#undef GNSSHIP_PERSIST
    *plan = gnsship_trk_plan{};
    plan->engine = GNSSHIP_TRK_ENGINE_PERSIST;
    plan->format = r.fmt;
    plan->n_taps = nt;
    plan->data_prompt = data ? 1 : 0;
    plan->lds_bytes = static_cast<int32_t>(lds);
    plan->thru = thru ? 1 : 0;
    plan->avx = avx ? 1 : 0;
    return hipGetLastError();
}

}  // namespace gnsship
