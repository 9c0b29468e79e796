// cond_xlating_fir.hip — the signal conditioner's input filter for gfx950: a streaming, stateful,
// multi-band frequency-translating FIR decimator.
//
// Replaces the InputFilter of the flowgraph's Signal_Conditioner (gnss_flowgraph.cc:1008-1140) in its
// Freq_Xlating_Fir_Filter form (src/algorithms/input_filter/adapters/freq_xlating_fir_filter.cc:36-117:
// properties IF, sampling_frequency, decimation_factor, filter_type=lowpass with bw / tw :99-106, and
// gr::filter::freq_xlating_fir_filter_ccf::make(decimation, taps, IF, fs) :115); Fir_Filter is the same
// stage with IF = 0.
//
// GNU Radio is not in the reference tree; freq_xlating_fir_filter_ccf(D, taps, fc, fs) is restated from
// its published definition.  With ω = 2π·fc/fs, T real taps h and zeros before the stream,
//   y[k] = e^{−jωDk} · Σ_{i<T} (h[i]·e^{jωi}) · x[kD − i] = Σ_{i<T} h[i] · x[kD − i] · e^{−jω(kD − i)}.
// The device runs the second form (mix, then a real-tap FIR: half the multiplies).
//
// Exact phase.  The phasor of input sample n (absolute index since create / reset) is
// e^{−j2π·frac(fc·n/fs)}; with integer fc and fs, frac(fc·n/fs) = ((fc mod fs)·(n mod fs) mod fs)/fs in
// 64-bit integers (fs < 2³¹), so the phase is as good hours into a file as at its start.  The fraction is
// divided and sincospi'd in double and rounded once to float: a pure function of n.
//
// Device form: one launch per run for all bands.  A 256-lane workgroup owns a tile of L input samples
// plus the max_b(T_b) − 1 samples before it.  Each lane reads its share of that span from HBM once
// (format conversion in the load; samples before the call come from the carried history) and keeps it
// in registers; then, band after band, the lanes write the span mixed by that band's phasors into LDS
// and lane j forms output j of the tile as a serial sum in tap order (i = 0 first), so every output is a
// function of the stream and its own index only — not of the tile shape or of where calls are cut.
// The launch also writes the next call's history (the last max T − 1 raw samples of history ‖ input) and
// sample count into the other half of a double buffer.  Nothing returns to the host.
// LDS: 8·(L + max T − 1) B = 16 KiB (max T ≤ 1025, L = 2049 − max T) or 64 KiB (L = 8193 − max T).
// HBM: s B in + Σ_b 8/D_b B out per input sample (s = 8, 4 or 2; real items 4, 2 or 1; bit-packed items
// 0.25 to 1), plus the tile overlap re-read from L2.
//
// Input items beside the three complex ones: real-sampled IF (the adapter's float / short / byte item
// types, freq_xlating_fir_filter.cc:118-159: freq_xlating_fir_filter_fcf / _scf) and 2- or 4-bit fields
// packed into bytes (GNSSHIP_FMT_PACKED: the reference's Two_Bit_Packed, Nsr, Two_Bit_Cpx and
// Four_Bit_Cpx file sources).  Both are conversions in the span's load; a real span is held as one float
// per sample and mixed with two multiplies, which equals the complex mix of (x, 0) up to signs of zero.
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "host_api.h"

#pragma clang fp contract(off)

namespace gnsship {
size_t fmt_bytes(int fmt);
}  // namespace gnsship

using namespace gnsship;

namespace {

constexpr int kCondThreads = 256;
constexpr int kCondMaxBands = 4;
constexpr int kCondMaxTaps = 4096;
// Span samples a lane holds: the kernel is built for 8 (spans up to 2048 samples, 16 KiB of LDS: every
// filter of up to 1025 taps) and for 32 (up to 8192 samples, 64 KiB: the longer ones).
constexpr int kCondRegsSmall = 8, kCondRegsLarge = 32;
constexpr int kCondSpanSmall = kCondThreads * kCondRegsSmall, kCondSpanLarge = kCondThreads * kCondRegsLarge;

struct CondBandDev {
    const float* taps;  // h[0..T − 1]
    float2* out;
    int32_t n_taps;
    int32_t decim;
    uint32_t fc_mod;     // fc mod fs, in [0, fs)
    uint32_t step_mod;   // (fc_mod · kCondThreads) mod fs
};

// A packed format for the loads.  shifts: the bit offset of the field of each sample slot of a byte, 8 bits
// per slot — real: slots 0..3; complex: re of slots 0, 1 in bits 0-15 and im in bits 16-31.
// info: field width | log2(samples per byte) << 8 | (1: value 2s + 1, 0: value s) << 16.
struct CondPack {
    uint32_t shifts;
    uint32_t info;
};

struct CondArgs {
    CondBandDev band[kCondMaxBands];
    int32_t n_bands;
    int32_t tile;        // L
    int32_t n_hist;      // max T − 1
    uint32_t fs;
    int64_t n_in;
    const float2* hist_old;
    float2* hist_new;
    const int64_t* count_old;  // absolute index of this call's first sample
    int64_t* count_new;
    CondPack pack;       // packed formats only (last: the other formats' argument layout is unchanged)
};

// Load shapes of the packed formats (kernel template values beside GNSSHIP_FMT_*; not ABI values): the
// field width, order and value map are wave-uniform scalars (CondPack), so one instantiation serves every
// real and one every complex packing.
constexpr int kCondPackedReal = 6, kCondPackedCplx = 7;

template <int FMT>
constexpr bool cond_is_real() { return FMT == GNSSHIP_FMT_RF32 || FMT == GNSSHIP_FMT_RI16 || FMT == GNSSHIP_FMT_RI8 || FMT == kCondPackedReal; }

// Field j of a byte: the two's-complement integer s of `bits` bits at bit offset `shift`; the sample value
// is 2s + 1 (m = 1) or s (m = 0).
__device__ __forceinline__ float cond_field(uint32_t byte, uint32_t shift, uint32_t bits, int m)
{
    const int32_t s = static_cast<int32_t>(byte << (32u - bits - shift)) >> (32u - bits);
    return static_cast<float>(s * (m + 1) + m);
}

// Sample i of the call's input as (re, im); im = 0 for the real formats.  Packed: sample i sits in byte
// i >> log2(samples per byte) at slot i mod (samples per byte), whatever i the tile starts at.
template <int FMT>
__device__ __forceinline__ float2 cond_load(const void* in, int64_t i, const CondPack pk)
{
    if constexpr (FMT == GNSSHIP_FMT_CF32) {
        return reinterpret_cast<const float2*>(in)[i];
    } else if constexpr (FMT == GNSSHIP_FMT_CI16) {
        const short2 v = reinterpret_cast<const short2*>(in)[i];
        return make_float2(static_cast<float>(v.x), static_cast<float>(v.y));
    } else if constexpr (FMT == GNSSHIP_FMT_CI8) {
        const char2 v = reinterpret_cast<const char2*>(in)[i];
        return make_float2(static_cast<float>(v.x), static_cast<float>(v.y));
    } else if constexpr (FMT == GNSSHIP_FMT_RF32) {
        return make_float2(reinterpret_cast<const float*>(in)[i], 0.0f);
    } else if constexpr (FMT == GNSSHIP_FMT_RI16) {
        return make_float2(static_cast<float>(reinterpret_cast<const short*>(in)[i]), 0.0f);
    } else if constexpr (FMT == GNSSHIP_FMT_RI8) {
        return make_float2(static_cast<float>(reinterpret_cast<const signed char*>(in)[i]), 0.0f);
    } else {
        const uint32_t bits = pk.info & 0xffu, l = (pk.info >> 8) & 0xffu;
        const int m = static_cast<int>(pk.info >> 16);
        const uint32_t byte = reinterpret_cast<const uint8_t*>(in)[i >> l];
        const uint32_t sh = pk.shifts >> (8u * (static_cast<uint32_t>(i) & ((1u << l) - 1u)));
        if constexpr (FMT == kCondPackedReal)
            return make_float2(cond_field(byte, sh & 0xffu, bits, m), 0.0f);
        else
            return make_float2(cond_field(byte, sh & 0xffu, bits, m), cond_field(byte, (sh >> 16) & 0xffu, bits, m));
    }
}

template <int FMT, int kCondRegs>
__global__ __launch_bounds__(kCondThreads) void cond_xlating_fir_kernel(const void* __restrict__ in, const CondArgs a)
{
    extern __shared__ float2 cond_lds[];
    const int tid = threadIdx.x;
    const int n_hist = a.n_hist;
    const int64_t t0 = static_cast<int64_t>(blockIdx.x) * a.tile;  // tile = call-relative samples [t0, t0 + len)
    const int len = static_cast<int>((a.n_in - t0) < a.tile ? (a.n_in - t0) : a.tile);
    const int64_t g0 = t0 - n_hist;  // call-relative index of span slot 0 (< 0: history)
    const int span = n_hist + len;   // <= kCondThreads · kCondRegs (gnsship_cond_create)
    const int64_t first = *a.count_old;

    // the next call's history and sample count (the other half of the double buffer)
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCondThreads + tid; i < n_hist; i += static_cast<int64_t>(gridDim.x) * kCondThreads) {
        const int64_t g = a.n_in - n_hist + i;
        a.hist_new[i] = g < 0 ? a.hist_old[n_hist + g] : cond_load<FMT>(in, g, a.pack);
    }
    if (blockIdx.x == 0 && tid == 0) *a.count_new = first + a.n_in;

    // the span, once from HBM into registers
    constexpr bool kReal = cond_is_real<FMT>();
    using raw_t = std::conditional_t<kReal, float, float2>;
    raw_t raw[kCondRegs];
#pragma unroll
    for (int r = 0; r < kCondRegs; r++) {
        const int idx = r * kCondThreads + tid;
        if constexpr (kReal) {
            // through a scalar: a conditional write into raw[] made the 32-register form one 32-wide vector
            // value (1.8 KiB of scratch, 1 wave/SIMD); this way 187 VGPRs, none
            float v = 0.0f;
            if (idx < span) {
                const int64_t g = g0 + idx;
                v = g < 0 ? a.hist_old[n_hist + g].x : cond_load<FMT>(in, g, a.pack).x;
            }
            raw[r] = v;
        } else {
            raw[r] = make_float2(0.0f, 0.0f);
            if (idx < span) {
                const int64_t g = g0 + idx;
                raw[r] = g < 0 ? a.hist_old[n_hist + g] : cond_load<FMT>(in, g, a.pack);
            }
        }
    }
    // (absolute index of this lane's slot 0) mod fs; before the stream's sample 0 the samples are zero
    int64_t nm = (first + g0 + tid) % static_cast<int64_t>(a.fs);
    if (nm < 0) nm += a.fs;

    for (int b = 0; b < a.n_bands; b++) {
        const CondBandDev bd = a.band[b];
        const int lo = n_hist - (bd.n_taps - 1);  // slots below are not read by this band
        uint32_t rr = static_cast<uint32_t>((static_cast<uint64_t>(bd.fc_mod) * static_cast<uint64_t>(nm)) % a.fs);
        const double inv_scale = 2.0 / static_cast<double>(a.fs);
#pragma unroll
        for (int r = 0; r < kCondRegs; r++) {
            const int idx = r * kCondThreads + tid;
            if (idx >= lo && idx < span) {
                // e^{−j2π·rr/fs}: (cos, −sin), one rounding to float each
                double s, c;
                sincospi(static_cast<double>(rr) * inv_scale, &s, &c);
                const float cf = static_cast<float>(c), sf = static_cast<float>(s);
                if constexpr (kReal) {
                    // (x, 0)·(cos, −sin): what the complex form gives up to signs of zero
                    const float x = raw[r];
                    cond_lds[idx] = make_float2(__fmul_rn(x, cf), -__fmul_rn(x, sf));
                } else {
                    const float2 x = raw[r];
                    cond_lds[idx] = make_float2(__fadd_rn(__fmul_rn(x.x, cf), __fmul_rn(x.y, sf)), __fsub_rn(__fmul_rn(x.y, cf), __fmul_rn(x.x, sf)));
                }
            }
            rr += bd.step_mod;  // < 2·fs < 2³²
            if (rr >= a.fs) rr -= a.fs;
        }
        __syncthreads();
        const int64_t d = bd.decim;
        const int64_t k_lo = (t0 + d - 1) / d, k_hi = (t0 + len + d - 1) / d;  // outputs k with k·D in the tile
        for (int64_t k = k_lo + tid; k < k_hi; k += kCondThreads) {
            const float2* z = cond_lds + static_cast<int>(k * d - g0);  // slot of x[kD]; z[−i] = x[kD − i]
            float re = 0.0f, im = 0.0f;
#pragma unroll 8
            for (int i = 0; i < bd.n_taps; i++) {
                const float h = bd.taps[i];
                const float2 v = z[-i];
                re = __fmaf_rn(h, v.x, re);
                im = __fmaf_rn(h, v.y, im);
            }
            bd.out[k] = make_float2(re, im);
        }
        __syncthreads();
    }
}

__global__ void cond_set_count_kernel(int64_t* count, int64_t value) { *count = value; }

// The loads' description of a valid packed format (zeros for the others).  Field j of a byte in stream
// order sits at bit offset bits·j (LSB first) or 8 − bits·(j + 1) (MSB first); a complex sample m takes
// fields 2m, 2m + 1 as (re, im) (IQ) or (im, re) (QI).
CondPack cond_pack(int fmt)
{
    CondPack pk = {0u, 0u};
    if (!GNSSHIP_FMT_IS_PACKED(fmt)) return pk;
    const int bits = GNSSHIP_FMT_PACKED_BITS(fmt), comp = GNSSHIP_FMT_PACKED_COMPONENTS(fmt);
    const bool msb = GNSSHIP_FMT_PACKED_ORDER(fmt) == GNSSHIP_FMT_PACKED_MSB_FIRST;
    const int fields = 8 / bits;
    auto offset = [&](int j) { return static_cast<uint32_t>(msb ? 8 - bits * (j + 1) : bits * j); };
    int log2_spb = 0;
    if (comp == GNSSHIP_FMT_PACKED_REAL) {
        for (int j = 0; j < fields; j++) pk.shifts |= offset(j) << (8 * j);
        log2_spb = fields == 4 ? 2 : 1;
    } else {
        const int re = comp == GNSSHIP_FMT_PACKED_QI ? 1 : 0;
        for (int m = 0; m < fields / 2; m++) pk.shifts |= (offset(2 * m + re) << (8 * m)) | (offset(2 * m + 1 - re) << (16 + 8 * m));
        log2_spb = fields == 4 ? 1 : 0;
    }
    const uint32_t two_s_plus_1 = GNSSHIP_FMT_PACKED_MAP(fmt) == GNSSHIP_FMT_PACKED_MAP_2S1 ? 1u : 0u;
    pk.info = static_cast<uint32_t>(bits) | (static_cast<uint32_t>(log2_spb) << 8) | (two_s_plus_1 << 16);
    return pk;
}

}  // namespace

// Bits per input sample of a format the conditioner reads (0: not one).  fmt_bytes() stays 0 for the real
// and packed formats: the engines do not read them.
extern "C" int gnsship_cond_fmt_bits(int fmt)
{
    switch (fmt) {
    case GNSSHIP_FMT_CF32: return 64;
    case GNSSHIP_FMT_CI16: return 32;
    case GNSSHIP_FMT_CI8: return 16;
    case GNSSHIP_FMT_RF32: return 32;
    case GNSSHIP_FMT_RI16: return 16;
    case GNSSHIP_FMT_RI8: return 8;
    default: break;
    }
    if (!GNSSHIP_FMT_IS_PACKED(fmt)) return 0;
    const int bits = GNSSHIP_FMT_PACKED_BITS(fmt), comp = GNSSHIP_FMT_PACKED_COMPONENTS(fmt);
    if ((bits != 2 && bits != 4) || comp > GNSSHIP_FMT_PACKED_QI) return 0;
    return comp == GNSSHIP_FMT_PACKED_REAL ? bits : 2 * bits;
}

struct gnsship_cond {
    gnsship_ctx* ctx = nullptr;
    int n_bands = 0;
    int tile = 0, n_hist = 0;
    uint32_t fs = 0;
    int64_t max_in = 0;
    int64_t count_host = 0;  // mirror of the device count (every run adds n_in), for gnsship_cond_samples_in
    CondBandDev band[kCondMaxBands] = {};
    float* taps_dev[kCondMaxBands] = {};
    float2* out_dev[kCondMaxBands] = {};
    float2* hist_dev[2] = {nullptr, nullptr};
    int64_t* count_dev = nullptr;  // [2]
    int cur = 0;
    DevBuf stage_dev;  // host input
};

// The adapter's filter_type=lowpass taps (freq_xlating_fir_filter.cc:99-106):
// firdes::low_pass(1.0, fs, bw, tw), bw defaulting to (fs / decimation) / 2 and tw to bw / 10.
extern "C" int gnsship_cond_lowpass_taps(double fs, int decimation, double bw, double tw, float* taps, int taps_cap, int* n_taps)
{
    if (!n_taps || decimation < 1 || !(fs > 0.0) || bw < 0.0 || tw < 0.0) return GNSSHIP_E_INVAL;
    if (bw == 0.0) bw = (fs / decimation) / 2;
    if (tw == 0.0) tw = bw / 10.0;
    return gnsship_firdes_low_pass(1.0, fs, bw, tw, taps, taps_cap, n_taps);
}

extern "C" int gnsship_cond_destroy(gnsship_cond* c)
{
    if (!c) return GNSSHIP_E_INVAL;
    quiesce(c->ctx);
    for (int b = 0; b < kCondMaxBands; b++) free_all({c->taps_dev[b], c->out_dev[b]});
    free_all({c->hist_dev[0], c->hist_dev[1], c->count_dev});
    release(c->stage_dev);
    delete c;
    return GNSSHIP_OK;
}

extern "C" int gnsship_cond_create(gnsship_ctx* ctx, double fs_in, const gnsship_cond_band* bands, int n_bands, int64_t max_in_samples,
    gnsship_cond** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!bands || n_bands < 1 || n_bands > kCondMaxBands) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: 1 <= n_bands <= 4");
    if (!(fs_in >= 1.0) || fs_in >= 2147483648.0 || fs_in != std::floor(fs_in))
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: fs_in must be a whole number of Hz in [1, 2^31)");
    const int64_t fs = static_cast<int64_t>(fs_in);
    // the grid (one workgroup per tile of >= 1 sample) and the output buffers are sized from this
    if (max_in_samples < 1 || max_in_samples > GNSSHIP_COND_MAX_IN_SAMPLES)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: 1 <= max_in_samples <= 2^30");
    int t_max = 1;
    for (int b = 0; b < n_bands; b++) {
        const gnsship_cond_band& bd = bands[b];
        if (!(std::fabs(bd.if_hz) < 9.0e15) || bd.if_hz != std::floor(bd.if_hz))
            return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: if_hz must be a whole number of Hz");
        if (bd.decimation < 1) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: decimation >= 1");
        if (!bd.taps || bd.n_taps < 1 || bd.n_taps > kCondMaxTaps) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: 1 <= n_taps <= 4096");
        if (max_in_samples < bd.decimation) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_create: max_in_samples below a band's decimation");
        t_max = std::max(t_max, bd.n_taps);
    }
    if (int rc = set_device(ctx)) return rc;
    gnsship_cond* c = new (std::nothrow) gnsship_cond();
    if (!c) return GNSSHIP_E_NOMEM;
    c->ctx = ctx;
    c->n_bands = n_bands;
    c->fs = static_cast<uint32_t>(fs);
    c->max_in = max_in_samples;
    c->n_hist = t_max - 1;
    c->tile = (c->n_hist <= kCondSpanSmall / 2 ? kCondSpanSmall : kCondSpanLarge) - c->n_hist;  // >= half the span
    const size_t n_hist_alloc = static_cast<size_t>(c->n_hist > 0 ? c->n_hist : 1);
    hipError_t e = hipSuccess;
    for (int b = 0; b < n_bands && e == hipSuccess; b++) {
        const gnsship_cond_band& bd = bands[b];
        int64_t fc = static_cast<int64_t>(bd.if_hz) % fs;
        if (fc < 0) fc += fs;
        e = hipMalloc(&c->taps_dev[b], sizeof(float) * bd.n_taps);
        if (e == hipSuccess) e = hipMemcpy(c->taps_dev[b], bd.taps, sizeof(float) * bd.n_taps, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&c->out_dev[b], sizeof(float2) * static_cast<size_t>(max_in_samples / bd.decimation));
        c->band[b].taps = c->taps_dev[b];
        c->band[b].out = c->out_dev[b];
        c->band[b].n_taps = bd.n_taps;
        c->band[b].decim = bd.decimation;
        c->band[b].fc_mod = static_cast<uint32_t>(fc);
        c->band[b].step_mod = static_cast<uint32_t>((static_cast<uint64_t>(fc) * kCondThreads) % static_cast<uint64_t>(fs));
    }
    if (e == hipSuccess)  // zeroed on the stream: ordered before the runs
        e = alloc_all(ctx, {dev_alloc(&c->hist_dev[0], n_hist_alloc, true), dev_alloc(&c->hist_dev[1], n_hist_alloc, true), dev_alloc(&c->count_dev, 2, true)});
    if (e != hipSuccess) {
        gnsship_cond_destroy(c);
        return hip_fail(ctx, e, "gnsship_cond_create");
    }
    *out = c;
    return GNSSHIP_OK;
}

extern "C" int gnsship_cond_reset(gnsship_cond* c, uint64_t first_sample)
{
    if (!c) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = c->ctx;
    if (first_sample > static_cast<uint64_t>(INT64_MAX) / 2) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_reset: first_sample below 2^62");
    if (int rc = set_device(ctx)) return rc;
    const size_t hist_bytes = sizeof(float2) * static_cast<size_t>(c->n_hist > 0 ? c->n_hist : 1);
    hipError_t e = hipMemsetAsync(c->hist_dev[c->cur], 0, hist_bytes, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "gnsship_cond_reset");
    hipLaunchKernelGGL(cond_set_count_kernel, dim3(1), dim3(1), 0, ctx->stream, c->count_dev + c->cur, static_cast<int64_t>(first_sample));
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "gnsship_cond_reset(launch)");
    c->count_host = static_cast<int64_t>(first_sample);
    return GNSSHIP_OK;
}

extern "C" int gnsship_cond_samples_in(gnsship_cond* c, uint64_t* n)
{
    if (!c || !n) return GNSSHIP_E_INVAL;
    *n = static_cast<uint64_t>(c->count_host);
    return GNSSHIP_OK;
}

extern "C" int gnsship_cond_run(gnsship_cond* c, const void* in, int fmt, int in_on_device, int64_t n_in, void* const* dev_dst,
    float* const* host_out, void** dev_out, int64_t* n_out)
{
    if (!c) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = c->ctx;
    const int bps = gnsship_cond_fmt_bits(fmt);
    if (!in || bps == 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_run: null input or unknown sample format");
    if (n_in < 1 || n_in > c->max_in) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_run: 1 <= n_in <= max_in_samples");
    for (int b = 0; b < c->n_bands; b++)
        if (n_in % c->band[b].decim != 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_run: n_in must be a multiple of every band's decimation");
    if (bps < 8 && n_in % (8 / bps) != 0)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cond_run: n_in must be a multiple of the samples per byte of a packed format");
    if (int rc = set_device(ctx)) return rc;
    const void* src = in;
    if (!in_on_device) {
        const size_t bytes = (static_cast<size_t>(n_in) * static_cast<size_t>(bps) + 7) / 8;
        if (int rc = stage(ctx, c->stage_dev, in, bytes, "gnsship_cond_run", "stage")) return rc;
        src = c->stage_dev.dev;
    }
    CondArgs a;
    for (int b = 0; b < kCondMaxBands; b++) a.band[b] = c->band[b];
    for (int b = 0; b < c->n_bands; b++)
        if (dev_dst && dev_dst[b]) a.band[b].out = static_cast<float2*>(dev_dst[b]);
    a.n_bands = c->n_bands;
    a.tile = c->tile;
    a.n_hist = c->n_hist;
    a.fs = c->fs;
    a.n_in = n_in;
    a.hist_old = c->hist_dev[c->cur];
    a.hist_new = c->hist_dev[c->cur ^ 1];
    a.count_old = c->count_dev + c->cur;
    a.count_new = c->count_dev + (c->cur ^ 1);
    a.pack = cond_pack(fmt);
    const int64_t blocks = (n_in + c->tile - 1) / c->tile;  // <= 2^30: n_in <= GNSSHIP_COND_MAX_IN_SAMPLES
    const size_t lds = sizeof(float2) * static_cast<size_t>(c->n_hist + c->tile);
    const dim3 grid(static_cast<unsigned>(blocks)), block(kCondThreads);
    const bool small = c->n_hist + c->tile <= kCondSpanSmall;
#define GNSSHIP_COND_LAUNCH(FMT)                                                                                                      \
    if (small)                                                                                                                        \
        hipLaunchKernelGGL((cond_xlating_fir_kernel<FMT, kCondRegsSmall>), grid, block, lds, ctx->stream, src, a);                    \
    else                                                                                                                              \
        hipLaunchKernelGGL((cond_xlating_fir_kernel<FMT, kCondRegsLarge>), grid, block, lds, ctx->stream, src, a)
    switch (fmt) {
    case GNSSHIP_FMT_CF32:
        GNSSHIP_COND_LAUNCH(GNSSHIP_FMT_CF32);
        break;
    case GNSSHIP_FMT_CI16:
        GNSSHIP_COND_LAUNCH(GNSSHIP_FMT_CI16);
        break;
    case GNSSHIP_FMT_CI8:
        GNSSHIP_COND_LAUNCH(GNSSHIP_FMT_CI8);
        break;
    case GNSSHIP_FMT_RF32:
        GNSSHIP_COND_LAUNCH(GNSSHIP_FMT_RF32);
        break;
    case GNSSHIP_FMT_RI16:
        GNSSHIP_COND_LAUNCH(GNSSHIP_FMT_RI16);
        break;
    case GNSSHIP_FMT_RI8:
        GNSSHIP_COND_LAUNCH(GNSSHIP_FMT_RI8);
        break;
    default:  // a valid packed format: gnsship_cond_fmt_bits accepted it
        if (GNSSHIP_FMT_PACKED_COMPONENTS(fmt) == GNSSHIP_FMT_PACKED_REAL) {
            GNSSHIP_COND_LAUNCH(kCondPackedReal);
        } else {
            GNSSHIP_COND_LAUNCH(kCondPackedCplx);
        }
        break;
    }
#undef GNSSHIP_COND_LAUNCH
    if (int rc = launched(ctx, "gnsship_cond_run(launch)")) return rc;
    c->cur ^= 1;
    c->count_host += n_in;
    DevCopy copies[kCondMaxBands] = {};
    for (int b = 0; b < c->n_bands; b++) {
        const int64_t nk = n_in / c->band[b].decim;
        if (host_out) copies[b] = {host_out[b], a.band[b].out, sizeof(float2) * static_cast<size_t>(nk)};
        if (dev_out) dev_out[b] = a.band[b].out;
        if (n_out) n_out[b] = nk;
    }
    return copy_out(ctx, copies, static_cast<size_t>(c->n_bands), "gnsship_cond_run(download)");
}
