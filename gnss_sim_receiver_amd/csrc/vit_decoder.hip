// vit_decoder.hip — the K = 7, rate-1/2 Viterbi decoder of the Galileo telemetry block for gfx950, with the two
// steps the block runs ahead of it: the first thing galileo_telemetry_decoder_gs does to an I/NAV, F/NAV or C/NAV
// page (decode_INAV_word / decode_FNAV_word / decode_CNAV_word, galileo_telemetry_decoder_gs.cc:354-371, :585-599,
// :684-697) — de-interleave (:342-351), undo the NOT gate of G2 (:362-368), Viterbi_Decoder::decode
// (telemetry_decoder/libs/viterbi_decoder.cc:47-120) — for many channels' pages in one launch.
//
// Layout: one wavefront decodes one frame, lane = next state s' (64 states = 64 lanes); a workgroup of
// kVitFramesPerWg waves holds as many frames, each wave with its own slice of dynamic LDS: per step of the T = LL + 6
// one 16-byte pair of decision word and "stored" word, then the 2·T de-interleaved symbols (24·T bytes, 12 KiB at
// the 1024-symbol limit, 48 KiB per workgroup).
//   load       lanes read the frame as received (coalesced) and write each symbol to its de-interleaved place,
//              out[c·rows + r] = in[r·cols + c], with the frame's `negate` flag (the block's 180° case, :1026-1029)
//              and the G2 flip (odd de-interleaved positions) applied as sign changes on the way.
//   trellis    per step: the two predecessor metrics by cross-lane read (p0 = (s' & 31) << 1, p1 = p0 | 1), one
//              float add each, the reference's two strict comparisons in its order (p0 first, so p0 wins a tie;
//              an entry neither candidate lifts above −1e7 is not stored), the decision and the "stored" flag as
//              one 64-bit ballot word each, a wave-wide maximum (DPP within rows of 16 lanes, lane reads across) and
//              the subtraction.
//   traceback  serial, one lane, out of LDS: from state 0, the 6 tail steps skipped, LL bytes of 0 / 1.  An entry
//              nothing stored reads as predecessor 0, bit 0 (a new object's content; include/gnsship.h).
// Trellis and traceback are vit_wave.h's, shared with the telemetry framing kernel (tlm_galileo.hip).
//
// REFERENCE mode reproduces Viterbi_Decoder::decode as written: only the first symbol of each pair enters the
// metric (:61 copies d_nn − 1 = 1 value; Gamma = {0, 0 + 0, 0 + r0, (0 + 0) + r0}, :151-166) and the 64 metrics
// carry over from call to call per channel (:56 sets entry 0 alone).  FULL mode puts both symbols in the metric and
// starts every frame from state 0 alone.  Every float operation is one the reference performs (add, compare,
// subtract), contraction off: bit-exact against tests/viterbi_model.py.  No operand is ever −0 (0 + x never is),
// so the maximum depends on the values alone.  Inputs are finite by contract; with NaN / Inf the result is
// unspecified, but every index is formed from lane numbers and ballot bits and stays in range.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "host_api.h"
#include "vit_wave.h"

#pragma clang fp contract(off)

using namespace gnsship;

namespace {

constexpr int kVitFramesPerWg = 4;  // waves per workgroup: 4 · 24 · 512 = 48 KiB of LDS at the longest frame

struct VitArgs {
    const float* sym;         // n_frames × 2·steps, as received
    const int32_t* channels;  // per frame
    const uint8_t* negate;    // per frame, or null
    float* sections;          // max_channels × 64
    uint8_t* bits;            // n_frames × data_length
    int32_t n_frames;
    int32_t steps;            // LL + 6
    int32_t data_length;      // LL
    int32_t rows, cols;       // interleaver, rows 0 = none
    int32_t invert_g2, mode;
    int32_t g0, g1;
};

// kFull: GNSSHIP_VIT_MODE_FULL (both symbols in the metric, nothing carried)
template <bool kFull>
__global__ __launch_bounds__(kVitFramesPerWg * 64) void vit_decode_kernel(const VitArgs a)
{
    extern __shared__ ulonglong2 vit_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kVitFramesPerWg + wave;
    const bool active = f < a.n_frames;  // wave-uniform; idle waves only meet the barriers
    const int T = a.steps, LL = a.data_length;
    ulonglong2* surv = vit_lds + static_cast<size_t>(wave) * vit_wave_lds_words(T);  // per step: x decisions, y stored
    float* sym = reinterpret_cast<float*>(surv + T);
    uint8_t* obits = reinterpret_cast<uint8_t*>(sym);  // the symbols are dead once the trellis is through

    if (active) {
        const float* in = a.sym + f * (2 * T);
        const bool neg = a.negate != nullptr && a.negate[f] != 0;
        for (int i = lane; i < 2 * T; i += 64) {
            float v = in[i];
            const int j = vit_place(i, a.rows, a.cols, neg, a.invert_g2 != 0, v);  // rows · cols == 2·T (checked by create), so j < 2·T
            sym[j] = v;
        }
    }
    __syncthreads();

    if (active) {
        const int64_t sec = static_cast<int64_t>(a.channels[f]) * kVitStates + lane;
        const float prev = vit_wave_trellis<kFull>(surv, sym, T, kFull ? -kVitMaxLog : a.sections[sec], lane, a.g0, a.g1);
        if (!kFull) a.sections[sec] = prev;
    }
    __syncthreads();

    if (active && lane == 0) vit_wave_traceback(surv, obits, T, LL);
    __syncthreads();

    if (active)
        for (int i = lane; i < LL; i += 64) a.bits[f * LL + i] = obits[i];
}

__global__ void vit_fill_kernel(float* p, int64_t n, float v)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

struct gnsship_vit {
    gnsship_ctx* ctx = nullptr;
    gnsship_vit_conf conf = {};
    int32_t max_channels = 0;
    int32_t frame = 0;  // symbols per frame
    float* sections_dev = nullptr;
    DevBuf channels_dev, negate_dev, bits_dev;  // per frame: int32_t, uint8_t, data_length × uint8_t
    DevBuf sym_dev;                             // host symbols (float)
    std::vector<uint32_t> seen;  // per channel: the run that last named it
    uint32_t run_id = 0;
};

extern "C" int gnsship_vit_destroy(gnsship_vit* v)
{
    if (!v) return GNSSHIP_E_INVAL;
    quiesce(v->ctx);
    free_all({v->sections_dev});
    for (DevBuf* b : {&v->channels_dev, &v->negate_dev, &v->bits_dev, &v->sym_dev}) release(*b);
    delete v;
    return GNSSHIP_OK;
}

static int vit_fill(gnsship_vit* v, int64_t first, int64_t n, const char* where)
{
    gnsship_ctx* ctx = v->ctx;
    hipLaunchKernelGGL(vit_fill_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ctx->stream, v->sections_dev + first, n, -kVitMaxLog);
    return launched(ctx, where);
}

extern "C" int gnsship_vit_create(gnsship_ctx* ctx, const gnsship_vit_conf* conf, int32_t max_channels, gnsship_vit** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: null configuration");
    if (conf->constraint_length != 7 || conf->rate_n != 2) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: constraint_length 7 and rate_n 2 only");
    for (int i = 0; i < 2; i++)
        if (conf->g[i] < 0 || conf->g[i] > 127) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: g[] must be 7-bit words");
    if (conf->data_length < 1 || conf->data_length > GNSSHIP_VIT_MAX_FRAME_SYMBOLS / 2 - kVitTail)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: data_length >= 1 and 2*(data_length + 6) <= 1024 symbols");
    const int32_t frame = 2 * (conf->data_length + kVitTail);
    const bool none = conf->interleaver_rows == 0 && conf->interleaver_cols == 0;
    if (!none && (conf->interleaver_rows < 1 || conf->interleaver_cols < 1 ||
                     static_cast<int64_t>(conf->interleaver_rows) * conf->interleaver_cols != frame))
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: interleaver_rows*interleaver_cols must equal 2*(data_length + 6)");
    if (conf->mode != GNSSHIP_VIT_MODE_REFERENCE && conf->mode != GNSSHIP_VIT_MODE_FULL) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: unknown mode");
    if (max_channels < 1 || max_channels > GNSSHIP_VIT_MAX_CHANNELS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_create: 1 <= max_channels <= 2^20");
    if (int rc = set_device(ctx)) return rc;
    gnsship_vit* v = new (std::nothrow) gnsship_vit();
    if (!v) return GNSSHIP_E_NOMEM;
    v->ctx = ctx;
    v->conf = *conf;
    v->max_channels = max_channels;
    v->frame = frame;
    v->seen.assign(static_cast<size_t>(max_channels), 0u);
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&v->sections_dev), sizeof(float) * kVitStates * static_cast<size_t>(max_channels));
    if (e != hipSuccess) {
        gnsship_vit_destroy(v);
        return hip_fail(ctx, e, "gnsship_vit_create");
    }
    if (int rc = vit_fill(v, 0, static_cast<int64_t>(max_channels) * kVitStates, "gnsship_vit_create(fill)")) {
        gnsship_vit_destroy(v);
        return rc;
    }
    *out = v;
    return GNSSHIP_OK;
}

extern "C" int gnsship_vit_reset_channel(gnsship_vit* v, int32_t channel)
{
    if (!v) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = v->ctx;
    if (channel < 0 || channel >= v->max_channels) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_reset_channel: channel out of range");
    if (int rc = set_device(ctx)) return rc;
    return vit_fill(v, static_cast<int64_t>(channel) * kVitStates, kVitStates, "gnsship_vit_reset_channel");
}

extern "C" int gnsship_vit_state_get(gnsship_vit* v, int32_t channel, float* section)
{
    if (!v || !section) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = v->ctx;
    if (channel < 0 || channel >= v->max_channels) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_state_get: channel out of range");
    if (int rc = set_device(ctx)) return rc;
    return copy_out(ctx, {{section, v->sections_dev + static_cast<int64_t>(channel) * kVitStates, sizeof(float) * kVitStates}}, "gnsship_vit_state_get");
}

extern "C" int gnsship_vit_run(gnsship_vit* v, const float* symbols, int on_device, int32_t n_frames, const int32_t* channels,
    const uint8_t* negate, uint8_t* bits_host, void* bits_dev)
{
    if (!v) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = v->ctx;
    if (n_frames < 0 || n_frames > GNSSHIP_VIT_MAX_FRAMES) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_run: 0 <= n_frames <= 2^22");
    if (n_frames == 0) return GNSSHIP_OK;
    if (!symbols || !channels) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_run: null symbols or channels");
    for (int32_t i = 0; i < n_frames; i++)
        if (channels[i] < 0 || channels[i] >= v->max_channels) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_run: channel out of range");
    if (v->conf.mode == GNSSHIP_VIT_MODE_REFERENCE) {
        // a channel's frames are ordered through its carried metrics: one per call
        if (++v->run_id == 0) {
            std::fill(v->seen.begin(), v->seen.end(), 0u);
            v->run_id = 1;
        }
        for (int32_t i = 0; i < n_frames; i++) {
            if (v->seen[channels[i]] == v->run_id) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_vit_run: a channel may appear once per call in reference mode");
            v->seen[channels[i]] = v->run_id;
        }
    }
    if (int rc = set_device(ctx)) return rc;
    const int LL = v->conf.data_length;
    const size_t nf = static_cast<size_t>(n_frames);
    if (int rc = reserve(ctx, v->channels_dev, sizeof(int32_t) * nf, "gnsship_vit_run", "buffers")) return rc;
    if (int rc = reserve(ctx, v->negate_dev, nf, "gnsship_vit_run", "buffers")) return rc;
    if (int rc = reserve(ctx, v->bits_dev, nf * LL, "gnsship_vit_run", "buffers")) return rc;
    const float* src = symbols;
    if (!on_device) {
        if (int rc = stage(ctx, v->sym_dev, symbols, sizeof(float) * nf * v->frame, "gnsship_vit_run", "stage")) return rc;
        src = v->sym_dev.as<float>();
    }
    hipError_t e = hipMemcpyAsync(v->channels_dev.dev, channels, sizeof(int32_t) * nf, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && negate) e = hipMemcpyAsync(v->negate_dev.dev, negate, nf, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "gnsship_vit_run(upload)");
    VitArgs a = {};
    a.sym = src;
    a.channels = v->channels_dev.as<int32_t>();
    a.negate = negate ? v->negate_dev.as<uint8_t>() : nullptr;
    a.sections = v->sections_dev;
    a.bits = bits_dev ? static_cast<uint8_t*>(bits_dev) : v->bits_dev.as<uint8_t>();
    a.n_frames = n_frames;
    a.steps = LL + kVitTail;
    a.data_length = LL;
    a.rows = v->conf.interleaver_rows;
    a.cols = v->conf.interleaver_cols;
    a.invert_g2 = v->conf.invert_g2 ? 1 : 0;
    a.mode = v->conf.mode;
    a.g0 = v->conf.g[0];
    a.g1 = v->conf.g[1];
    const unsigned blocks = static_cast<unsigned>((n_frames + kVitFramesPerWg - 1) / kVitFramesPerWg);
    const size_t lds = static_cast<size_t>(kVitFramesPerWg) * 16 * vit_wave_lds_words(a.steps);  // <= 48 KiB
    if (a.mode == GNSSHIP_VIT_MODE_FULL)
        hipLaunchKernelGGL(vit_decode_kernel<true>, dim3(blocks), dim3(kVitFramesPerWg * 64), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL(vit_decode_kernel<false>, dim3(blocks), dim3(kVitFramesPerWg * 64), lds, ctx->stream, a);
    if (int rc = launched(ctx, "gnsship_vit_run(launch)")) return rc;
    return copy_out(ctx, {{bits_host, a.bits, nf * LL}}, "gnsship_vit_run(download)");
}
