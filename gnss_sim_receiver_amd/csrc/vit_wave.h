// vit_wave.h — one wavefront's share of the K = 7, rate-1/2 Viterbi decoder of the Galileo telemetry block
// (telemetry_decoder/libs/viterbi_decoder.cc:47-120): the trellis with lane = next state and the serial traceback, as
// vit_decoder.hip describes them.  Called by vit_decode_kernel (vit_decoder.hip: one frame per wave, frames handed in)
// and by tlm_kernel (tlm_galileo.hip: the frames a channel's frame-sync machine finds due).  Every float operation is
// one the reference performs (add, compare, subtract), in its order; include with contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gnsship {

constexpr int kVitStates = 64;
constexpr int kVitTail = 6;         // K − 1
constexpr float kVitMaxLog = 1e7f;  // d_MAXLOG

// 16-byte words of LDS per wave: T survivor words and 2·T symbols
__host__ __device__ constexpr int vit_wave_lds_words(int steps) { return steps + (steps + 1) / 2; }

__device__ __forceinline__ int vit_parity7(int x) { return __popc(x & 127) & 1; }

// nsc_enc_bit (viterbi_decoder.cc:183-204): the output symbol of the branch from state p with information bit `bit`
__device__ __forceinline__ int vit_branch(int g0, int g1, int bit, int p)
{
    const int w = (bit << 6) ^ p;
    return (vit_parity7(w & g0) << 1) | vit_parity7(w & g1);
}

// The order of finite floats as the order of signed integers: negative values get their magnitude bits inverted.
// Its own inverse.  (−0 would sort below +0; no operand here is ever −0.)
__device__ __forceinline__ int vit_order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

template <int kCtrl>
__device__ __forceinline__ int vit_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, kCtrl, 0xF, 0xF, true);  // every lane has a source lane in these patterns
}

// The maximum of a value over the wave, in every lane; all 64 lanes must be active and the values finite.  Taken on
// the integer keys, where a DPP operand folds into the max instruction and the last three maxima are scalar: four
// steps leave each row of 16 lanes with its own maximum (lane ^ 1, lane ^ 2 by quad_perm, then row_half_mirror and
// row_mirror), four lane reads join the rows.  The maximum of a set does not depend on the order it is taken in.
__device__ __forceinline__ float vit_wave_max(float x)
{
    constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kRowHalfMirror = 0x141, kRowMirror = 0x140;
    int v = vit_order_key(__float_as_int(x));
    v = max(v, vit_dpp<kQuadXor1>(v));
    v = max(v, vit_dpp<kQuadXor2>(v));
    v = max(v, vit_dpp<kRowHalfMirror>(v));
    v = max(v, vit_dpp<kRowMirror>(v));
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return __int_as_float(vit_order_key(max(max(r0, r1), max(r2, r3))));
}

// Where symbol i of a frame as received goes, and with which sign: out[c·rows + r] = in[r·cols + c] (rows 0: no
// interleaver), negated when `negate` (the block's 180° case, :1026-1029) and, with invert_g2, at the odd de-interleaved
// positions (:362-368).  rows · cols equals the frame length, so the position stays inside the frame.
__device__ __forceinline__ int vit_place(int i, int rows, int cols, bool negate, bool invert_g2, float& v)
{
    int j = i;
    if (rows > 0) {
        const int r = i / cols, c = i - r * cols;
        j = c * rows + r;
    }
    if (negate) v = -v;
    if (invert_g2 && (j & 1)) v = -v;
    return j;
}

// The trellis over T steps, all 64 lanes of the wave: sym holds the 2·T prepared symbols in LDS, surv receives per step
// the decision word (x) and the "stored" word (y); `prev` is this lane's carried metric (ignored in full mode and for
// lane 0, :56).  Returns the lane's metric after the last step.  kFull: GNSSHIP_VIT_MODE_FULL.
template <bool kFull>
__device__ __forceinline__ float vit_wave_trellis(ulonglong2* surv, const float* sym, int T, float prev, int lane, int g0, int g1)
{
    const int p0 = (lane & 31) << 1, p1 = p0 | 1, bit = lane >> 5;
    const int out0 = vit_branch(g0, g1, bit, p0), out1 = vit_branch(g0, g1, bit, p1);
    // the branch symbols' two bits select the terms of Gamma (:157-164)
    const bool a_lo = out0 & 1, a_hi = out0 & 2, b_lo = out1 & 1, b_hi = out1 & 2;
    if (kFull) prev = -kVitMaxLog;
    if (lane == 0) prev = 0.0f;  // :56
    float2 next = reinterpret_cast<const float2*>(sym)[0];
    for (int t = 0; t < T; t++) {
        const float2 r = next;
        next = reinterpret_cast<const float2*>(sym)[min(t + 1, T - 1)];  // ahead of the step that needs it
        // Gamma(0) = 0, Gamma(1) = 0 + rec[1], Gamma(2) = 0 + rec[0], Gamma(3) = (0 + rec[1]) + rec[0]; rec[1] stays 0
        // in reference mode, where Gamma(1) = 0 and Gamma(3) = (0 + 0) + rec[0] = Gamma(2)
        const float gm2 = 0.0f + r.x;
        float ga, gb;
        if (kFull) {
            const float gm1 = 0.0f + r.y, gm3 = gm1 + r.x;
            ga = a_hi ? (a_lo ? gm3 : gm2) : (a_lo ? gm1 : 0.0f);
            gb = b_hi ? (b_lo ? gm3 : gm2) : (b_lo ? gm1 : 0.0f);
        } else {
            ga = a_hi ? gm2 : 0.0f;
            gb = b_hi ? gm2 : 0.0f;
        }
        const float m0 = __shfl(prev, p0) + ga;
        const float m1 = __shfl(prev, p1) + gb;
        float cur = -kVitMaxLog;
        const bool s0 = m0 > cur;
        cur = s0 ? m0 : cur;
        const bool s1 = m1 > cur;
        cur = s1 ? m1 : cur;
        const unsigned long long d = __ballot(s1), s = __ballot(s0 || s1);
        if (lane == 0) surv[t] = make_ulonglong2(d, s);
        prev = cur - vit_wave_max(cur);
    }
    return prev;
}

// The traceback, one lane: from state 0, the 6 tail steps skipped, LL bytes of 0 / 1 into obits.  An entry nothing
// stored reads as predecessor 0, bit 0 (a new object's content; include/gnsship.h).
__device__ __forceinline__ void vit_wave_traceback(const ulonglong2* surv, uint8_t* obits, int T, int LL)
{
    int state = 0;
    for (int t = T - 1; t >= 0; t--) {
        const ulonglong2 w = surv[t];
        const bool st = (w.y >> state) & 1ull;
        if (t < LL) obits[t] = st ? static_cast<uint8_t>(state >> 5) : 0;
        state = st ? (((state & 31) << 1) | static_cast<int>((w.x >> state) & 1ull)) : 0;
    }
}

}  // namespace gnsship
