// code_bits.h — ±1 code replicas held as sign bits in LDS (trk_lane.hip, and trk_fast.hip where two
// float replicas leave its product ring too little room): the product a·c of a sample product with a
// ±1 chip is a sign flip, exact, so the taps are bit-identical to the float replica's.  Every chip must
// be ±1 (checked when the code is set — gnsship_code_set).
#pragma once
#include <cstdint>

#include "corr_device.h"

namespace gnsship {

// Sign-bit replica of a padded code (engine.h padded_code_quads): bit p of the table is chip
// p − kCodeMargin < 0 (p over the replica and its wrapped margins).
__host__ __device__ constexpr int lane_code_words(int code_cap_floats) { return (code_cap_floats + 31) / 32; }

// The chip (±1.0f) the resampler picks for tap shift `sh` at sample n (sn = step·(float)n): the chip
// index as code_at (corr_device.h) forms it, looked up in the sign-bit replica.
static_assert(kCodeMargin == 32, "chip i sits at bit i & 31 of word (i >> 5) + 1");
template <bool IN_MARGIN>
__device__ __forceinline__ float code_chip(const uint32_t* bits, int L, float sn, float sh, float rem)
{
    int i = cvt_floor_i32(__fsub_rn(__fadd_rn(sn, sh), rem));
    if constexpr (!IN_MARGIN) i = wrap_index(i, L);
    const uint32_t w = bits[(i >> 5) + 1];
    return __builtin_bit_cast(float, ((w >> (i & 31)) << 31) | 0x3f800000u);
}

// Build the sign-bit replica of code `cd` at dst (whole waves, one 64-chip ballot per step): wave
// `wave` of `n_waves` takes every n_waves-th step.
__device__ inline void stage_code_bits(uint32_t* dst, const CodeDesc& cd, int words, int lane, int wave = 0, int n_waves = 1)
{
    const int P = cd.len + 2 * kCodeMargin;
    for (int base = wave * kWave; base < 32 * words; base += n_waves * kWave) {
        const int i = base + lane;
        const float v = i < P ? cd.ptr[i - kCodeMargin] : 1.0f;
        const unsigned long long m = __ballot(v < 0.0f);
        if (lane == 0) {
            dst[base >> 5] = static_cast<uint32_t>(m);
            if ((base >> 5) + 1 < words) dst[(base >> 5) + 1] = static_cast<uint32_t>(m >> 32);
        }
    }
}

}  // namespace gnsship
