// tlm_device.h — device helpers of the wave-per-channel telemetry kernels (tlm_galileo.hip, tlm_gps_lnav.hip,
// tlm_gps_cnav.hip, tlm_bds_dnav.hip).  tlm_glo_gnav.hip keeps a channel in one lane and uses none of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gnsship {

// A value every lane holds alike, moved to scalar registers.
__device__ __forceinline__ int tlm_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t tlm_uniform(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }
__device__ __forceinline__ uint64_t tlm_uniform64(uint64_t v)
{
    const uint32_t lo = tlm_uniform(static_cast<uint32_t>(v)), hi = tlm_uniform(static_cast<uint32_t>(v >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The sign-code history of the LNAV and DNAV kernels.  In HBM a channel keeps two bit strings (neg, pos; bit i is the i-th
// oldest entry); for a run they become a linear LDS buffer of codes, oldest first — 0 (zero, −0, NaN), 1 (> 0), 2 (< 0) —
// and are packed again once at the end.  One wavefront; the caller places the barriers.
// the `size` oldest entries to buf[0 .. size), zeros to the rest of buf[0 .. buf_size)
__device__ __forceinline__ void tlm_codes_unpack(uint8_t* buf, int buf_size, const uint32_t* neg, const uint32_t* pos, int size, int lane)
{
    for (int i = lane; i < buf_size; i += 64) {
        uint8_t code = 0;
        if (i < size) {
            const uint32_t ng = (neg[i >> 5] >> (i & 31)) & 1u, ps = (pos[i >> 5] >> (i & 31)) & 1u;
            code = ng ? 2 : (ps ? 1 : 0);
        }
        buf[i] = code;
    }
}
// buf[0 .. size) to the `words` (even) 32-bit words of neg and pos, by ballot; the bits from `size` on are zero
__device__ __forceinline__ void tlm_codes_pack(const uint8_t* buf, int words, uint32_t* neg, uint32_t* pos, int size, int lane)
{
    for (int w = 0; w < words / 2; w++) {
        const int i = 64 * w + lane;
        const uint8_t code = i < size ? buf[i] : 0;
        const unsigned long long ng = __ballot(code == 2), ps = __ballot(code == 1);
        if (lane == 0) {
            neg[2 * w] = static_cast<uint32_t>(ng);
            neg[2 * w + 1] = static_cast<uint32_t>(ng >> 32);
            pos[2 * w] = static_cast<uint32_t>(ps);
            pos[2 * w + 1] = static_cast<uint32_t>(ps >> 32);
        }
    }
}

}  // namespace gnsship
