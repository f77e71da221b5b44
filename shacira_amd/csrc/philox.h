// philox.h -- the counter-based generator shared by mesh_sample.hip and shade.hip: Philox4x32-10, the two maps of a word to the unit
// interval and the Box-Muller step that makes three standard normals of four words. Every caller gets the same bits from the same
// (counter, key); a stream is told apart by the counter's upper words, which each file picks for itself.
#ifndef SHACIRA_PHILOX_H
#define SHACIRA_PHILOX_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace shacira {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
        const uint32_t hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kW0;
        k1 += kW1;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

__device__ __forceinline__ float unit_open_above(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }         // [0, 1)
__device__ __forceinline__ float unit_open_below(uint32_t w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }  // (0, 1]

// Box-Muller: two radii, two angles, three of the four normals
__device__ __forceinline__ void box_muller3(const uint32_t g[4], float out[3]) {
    const float r0 = sqrtf(-2.0f * logf(unit_open_below(g[0])));
    const float r1 = sqrtf(-2.0f * logf(unit_open_below(g[2])));
    float s0, c0, s1, c1;
    sincospif(2.0f * unit_open_above(g[1]), &s0, &c0);
    sincospif(2.0f * unit_open_above(g[3]), &s1, &c1);
    out[0] = r0 * c0;
    out[1] = r0 * s0;
    out[2] = r1 * c1;
    (void)s1;
}

}  // namespace shacira

#endif  // SHACIRA_PHILOX_H
