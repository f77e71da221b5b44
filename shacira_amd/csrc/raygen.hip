// raygen.hip -- rays and target colours of (view, pixel) pairs from per-camera records and the training images: their uint8 bytes
// (shacira_raygen) or the uint16 block sums of a mip level (shacira_raygen_sums, made by image_mip.hip); contracts in
// include/shacira_hip.h. The two differ in the pixel source only -- BytePixels / SumPixels of raygen_device.h, which hand the body a pixel's
// integers and their divisor -- and share every other line. One lane makes one ray:
//   reads    its two indices (or derives them from the ray number in the whole-view form), its jitter pair, the camera's record
//            (SHACIRA_RAYGEN_RECORD_FLOATS floats = five 16-byte loads; V records are a few KiB and stay in cache) and the
//            pixel's 3 or 4 bytes (6 or 8 bytes of sums);
//   writes   three floats each into origins, dirs and rgb, and one mask byte. Lane i stores at base + 12 i, so a wavefront's
//            64 lanes cover one contiguous run of 768 bytes per output: whole cache lines from one instruction whenever n is
//            large, whatever the order of the indices. No LDS, no atomics, no workspace: two calls give the same bits.
// The library is built with -ffp-contract=off: every product, sum, quotient and square root below is rounded once, as written
// (division and sqrtf are the correctly rounded ones). Not differentiable.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"
#include "raygen_device.h"      // Float3, BytePixels / SumPixels, pixel_ray, pixel_colour, make_rays: shared with spc.hip

namespace shacira {

namespace {

constexpr int64_t kRaygenMaxGrid = (int64_t)1 << 24;

template <bool kWhole>
__global__ void __launch_bounds__(kRaygenBlock) raygen_kernel(const float4 *__restrict__ cams, int num_views, int width, int height,
                                                              const int32_t *__restrict__ view_idx,
                                                              const int32_t *__restrict__ pixel_idx,
                                                              const float2 *__restrict__ jitter, int64_t n,
                                                              const uint8_t *__restrict__ images, int channels, int bg_black,
                                                              int word_loads, Float3 *__restrict__ origins,
                                                              Float3 *__restrict__ dirs, Float3 *__restrict__ rgb,
                                                              uint8_t *__restrict__ mask) {
    make_rays<kWhole>(cams, num_views, width, height, view_idx, pixel_idx, jitter, n, BytePixels{images, channels, word_loads},
                      bg_black, origins, dirs, rgb, mask);
}

// the same rays with colours from a mip level's sums
template <bool kWhole>
__global__ void __launch_bounds__(kRaygenBlock) raysums_kernel(const float4 *__restrict__ cams, int num_views, int width, int height,
                                                               const int32_t *__restrict__ view_idx,
                                                               const int32_t *__restrict__ pixel_idx,
                                                               const float2 *__restrict__ jitter, int64_t n,
                                                               const uint16_t *__restrict__ sums, int channels, uint32_t denom,
                                                               int bg_black, int wide, Float3 *__restrict__ origins,
                                                               Float3 *__restrict__ dirs, Float3 *__restrict__ rgb,
                                                               uint8_t *__restrict__ mask) {
    make_rays<kWhole>(cams, num_views, width, height, view_idx, pixel_idx, jitter, n, SumPixels{sums, channels, wide, denom},
                      bg_black, origins, dirs, rgb, mask);
}

}  // namespace

hipError_t raygen_dispatch(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                           const int32_t *pixel_idx, const float *jitter, int64_t n, const uint8_t *images, int channels,
                           bool bg_black, float *origins, float *dirs, float *rgb, uint8_t *mask, hipStream_t s) {
    const int64_t blocks = (n + kRaygenBlock - 1) / kRaygenBlock;
    const dim3 grid((uint32_t)(blocks < kRaygenMaxGrid ? blocks : kRaygenMaxGrid));
    const int word_loads = images && channels == 4 && (reinterpret_cast<uintptr_t>(images) & 3u) == 0;
    if (view_idx)
        hipLaunchKernelGGL(raygen_kernel<false>, grid, dim3(kRaygenBlock), 0, s, reinterpret_cast<const float4 *>(cams), num_views,
                           width, height, view_idx, pixel_idx, reinterpret_cast<const float2 *>(jitter), n, images, channels,
                           (int)bg_black, word_loads, reinterpret_cast<Float3 *>(origins), reinterpret_cast<Float3 *>(dirs),
                           reinterpret_cast<Float3 *>(rgb), mask);
    else
        hipLaunchKernelGGL(raygen_kernel<true>, grid, dim3(kRaygenBlock), 0, s, reinterpret_cast<const float4 *>(cams), num_views,
                           width, height, view_idx, pixel_idx, reinterpret_cast<const float2 *>(jitter), n, images, channels,
                           (int)bg_black, word_loads, reinterpret_cast<Float3 *>(origins), reinterpret_cast<Float3 *>(dirs),
                           reinterpret_cast<Float3 *>(rgb), mask);
    return hipGetLastError();
}

hipError_t raygen_sums_dispatch(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                                const int32_t *pixel_idx, const float *jitter, int64_t n, const uint16_t *sums, int channels,
                                int mip, bool bg_black, float *origins, float *dirs, float *rgb, uint8_t *mask, hipStream_t s) {
    const int64_t blocks = (n + kRaygenBlock - 1) / kRaygenBlock;
    const dim3 grid((uint32_t)(blocks < kRaygenMaxGrid ? blocks : kRaygenMaxGrid));
    const int wide = sums && channels == 4 && (reinterpret_cast<uintptr_t>(sums) & 7u) == 0;
    const uint32_t denom = 255u << (2 * mip);
    if (view_idx)
        hipLaunchKernelGGL(raysums_kernel<false>, grid, dim3(kRaygenBlock), 0, s, reinterpret_cast<const float4 *>(cams), num_views,
                           width, height, view_idx, pixel_idx, reinterpret_cast<const float2 *>(jitter), n, sums, channels, denom,
                           (int)bg_black, wide, reinterpret_cast<Float3 *>(origins), reinterpret_cast<Float3 *>(dirs),
                           reinterpret_cast<Float3 *>(rgb), mask);
    else
        hipLaunchKernelGGL(raysums_kernel<true>, grid, dim3(kRaygenBlock), 0, s, reinterpret_cast<const float4 *>(cams), num_views,
                           width, height, view_idx, pixel_idx, reinterpret_cast<const float2 *>(jitter), n, sums, channels, denom,
                           (int)bg_black, wide, reinterpret_cast<Float3 *>(origins), reinterpret_cast<Float3 *>(dirs),
                           reinterpret_cast<Float3 *>(rgb), mask);
    return hipGetLastError();
}

}  // namespace shacira
