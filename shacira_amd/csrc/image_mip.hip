// image_mip.hip -- one mip level of uint8 images as exact block sums (contract in include/shacira_hip.h, shacira_image_mip):
// sums[v, y, x, c] = the sum of the 2^mip x 2^mip block of images[v, :, :, c] whose corner is (y << mip, x << mip), a uint16
// (at most 255 * 4^4 = 65280 for mip <= 4). A power-of-two INTER_AREA resize is this sum over 4^mip.
//   reads    every source byte once. Lanes run along x: consecutive lanes read consecutive pieces of one source row, so a
//            wavefront's load instruction covers whole contiguous lines of that row, and the 2^mip rows of a block are 2^mip
//            independent loads in flight;
//   writes   one uint16 per channel and output pixel, lanes along x again.
// Four channels on an aligned base take the packed form: a dword is one pixel, (w & 0x00FF00FF) and ((w >> 8) & 0x00FF00FF)
// hold channels 0, 2 and 1, 3 in 16-bit halves, and two dword accumulators carry all four sums without a carry between the
// halves (65280 < 2^16). With a 16-byte aligned base a lane loads 16 bytes (8 at mip 1) per row, and at mip 3 / 4 the 32 / 64
// bytes of a block's row are shared by 2 / 4 neighbouring lanes whose partial sums meet through two cross-lane exchanges: the
// wavefront still reads 1 KiB of one row per instruction, where one lane per block would stride its 16-byte loads by 32 / 64
// bytes and touch every line two / four times. Any other channel count or base takes byte loads, one lane per output pixel.
// No workspace, no atomics, no LDS allocation: capturable, and integer sums are the same bits on every call.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace shacira {

namespace {

constexpr int kMipBlock = 256;
constexpr int64_t kMipMaxGrid = (int64_t)1 << 22;

__device__ __forceinline__ void mip_add(uint32_t w, uint32_t &lo, uint32_t &hi) {
    lo += w & 0x00FF00FFu;
    hi += (w >> 8) & 0x00FF00FFu;
}

// rows = V * (H >> mip) output rows (a view's rows follow the previous view's: the source row of output row r is r << mip in
// the [V H, W] stack), w = W >> mip. kWide: 16-byte aligned base, loads of min(16, 4 << kMip) bytes, kLanes lanes per block
template <int kMip, bool kWide>
__global__ void __launch_bounds__(kMipBlock) mip_rgba_kernel(const uint32_t *__restrict__ src, int64_t rows, int64_t w,
                                                             uint2 *__restrict__ sums) {
    constexpr int f = 1 << kMip;
    constexpr int kLanes = (kWide && f > 4) ? f / 4 : 1;       // lanes that share one block
    constexpr int kDwords = f / kLanes;                        // source pixels per lane and row
    const int64_t W = w * f;
    const int64_t total = rows * w * kLanes;
    const bool narrow = total <= (int64_t)UINT32_MAX;          // uniform: 32-bit divisions where they suffice
    for (int64_t t = (int64_t)blockIdx.x * kMipBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kMipBlock) {
        // a block's kLanes lanes are neighbours inside one wavefront (kMipBlock and the grid stride are multiples of kLanes),
        // and they enter and leave this loop together
        const int sub = (int)(t & (kLanes - 1));
        const int64_t o = t / kLanes;
        int64_t r, x;
        if (narrow) {
            r = (uint32_t)o / (uint32_t)w;
            x = (uint32_t)o - (uint32_t)r * (uint32_t)w;
        } else {
            r = o / w;
            x = o - r * w;
        }
        const uint32_t *p = src + ((r * f) * W + x * f + sub * kDwords);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int dy = 0; dy < f; ++dy, p += W) {
            if (kWide && kDwords == 2) {
                const uint2 q = *reinterpret_cast<const uint2 *>(p);
                mip_add(q.x, lo, hi);
                mip_add(q.y, lo, hi);
            } else if (kWide) {
                const uint4 q = *reinterpret_cast<const uint4 *>(p);
                mip_add(q.x, lo, hi);
                mip_add(q.y, lo, hi);
                mip_add(q.z, lo, hi);
                mip_add(q.w, lo, hi);
            } else {
#pragma unroll
                for (int dx = 0; dx < kDwords; ++dx) mip_add(p[dx], lo, hi);
            }
        }
#pragma unroll
        for (int m = 1; m < kLanes; m <<= 1) {
            lo += (uint32_t)__shfl_xor((int)lo, m);
            hi += (uint32_t)__shfl_xor((int)hi, m);
        }
        // lo = s0 | s2 << 16, hi = s1 | s3 << 16  ->  the pixel's four uint16 in order
        if (sub == 0) sums[o] = make_uint2((lo & 0xFFFFu) | (hi << 16), (lo >> 16) | (hi & 0xFFFF0000u));
    }
}

// any channel count, any alignment: one lane per output pixel, byte loads
__global__ void __launch_bounds__(kMipBlock) mip_bytes_kernel(const uint8_t *__restrict__ src, int64_t rows, int64_t w,
                                                              int channels, int mip, uint16_t *__restrict__ sums) {
    const int f = 1 << mip;
    const int64_t W = w * f;
    const int64_t total = rows * w;
    const bool narrow = total <= (int64_t)UINT32_MAX;
    for (int64_t o = (int64_t)blockIdx.x * kMipBlock + threadIdx.x; o < total; o += (int64_t)gridDim.x * kMipBlock) {
        int64_t r, x;
        if (narrow) {
            r = (uint32_t)o / (uint32_t)w;
            x = (uint32_t)o - (uint32_t)r * (uint32_t)w;
        } else {
            r = o / w;
            x = o - r * w;
        }
        const uint8_t *p = src + ((r * f) * W + x * f) * channels;
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        for (int dy = 0; dy < f; ++dy, p += W * channels) {
            const uint8_t *q = p;
            for (int dx = 0; dx < f; ++dx, q += channels) {
                s0 += q[0];
                if (channels > 1) s1 += q[1];
                if (channels > 2) s2 += q[2];
                if (channels > 3) s3 += q[3];
            }
        }
        uint16_t *out = sums + o * channels;
        out[0] = (uint16_t)s0;
        if (channels > 1) out[1] = (uint16_t)s1;
        if (channels > 2) out[2] = (uint16_t)s2;
        if (channels > 3) out[3] = (uint16_t)s3;
    }
}

template <int kMip, bool kWide>
void launch_rgba(const uint8_t *images, int64_t rows, int64_t w, uint16_t *sums, hipStream_t s) {
    constexpr int f = 1 << kMip;
    constexpr int kLanes = (kWide && f > 4) ? f / 4 : 1;
    const int64_t blocks = (rows * w * kLanes + kMipBlock - 1) / kMipBlock;
    const dim3 grid((uint32_t)(blocks < kMipMaxGrid ? blocks : kMipMaxGrid));
    hipLaunchKernelGGL((mip_rgba_kernel<kMip, kWide>), grid, dim3(kMipBlock), 0, s, reinterpret_cast<const uint32_t *>(images),
                       rows, w, reinterpret_cast<uint2 *>(sums));
}

}  // namespace

hipError_t image_mip_dispatch(const uint8_t *images, int64_t num_views, int64_t height, int64_t width, int channels, int mip,
                              uint16_t *sums, hipStream_t s) {
    const int64_t rows = num_views * (height >> mip), w = width >> mip;
    const uintptr_t src = reinterpret_cast<uintptr_t>(images), dst = reinterpret_cast<uintptr_t>(sums);
    if (channels == 4 && (src & 3u) == 0 && (dst & 7u) == 0) {
        // a row is 4 W bytes and W a multiple of 2^mip: every load is as aligned as the base is, up to 4 << mip bytes
        const bool wide = (src & 15u) == 0;
        switch (mip * 2 + (wide ? 1 : 0)) {
            case 2: launch_rgba<1, false>(images, rows, w, sums, s); break;
            case 3: launch_rgba<1, true>(images, rows, w, sums, s); break;
            case 4: launch_rgba<2, false>(images, rows, w, sums, s); break;
            case 5: launch_rgba<2, true>(images, rows, w, sums, s); break;
            case 6: launch_rgba<3, false>(images, rows, w, sums, s); break;
            case 7: launch_rgba<3, true>(images, rows, w, sums, s); break;
            case 8: launch_rgba<4, false>(images, rows, w, sums, s); break;
            default: launch_rgba<4, true>(images, rows, w, sums, s); break;
        }
    } else {
        const int64_t blocks = (rows * w + kMipBlock - 1) / kMipBlock;
        const dim3 grid((uint32_t)(blocks < kMipMaxGrid ? blocks : kMipMaxGrid));
        hipLaunchKernelGGL(mip_bytes_kernel, grid, dim3(kMipBlock), 0, s, images, rows, w, channels, mip, sums);
    }
    return hipGetLastError();
}

}  // namespace shacira
