// pixels.hip -- training batches and the image loss straight from the uint8 image on the device (contracts in
// include/shacira_hip.h, shacira_pixel_batch / shacira_pixel_loss_forward / shacira_pixel_loss_backward). One lane makes one pixel:
//   batch    reads its pixel index (or derives it from the row number in the range form) and the pixel's 3 bytes, writes two
//            floats of coordinates and three of colour. Lane i stores at base + 8 i and base + 12 i, so a wavefront's 64 lanes
//            cover one contiguous run per output, whatever the order of the indices. No LDS, no atomics, no workspace.
//   loss     reads its prediction row (12 bytes) and the pixel's 3 bytes; keeps the fp64 sum of squared fp32 differences, the
//            integer sum of squared 8-bit level differences and the count of pixels in registers over the grid-stride loop,
//            adds them over the wavefront by shuffles and over the four wavefronts in order, and writes ONE partial triple per
//            workgroup. The finish kernel (one workgroup) adds the partials in a fixed order. No floating-point atomics: two
//            calls give the same bits.
//   grad     the same reads, writes g * (2 d) as 12-byte rows.
// The library is built with -ffp-contract=off: every difference, product and quotient below is rounded once, as written (the
// divisions are the correctly rounded ones). All byte offsets into the image are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace shacira {

namespace {

constexpr int kPixelBlock = 256;
constexpr int64_t kPixelMaxGrid = SHACIRA_PIXEL_MAX_GRID;      // one resident wave of workgroups; the loops stride beyond it
constexpr int kPixelFinishBlock = 256;

struct Float3 {      // 12 bytes, 4-byte aligned: loaded and stored as one dwordx3
    float x, y, z;
};

struct PixelPartial {      // one workgroup's sums, 24 bytes
    double sq;             // sum of (double)d * (double)d
    uint64_t lvl;          // sum of (level - byte)^2, exact
    uint64_t count;        // pixels that counted
};
static_assert(sizeof(PixelPartial) == SHACIRA_PIXEL_PARTIAL_BYTES, "the workspace is sized by the header's constant");

// kIdx: 0 the range form (pixel i is start + i), 32 / 64 the width of the indices
template <int kIdx>
__device__ __forceinline__ int64_t pixel_of(const void *__restrict__ pixel_idx, int64_t start, int64_t i) {
    if (kIdx == 32) return static_cast<const int32_t *>(pixel_idx)[i];
    if (kIdx == 64) return static_cast<const int64_t *>(pixel_idx)[i];
    return start + i;
}

template <int kIdx>
__global__ void __launch_bounds__(kPixelBlock) pixel_batch_kernel(const uint8_t *__restrict__ image, int64_t height,
                                                                  int64_t width, const void *__restrict__ pixel_idx,
                                                                  int64_t start, int64_t n, float2 *__restrict__ coords,
                                                                  Float3 *__restrict__ rgb) {
    const int64_t hw = height * width;
    const float nan = __builtin_nanf("");
    for (int64_t i = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPixelBlock) {
        const int64_t p = pixel_of<kIdx>(pixel_idx, start, i);
        if (p < 0 || p >= hw) {                       // reads nothing more
            if (coords) coords[i] = make_float2(nan, nan);
            if (rgb) rgb[i] = Float3{nan, nan, nan};
            continue;
        }
        if (coords) {
            float fy, fx;
            if (hw <= (int64_t)UINT32_MAX) {          // uniform: the 32-bit division is a fraction of the 64-bit one
                const uint32_t y = (uint32_t)p / (uint32_t)width, x = (uint32_t)p - y * (uint32_t)width;
                fy = (float)y;
                fx = (float)x;
            } else {
                const int64_t y = p / width, x = p - y * width;
                fy = (float)y;
                fx = (float)x;
            }
            coords[i] = make_float2((fy / (float)height - 0.5f) * 2.0f, (fx / (float)width - 0.5f) * 2.0f);
        }
        if (rgb) {
            const uint8_t *b = image + p * 3;
            rgb[i] = Float3{(float)b[0] / 255.0f, (float)b[1] / 255.0f, (float)b[2] / 255.0f};
        }
    }
}

// the 8-bit level of a prediction: clamp to [0, 1], times 255, truncated. The comparisons send NaN to 0
__device__ __forceinline__ uint32_t pixel_level(float v) {
    float c = v > 0.0f ? v : 0.0f;
    c = c < 1.0f ? c : 1.0f;
    return (uint32_t)(c * 255.0f);
}

template <int kIdx>
__global__ void __launch_bounds__(kPixelBlock) pixel_loss_kernel(const float *__restrict__ pred, int64_t pred_stride,
                                                                 const uint8_t *__restrict__ image, int64_t hw,
                                                                 const void *__restrict__ pixel_idx, int64_t start, int64_t n,
                                                                 uint8_t *__restrict__ out_image,
                                                                 PixelPartial *__restrict__ partials) {
    double sq = 0.0;
    uint64_t lvl = 0, count = 0;
    for (int64_t i = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPixelBlock) {
        const int64_t p = pixel_of<kIdx>(pixel_idx, start, i);
        if (p < 0 || p >= hw) continue;               // skipped and not counted
        const Float3 v = *reinterpret_cast<const Float3 *>(pred + i * pred_stride);
        const uint8_t *b = image + p * 3;
        const uint32_t b0 = b[0], b1 = b[1], b2 = b[2];
        const float d0 = v.x - (float)b0 / 255.0f, d1 = v.y - (float)b1 / 255.0f, d2 = v.z - (float)b2 / 255.0f;
        sq += (double)d0 * (double)d0;
        sq += (double)d1 * (double)d1;
        sq += (double)d2 * (double)d2;
        const uint32_t l0 = pixel_level(v.x), l1 = pixel_level(v.y), l2 = pixel_level(v.z);
        const int32_t e0 = (int32_t)l0 - (int32_t)b0, e1 = (int32_t)l1 - (int32_t)b1, e2 = (int32_t)l2 - (int32_t)b2;
        lvl += (uint64_t)(uint32_t)(e0 * e0 + e1 * e1 + e2 * e2);
        count += 1;
        if (out_image) {
            uint8_t *o = out_image + p * 3;
            o[0] = (uint8_t)l0;
            o[1] = (uint8_t)l1;
            o[2] = (uint8_t)l2;
        }
    }
    // every lane of every wavefront arrives here: the loop has no early return
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sq += __shfl_down(sq, d);
        lvl += (uint64_t)__shfl_down((unsigned long long)lvl, d);
        count += (uint64_t)__shfl_down((unsigned long long)count, d);
    }
    __shared__ PixelPartial swave[kPixelBlock / 64];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0) swave[wave] = PixelPartial{sq, lvl, count};
    __syncthreads();
    if (threadIdx.x == 0) {
        PixelPartial t = swave[0];
        for (int w = 1; w < kPixelBlock / 64; ++w) {
            t.sq += swave[w].sq;
            t.lvl += swave[w].lvl;
            t.count += swave[w].count;
        }
        partials[blockIdx.x] = t;
    }
}

// stats[0 .. 2] = the sums of the `blocks` partials: thread t adds partials t, t + 256, ... in that order, the 256 sums meet in a
// binary tree: a fixed order
__global__ void __launch_bounds__(kPixelFinishBlock) pixel_loss_finish_kernel(const PixelPartial *__restrict__ partials,
                                                                              int blocks, double *__restrict__ stats) {
    __shared__ PixelPartial part[kPixelFinishBlock];
    PixelPartial t = {0.0, 0, 0};
    for (int i = (int)threadIdx.x; i < blocks; i += kPixelFinishBlock) {
        t.sq += partials[i].sq;
        t.lvl += partials[i].lvl;
        t.count += partials[i].count;
    }
    part[threadIdx.x] = t;
    __syncthreads();
    for (int d = kPixelFinishBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            part[threadIdx.x].sq += part[threadIdx.x + d].sq;
            part[threadIdx.x].lvl += part[threadIdx.x + d].lvl;
            part[threadIdx.x].count += part[threadIdx.x + d].count;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = part[0].sq;
        stats[1] = (double)part[0].lvl;
        stats[2] = (double)part[0].count;
    }
}

template <int kIdx>
__global__ void __launch_bounds__(kPixelBlock) pixel_grad_kernel(const float *__restrict__ pred, int64_t pred_stride,
                                                                 const uint8_t *__restrict__ image, int64_t hw,
                                                                 const void *__restrict__ pixel_idx, int64_t start, int64_t n,
                                                                 const float *__restrict__ grad,
                                                                 Float3 *__restrict__ grad_pred) {
    const float g = grad[0];
    for (int64_t i = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPixelBlock) {
        const int64_t p = pixel_of<kIdx>(pixel_idx, start, i);
        if (p < 0 || p >= hw) {
            grad_pred[i] = Float3{0.0f, 0.0f, 0.0f};
            continue;
        }
        const Float3 v = *reinterpret_cast<const Float3 *>(pred + i * pred_stride);
        const uint8_t *b = image + p * 3;
        const float d0 = v.x - (float)b[0] / 255.0f, d1 = v.y - (float)b[1] / 255.0f, d2 = v.z - (float)b[2] / 255.0f;
        grad_pred[i] = Float3{g * (2.0f * d0), g * (2.0f * d1), g * (2.0f * d2)};
    }
}

int64_t pixel_blocks(int64_t n) {
    const int64_t blocks = (n + kPixelBlock - 1) / kPixelBlock;
    return blocks < kPixelMaxGrid ? blocks : kPixelMaxGrid;
}

}  // namespace

size_t pixel_loss_workspace(int64_t n) { return n > 0 ? (size_t)pixel_blocks(n) * sizeof(PixelPartial) : 0; }

hipError_t pixel_batch_dispatch(const uint8_t *image, int64_t height, int64_t width, const void *pixel_idx, int idx_bits,
                                int64_t start, int64_t n, float *coords, float *rgb, hipStream_t s) {
    const dim3 grid((uint32_t)pixel_blocks(n)), block(kPixelBlock);
    float2 *c = reinterpret_cast<float2 *>(coords);
    Float3 *r = reinterpret_cast<Float3 *>(rgb);
    if (!pixel_idx)
        hipLaunchKernelGGL(pixel_batch_kernel<0>, grid, block, 0, s, image, height, width, pixel_idx, start, n, c, r);
    else if (idx_bits == 32)
        hipLaunchKernelGGL(pixel_batch_kernel<32>, grid, block, 0, s, image, height, width, pixel_idx, start, n, c, r);
    else
        hipLaunchKernelGGL(pixel_batch_kernel<64>, grid, block, 0, s, image, height, width, pixel_idx, start, n, c, r);
    return hipGetLastError();
}

hipError_t pixel_loss_forward_dispatch(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height,
                                       int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n,
                                       uint8_t *out_image, double *stats, void *workspace, hipStream_t s) {
    const int64_t blocks = pixel_blocks(n), hw = height * width;
    const dim3 grid((uint32_t)blocks), block(kPixelBlock);
    PixelPartial *partials = static_cast<PixelPartial *>(workspace);
    if (!pixel_idx)
        hipLaunchKernelGGL(pixel_loss_kernel<0>, grid, block, 0, s, pred, pred_stride, image, hw, pixel_idx, start, n, out_image,
                           partials);
    else if (idx_bits == 32)
        hipLaunchKernelGGL(pixel_loss_kernel<32>, grid, block, 0, s, pred, pred_stride, image, hw, pixel_idx, start, n,
                           out_image, partials);
    else
        hipLaunchKernelGGL(pixel_loss_kernel<64>, grid, block, 0, s, pred, pred_stride, image, hw, pixel_idx, start, n,
                           out_image, partials);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(pixel_loss_finish_kernel, dim3(1), dim3(kPixelFinishBlock), 0, s, partials, (int)blocks, stats);
    return hipGetLastError();
}

hipError_t pixel_loss_backward_dispatch(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height,
                                        int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n,
                                        const float *grad, float *grad_pred, hipStream_t s) {
    const int64_t hw = height * width;
    const dim3 grid((uint32_t)pixel_blocks(n)), block(kPixelBlock);
    Float3 *g = reinterpret_cast<Float3 *>(grad_pred);
    if (!pixel_idx)
        hipLaunchKernelGGL(pixel_grad_kernel<0>, grid, block, 0, s, pred, pred_stride, image, hw, pixel_idx, start, n, grad, g);
    else if (idx_bits == 32)
        hipLaunchKernelGGL(pixel_grad_kernel<32>, grid, block, 0, s, pred, pred_stride, image, hw, pixel_idx, start, n, grad, g);
    else
        hipLaunchKernelGGL(pixel_grad_kernel<64>, grid, block, 0, s, pred, pred_stride, image, hw, pixel_idx, start, n, grad, g);
    return hipGetLastError();
}

}  // namespace shacira
