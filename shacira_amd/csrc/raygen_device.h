// raygen_device.h -- the ray and the target colour of one (view, pixel) pair, shared by raygen.hip (which stores them) and spc.hip
// (which turns them into the point and the colour bytes of a depth pixel). Contract: include/shacira_hip.h, shacira_raygen. Every
// file that includes this is built with -ffp-contract=off: each product, sum, quotient and square root below is rounded once, as
// written (division and sqrtf are the correctly rounded ones). Everything is file-local (an anonymous namespace per including file).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace shacira {

namespace {

constexpr int kRaygenBlock = 256;

struct Float3 {      // 12 bytes, 4-byte aligned: stored as one dwordx3
    float x, y, z;
};

// The pixel sources. load() yields the pixel's integers (b3 = full() without an alpha channel); a colour is the correctly rounded
// (float)b / (float)full().
struct BytePixels {                                   // uint8 [V, H, W, channels]
    const uint8_t *base;
    int channels, wide;                               // wide: 4 channels on a 4-byte aligned base, one load
    __device__ __forceinline__ bool present() const { return base != nullptr; }
    __device__ __forceinline__ float full() const { return 255.0f; }
    __device__ __forceinline__ void load(int64_t pixel, uint32_t &b0, uint32_t &b1, uint32_t &b2, uint32_t &b3) const {
        const uint8_t *p = base + pixel * channels;
        b3 = 255u;
        if (wide) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
            b0 = w & 255u;
            b1 = (w >> 8) & 255u;
            b2 = (w >> 16) & 255u;
            b3 = w >> 24;
        } else {
            b0 = p[0];
            b1 = p[1];
            b2 = p[2];
            if (channels == 4) b3 = p[3];
        }
    }
};

struct SumPixels {                                    // uint16 [V, H, W, channels]: sums of 4^mip bytes each
    const uint16_t *base;
    int channels, wide;                               // wide: 4 channels on an 8-byte aligned base, one load
    uint32_t denom;                                   // 255 << (2 mip) <= 65280: exact in fp32
    __device__ __forceinline__ bool present() const { return base != nullptr; }
    __device__ __forceinline__ float full() const { return (float)denom; }
    __device__ __forceinline__ void load(int64_t pixel, uint32_t &b0, uint32_t &b1, uint32_t &b2, uint32_t &b3) const {
        const uint16_t *p = base + pixel * channels;
        b3 = denom;
        if (wide) {
            const uint2 w = *reinterpret_cast<const uint2 *>(p);
            b0 = w.x & 0xFFFFu;
            b1 = w.x >> 16;
            b2 = w.y & 0xFFFFu;
            b3 = w.y >> 16;
        } else {
            b0 = p[0];
            b1 = p[1];
            b2 = p[2];
            if (channels == 4) b3 = p[3];
        }
    }
};

// origin and unit direction of pixel `pixel` (= y * width + x) of the camera whose record is at `rec`, offset by (jx, jy)
__device__ __forceinline__ void pixel_ray(const float4 *__restrict__ rec, int64_t pixel, int width, int height, float jx, float jy,
                                          Float3 &o, Float3 &d) {
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
    // R row-major r0.x r0.y r0.z | r0.w r1.x r1.y | r1.z r1.w r2.x, t = r2.y r2.z r2.w, tan = r3.x r3.y, x0 y0 = r3.z r3.w,
    // lens = r4.x, fov_distance * aspect = r4.y, fov_distance = r4.z
    const uint32_t y = (uint32_t)pixel / (uint32_t)width, x = (uint32_t)pixel - y * (uint32_t)width;
    const bool ortho = r4.x != 0.f;
    // the orthographic lens has no principal point: its pixels are not shifted
    const float px = ortho ? ((float)x + 0.5f) + jx : (((float)x + 0.5f) + jx) - r3.z;
    const float py = ortho ? ((float)y + 0.5f) + jy : (((float)y + 0.5f) + jy) + r3.w;
    const float u = 2.0f * (px / (float)width) - 1.0f;
    const float v = 2.0f * (py / (float)height) - 1.0f;
    float dx, dy, dz;
    o = Float3{r2.y, r2.z, r2.w};
    if (ortho) {
        const float ox = u * r4.y, oy = -v * r4.z;
        o.x = (r0.x * ox + r0.y * oy) + r2.y;
        o.y = (r0.w * ox + r1.x * oy) + r2.z;
        o.z = (r1.z * ox + r1.w * oy) + r2.w;
        dx = 0.f;
        dy = 0.f;
    } else {
        dx = u * r3.x;
        dy = -v * r3.y;
    }
    dz = -1.0f;
    const float wx = (r0.x * dx + r0.y * dy) + r0.z * dz;
    const float wy = (r0.w * dx + r1.x * dy) + r1.y * dz;
    const float wz = (r1.z * dx + r1.w * dy) + r2.x * dz;
    const float norm = sqrtf((wx * wx + wy * wy) + wz * wz);
    d = Float3{wx / norm, wy / norm, wz / norm};
}

// composited colour and mask of pixel `index` (= view * H W + pixel) of `images`
template <class Pixels>
__device__ __forceinline__ void pixel_colour(const Pixels &images, int64_t index, int bg_black, Float3 &c, uint8_t &m) {
    const int channels = images.channels;
    const float full = images.full();
    uint32_t b0, b1, b2, b3;
    images.load(index, b0, b1, b2, b3);
    c = Float3{(float)b0 / full, (float)b1 / full, (float)b2 / full};
    m = 1;
    if (channels == 4) {
        const float a = (float)b3 / full;
        const float rest = 1.0f - a;
        if (bg_black) {
            c.x = c.x - rest;
            c.y = c.y - rest;
            c.z = c.z - rest;
        } else {
            c.x = c.x * a + rest;
            c.y = c.y * a + rest;
            c.z = c.z * a + rest;
        }
        c.x = fminf(fmaxf(c.x, 0.0f), 1.0f);
        c.y = fminf(fmaxf(c.y, 0.0f), 1.0f);
        c.z = fminf(fmaxf(c.z, 0.0f), 1.0f);
        m = a > 0.5f ? 1 : 0;
    }
}

// kWhole: ray i is pixel i mod HW of view i div HW; otherwise the indices come from view_idx / pixel_idx
template <bool kWhole, class Pixels>
__device__ __forceinline__ void make_rays(const float4 *__restrict__ cams, int num_views, int width, int height,
                                          const int32_t *__restrict__ view_idx, const int32_t *__restrict__ pixel_idx,
                                          const float2 *__restrict__ jitter, int64_t n, const Pixels images, int bg_black,
                                          Float3 *__restrict__ origins, Float3 *__restrict__ dirs, Float3 *__restrict__ rgb,
                                          uint8_t *__restrict__ mask) {
    const int64_t hw = (int64_t)width * height;       // < 2^31, checked by the entry point
    const float nan = __builtin_nanf("");
    for (int64_t i = (int64_t)blockIdx.x * kRaygenBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRaygenBlock) {
        int64_t view, pixel;
        if (kWhole) {
            if (n <= (int64_t)UINT32_MAX) {           // uniform: the 32-bit division is a fraction of the 64-bit one
                view = (uint32_t)i / (uint32_t)hw;
                pixel = (uint32_t)i - (uint32_t)view * (uint32_t)hw;
            } else {
                view = i / hw;
                pixel = i - view * hw;
            }
        } else {
            view = view_idx[i];
            pixel = pixel_idx[i];
        }
        if (view < 0 || view >= num_views || pixel < 0 || pixel >= hw) {      // reads nothing more
            const Float3 bad = {nan, nan, nan};
            origins[i] = bad;
            dirs[i] = bad;
            if (images.present()) {
                rgb[i] = bad;
                mask[i] = 0;
            }
            continue;
        }
        float jx = 0.f, jy = 0.f;
        if (jitter) {
            const float2 j = jitter[i];
            jx = j.x;
            jy = j.y;
        }
        Float3 o, d;
        pixel_ray(cams + view * (SHACIRA_RAYGEN_RECORD_FLOATS / 4), pixel, width, height, jx, jy, o, d);
        origins[i] = o;
        dirs[i] = d;
        if (images.present()) {
            Float3 c;
            uint8_t m;
            pixel_colour(images, view * hw + pixel, bg_black, c, m);
            rgb[i] = c;
            mask[i] = m;
        }
    }
}

}  // namespace

}  // namespace shacira
