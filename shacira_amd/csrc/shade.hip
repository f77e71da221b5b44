// shade.hip -- the offline renderer's per-pixel passes over the buffers the tracer left on the device (contracts in
// include/shacira_hip.h: shacira_shade_view, shacira_shadow_rays, shacira_shadow_apply, shacira_sdf_slice_colors). One lane
// makes one pixel, 256 lanes a workgroup:
//   shade_view    matcap / normal / rb shading, the renderer's segmentation of the missed pixels, optionally the matcap
//                 coordinates and the 8-bit colours, in one pass;
//   shadow_rays   the ground plane, the shadow ray towards the jittered point light and the two flags;
//   shadow_apply  two launches: the shadow flag, the 0.7 / 1 map and its 17-tap blur down the columns into the workspace, then the
//                 blur along the rows times rgb. The border is scipy's 'reflect', periodic, so any H, W >= 1 works;
//   slice_colors  the colour map of an SDF slice, fp32.
// Rows of three floats are read and written as one dwordx3 at base + 12 i: a wavefront covers one contiguous run of 768 bytes.
// The library is built with -ffp-contract=off: every product, sum, quotient and square root below is rounded once, as written
// (division and sqrtf are the correctly rounded ones). No LDS, no atomics: two calls give the same bits. Not differentiable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "internal.h"
#include "philox.h"

namespace shacira {

namespace {

constexpr int kShadeBlock = 256;
constexpr int64_t kShadeMaxGrid = (int64_t)1 << 24;
constexpr uint32_t kShadowStream = 0x53484457u;      // the counter's third word: mesh_sample.hip uses 0 and 1 there

struct Float3 {      // 12 bytes, 4-byte aligned: stored as one dwordx3
    float x, y, z;
};

struct Byte3 {
    uint8_t x, y, z;
};

struct Mat3 {
    float m[9];
};

struct BlurTaps {
    float w[SHACIRA_SHADOW_BLUR_RADIUS + 1];        // w[k]: the tap at distance k from the centre
};

__device__ __forceinline__ float clamp01_nan0(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }   // NaN -> 0
__device__ __forceinline__ float clip01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }         // NaN stays

__device__ __forceinline__ uint8_t level8(float c) {      // saturating truncation of c * 255; NaN -> 0
    const float v = c * 255.0f;
    return v > 0.0f ? (v < 255.0f ? (uint8_t)v : (uint8_t)255) : (uint8_t)0;
}

__global__ void __launch_bounds__(kShadeBlock) shade_view_kernel(int64_t n, int mode, Float3 *__restrict__ normal,
                                                                 const Float3 *__restrict__ dirs, const uint8_t *__restrict__ hit,
                                                                 int has_mm, const Mat3 mm, const uint8_t *__restrict__ tex, int mh,
                                                                 int mw, int mc, Float3 *__restrict__ rgb,
                                                                 float2 *__restrict__ uv_out, Byte3 *__restrict__ rgb8_out) {
    for (int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kShadeBlock) {
        Float3 c = {0.0f, 0.0f, 0.0f};
        if (mode == SHACIRA_SHADE_MATCAP) {
            const Float3 nr = normal[i], d = dirs[i];
            Float3 v = d;
            if (has_mm) {
                v.x = (d.x * mm.m[0] + d.y * mm.m[1]) + d.z * mm.m[2];
                v.y = (d.x * mm.m[3] + d.y * mm.m[4]) + d.z * mm.m[5];
                v.z = (d.x * mm.m[6] + d.y * mm.m[7]) + d.z * mm.m[8];
            }
            v.z = -v.z;
            const float dot2 = 2.0f * ((nr.x * v.x + nr.y * v.y) + nr.z * v.z);
            const float rx = v.x - dot2 * nr.x, ry = v.y - dot2 * nr.y, rz = (v.z - dot2 * nr.z) - 1.0f;
            const float m = 2.0f * sqrtf((rx * rx + ry * ry) + rz * rz);
            const float u = clamp01_nan0(1.0f - (rx / m + 0.5f));
            const float w = clamp01_nan0(1.0f - (ry / m + 0.5f));
            if (uv_out) uv_out[i] = make_float2(u, w);
            if (tex) {
                const float x = u * (float)(mw - 1), y = w * (float)(mh - 1);
                const int xf = (int)floorf(x), yf = (int)floorf(y);
                const int x0 = xf < mw - 2 ? xf : mw - 2, y0 = yf < mh - 2 ? yf : mh - 2;      // u, w in [0, 1]: x0, y0 >= 0
                const float fx = x - (float)x0, fy = y - (float)y0;
                const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
                const uint8_t *t0 = tex + ((int64_t)y0 * mw + x0) * mc, *t1 = t0 + (int64_t)mw * mc;
                float ch[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    ch[k] = (((w00 * (float)t0[k] + w10 * (float)t0[mc + k]) + w01 * (float)t1[k]) + w11 * (float)t1[mc + k]) / 255.0f;
                c = Float3{ch[0], ch[1], ch[2]};
            }
        } else if (mode == SHACIRA_SHADE_NORMAL) {
            const Float3 nr = normal[i];
            c = Float3{(nr.x + 1.0f) / 2.0f, (nr.y + 1.0f) / 2.0f, (nr.z + 1.0f) / 2.0f};
        } else {
            c = rgb[i];
        }
        if (!rgb) continue;                                // uniform: the coordinates-only form
        if (hit && !hit[i]) {
            c = Float3{1.0f, 1.0f, 1.0f};
            if (normal) normal[i] = c;
        }
        rgb[i] = c;
        if (rgb8_out) rgb8_out[i] = Byte3{level8(c.x), level8(c.y), level8(c.z)};
    }
}

__global__ void __launch_bounds__(kShadeBlock) shadow_rays_kernel(int64_t n, const Float3 *__restrict__ origins,
                                                                  const Float3 *__restrict__ dirs, Float3 light, float min_y,
                                                                  uint32_t key0, uint32_t key1, float *__restrict__ depth,
                                                                  Float3 *__restrict__ xyz, Float3 *__restrict__ normal,
                                                                  uint8_t *__restrict__ hit, Float3 *__restrict__ so_out,
                                                                  Float3 *__restrict__ sd_out, uint8_t *__restrict__ light_hit,
                                                                  uint8_t *__restrict__ plane_hit) {
    for (int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kShadeBlock) {
        const Float3 o = origins[i], d = dirs[i];
        Float3 p = xyz[i], nr = normal[i];
        const float rate = -d.y;
        const float plane_t = (o.y - min_y) / rate;
        const bool ph = plane_t > 0.0f && plane_t < 500.0f && plane_t < depth[i];       // NaN and the infinities compare false
        if (ph) {
            hit[i] = 0;
            depth[i] = plane_t;
            p = Float3{o.x + d.x * plane_t, o.y + d.y * plane_t, o.z + d.z * plane_t};
            nr = Float3{0.0f, 1.0f, 0.0f};
            xyz[i] = p;
            normal[i] = nr;
        }
        const Float3 so = {p.x + 0.01f * nr.x, p.y + 0.01f * nr.y, p.z + 0.01f * nr.z};
        uint32_t g[4];
        philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), kShadowStream, 0u, key0, key1, g);
        float z[3];
        box_muller3(g, z);
        const float x0 = (light.x + 0.01f * z[0]) - so.x, x1 = (light.y + 0.01f * z[1]) - so.y,
                    x2 = (light.z + 0.01f * z[2]) - so.z;
        const float len = sqrtf((x0 * x0 + x1 * x1) + x2 * x2);
        const float den = len > 1e-12f ? len : 1e-12f;          // a NaN length divides by 1e-12: the row stays NaN
        const Float3 sd = {x0 / den, x1 / den, x2 / den};
        so_out[i] = so;
        sd_out[i] = sd;
        light_hit[i] = ((sd.x * nr.x + sd.y * nr.y) + sd.z * nr.z) > 0.0f ? 1 : 0;
        plane_hit[i] = ph ? 1 : 0;
    }
}

// scipy's mode='reflect' (d c b a | a b c d | d c b a), periodic with period 2 n: any i, any n >= 1
__device__ __forceinline__ int reflect_periodic(int i, int n) {
    const int period = 2 * n;
    int j = i % period;
    if (j < 0) j += period;
    return j < n ? j : period - 1 - j;
}

// the shadow flag, the map 1 or 0.7 and its blur down the columns (axis 0) into tmp [H, W]
__global__ void __launch_bounds__(kShadeBlock) shadow_blur_columns_kernel(int H, int W, const uint8_t *__restrict__ occluded,
                                                                          const uint8_t *__restrict__ light_hit,
                                                                          uint8_t *__restrict__ shadow_out, const BlurTaps taps,
                                                                          float *__restrict__ tmp) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kShadeBlock) {
        const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
        auto map_at = [&](int row) {
            const int64_t j = (int64_t)reflect_periodic(row, H) * W + x;
            const float s = (occluded[j] && light_hit[j]) ? 1.0f : 0.0f;
            return fminf(fmaxf((1.0f - s) + 0.7f, 0.0f), 1.0f);
        };
        shadow_out[i] = (occluded[i] && light_hit[i]) ? 1 : 0;
        float acc = taps.w[0] * map_at(y);
#pragma unroll
        for (int k = 1; k <= SHACIRA_SHADOW_BLUR_RADIUS; ++k) acc = acc + taps.w[k] * (map_at(y - k) + map_at(y + k));
        tmp[i] = acc;
    }
}

// the blur along the rows (axis 1) of tmp, times the first three channels of rgb [H W, C]
template <int C>
__global__ void __launch_bounds__(kShadeBlock) shadow_blur_rows_kernel(int H, int W, const float *__restrict__ tmp,
                                                                       const BlurTaps taps, float *__restrict__ rgb) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kShadeBlock) {
        const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
        const float *row = tmp + (int64_t)y * W;
        float acc = taps.w[0] * row[x];
#pragma unroll
        for (int k = 1; k <= SHACIRA_SHADOW_BLUR_RADIUS; ++k)
            acc = acc + taps.w[k] * (row[reflect_periodic(x - k, W)] + row[reflect_periodic(x + k, W)]);
        if (C == 3) {
            Float3 *p = reinterpret_cast<Float3 *>(rgb) + i;
            const Float3 c = *p;
            *p = Float3{c.x * acc, c.y * acc, c.z * acc};
        } else {
            float4 *p = reinterpret_cast<float4 *>(rgb) + i;
            const float4 c = *p;
            *p = make_float4(c.x * acc, c.y * acc, c.z * acc, c.w);        // alpha: the same bits back
        }
    }
}

__global__ void __launch_bounds__(kShadeBlock) sdf_slice_colors_kernel(int64_t n, const float *__restrict__ d,
                                                                       Float3 *__restrict__ vis) {
    for (int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kShadeBlock) {
        const float dd = clip01((d[i] + 1.0f) / 2.0f);
        const float blue = clip01((dd - 0.5f) * 2.0f);
        const float yellow = 1.0f - blue;
        Float3 c = {(0.0f + yellow * 0.4f) + 0.2f, (0.0f + yellow * 0.3f) + 0.2f, (blue + yellow * 0.0f) + 0.2f};
        if (dd - 0.5f < 0.0f) c = Float3{1.0f, 0.38f, 0.0f};
        bool line = false;
#pragma unroll
        for (int k = 0; k < 50; ++k) line = line || fabsf(dd - (float)(0.02 * (double)k)) < (float)0.0015;
        if (line) c = Float3{0.8f, 0.8f, 0.8f};
        if (fabsf(dd - 0.5f) < (float)0.004) c = Float3{0.0f, 0.0f, 0.0f};
        vis[i] = c;
    }
}

dim3 shade_grid(int64_t n) {
    const int64_t blocks = (n + kShadeBlock - 1) / kShadeBlock;
    return dim3((uint32_t)(blocks < kShadeMaxGrid ? blocks : kShadeMaxGrid));
}

}  // namespace

hipError_t shade_view_dispatch(int64_t n, int mode, float *normal, const float *dirs, const uint8_t *hit, const float *mm_host,
                               const uint8_t *tex, int mh, int mw, int mc, float *rgb, float *uv_out, uint8_t *rgb8_out,
                               hipStream_t s) {
    Mat3 mm = {};
    if (mm_host)
        for (int k = 0; k < 9; ++k) mm.m[k] = mm_host[k];
    hipLaunchKernelGGL(shade_view_kernel, shade_grid(n), dim3(kShadeBlock), 0, s, n, mode, reinterpret_cast<Float3 *>(normal),
                       reinterpret_cast<const Float3 *>(dirs), hit, mm_host ? 1 : 0, mm, tex, mh, mw, mc,
                       reinterpret_cast<Float3 *>(rgb), reinterpret_cast<float2 *>(uv_out), reinterpret_cast<Byte3 *>(rgb8_out));
    return hipGetLastError();
}

hipError_t shadow_rays_dispatch(int64_t n, const float *origins, const float *dirs, const float *light_host, float min_y,
                                uint64_t seed, float *depth, float *xyz, float *normal, uint8_t *hit, float *so, float *sd,
                                uint8_t *light_hit, uint8_t *plane_hit, hipStream_t s) {
    const Float3 light = {light_host[0], light_host[1], light_host[2]};
    hipLaunchKernelGGL(shadow_rays_kernel, shade_grid(n), dim3(kShadeBlock), 0, s, n, reinterpret_cast<const Float3 *>(origins),
                       reinterpret_cast<const Float3 *>(dirs), light, min_y, (uint32_t)seed, (uint32_t)(seed >> 32), depth,
                       reinterpret_cast<Float3 *>(xyz), reinterpret_cast<Float3 *>(normal), hit, reinterpret_cast<Float3 *>(so),
                       reinterpret_cast<Float3 *>(sd), light_hit, plane_hit);
    return hipGetLastError();
}

hipError_t shadow_apply_dispatch(int64_t H, int64_t W, int C, const uint8_t *occluded, const uint8_t *light_hit,
                                 uint8_t *shadow_out, float *rgb, void *workspace, hipStream_t s) {
    // scipy.ndimage.gaussian_filter(sigma=2): radius int(4 * 2 + 0.5) = 8, exp(-x^2 / 8) over their fp64 sum, rounded to fp32
    double w[SHACIRA_SHADOW_BLUR_RADIUS + 1], sum = 0.0;
    for (int k = 0; k <= SHACIRA_SHADOW_BLUR_RADIUS; ++k) {
        w[k] = std::exp(-0.5 * (double)(k * k) / 4.0);
        sum += k ? 2.0 * w[k] : w[k];
    }
    BlurTaps taps;
    for (int k = 0; k <= SHACIRA_SHADOW_BLUR_RADIUS; ++k) taps.w[k] = (float)(w[k] / sum);
    float *tmp = static_cast<float *>(workspace);
    const dim3 grid = shade_grid(H * W), block(kShadeBlock);
    hipLaunchKernelGGL(shadow_blur_columns_kernel, grid, block, 0, s, (int)H, (int)W, occluded, light_hit, shadow_out, taps, tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (C == 3)
        hipLaunchKernelGGL(shadow_blur_rows_kernel<3>, grid, block, 0, s, (int)H, (int)W, tmp, taps, rgb);
    else
        hipLaunchKernelGGL(shadow_blur_rows_kernel<4>, grid, block, 0, s, (int)H, (int)W, tmp, taps, rgb);
    return hipGetLastError();
}

hipError_t sdf_slice_colors_dispatch(int64_t n, const float *d, float *vis, hipStream_t s) {
    hipLaunchKernelGGL(sdf_slice_colors_kernel, shade_grid(n), dim3(kShadeBlock), 0, s, n, d, reinterpret_cast<Float3 *>(vis));
    return hipGetLastError();
}

}  // namespace shacira
