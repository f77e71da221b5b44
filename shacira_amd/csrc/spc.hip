// spc.hip -- coloured structured point clouds (SPC) from depth images or point clouds, and their first-hit tracer; contracts in
// include/shacira_hip.h ("Structured point clouds"). An SPC of level L (G = 2^L) is three device arrays: `words`, the packed
// occupancy (cell (x, y, z) is bit key & 31 of word key >> 5, key = (x G + y) G + z), `rank`, the exclusive prefix of the words'
// popcounts, and `colors`, RGBA bytes by slot = rank[key >> 5] + popc(words[key >> 5] & ((1 << (key & 31)) - 1)).
//   depthcloud_bounds    min / max per axis and the count of the points of all valid (finite-depth) pixels: lanes keep their own
//                        six extremes as ordered integers, a wavefront folds them with shuffles and issues six integer atomics --
//                        min and max do not depend on the order, so the result is deterministic.
//   depthcloud_points    the compacted cloud in (view, pixel) order by mesh_sample.hip's count-then-write idiom: a workgroup owns
//                        256 consecutive pixels, the rank inside it comes from the wavefront's ballot and a four-entry LDS prefix.
//   spc_mark             ORs the occupancy bit of every point's cell; spc_accumulate adds (R, G, B, 1) to the cell's slot with
//                        64-bit integer atomics (exact, so order-independent). Both are ONE template over the source of the
//                        points: an fp32 cloud, or (camera records, depth plane, images) -- the cloud is then never materialised.
//   spc_popcount, spc_resolve    the popcount per word (the caller scans it into `rank`) and the rounded integer mean per slot.
//   spc_first_hit        one lane per ray: the walk of grid_walk.h (shared with render.hip) stopped at the first set bit of `words`.
// The point of a pixel is o + d * depth with raygen's origin and unit direction (raygen_device.h), two roundings per axis; the
// library is built with -ffp-contract=off, so no product is fused into the sum. All address arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_walk.h"
#include "internal.h"
#include "raygen_device.h"

namespace shacira {

namespace {

constexpr int kSpcBlock = 256;
constexpr int64_t kSpcMaxGrid = 1 << 16;      // grid-stride kernels: enough workgroups to fill the device many times over
static_assert(kSpcBlock == 256, "four wavefronts: the LDS prefix has four entries");

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// a float's bits as an unsigned integer of the same order (-inf lowest, +inf highest below the NaNs), and back
__device__ __forceinline__ uint32_t ordered(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// ---- the sources of points ------------------------------------------------------------------------------------------------------
struct CloudSource {                                  // points fp32 [n, 3], colour bytes uint8 [n, 3] (or NULL)
    const Float3 *points;
    const uint8_t *rgb;
    __device__ __forceinline__ bool point(int64_t i, Float3 &p) const {
        p = points[i];
        return true;
    }
    __device__ __forceinline__ void colour(int64_t i, uint32_t &r, uint32_t &g, uint32_t &b) const {
        const uint8_t *c = rgb + i * 3;
        r = c[0];
        g = c[1];
        b = c[2];
    }
};

template <class Pixels>
struct DepthSource {                                  // pixel i of the [V, H, W] planes, i = view * H W + pixel
    const float4 *cams;
    const float *depth;
    Pixels images;
    int width, height, bg_black;
    uint32_t hw;                                      // H W < 2^31, checked by the entry point
    int wide_index;                                   // V H W > 2^32 - 1: the index needs the 64-bit division
    // false for an invalid pixel (depth not finite), which reads nothing but its depth
    __device__ __forceinline__ bool point(int64_t i, Float3 &p) const {
        const float dep = depth[i];
        if (!finite_bits(dep)) return false;
        int64_t view, pixel;
        if (!wide_index) {                            // uniform: the 32-bit division is a fraction of the 64-bit one
            view = (uint32_t)i / hw;
            pixel = (uint32_t)i - (uint32_t)view * hw;
        } else {
            view = i / (int64_t)hw;
            pixel = i - view * (int64_t)hw;
        }
        Float3 o, d;
        pixel_ray(cams + view * (SHACIRA_RAYGEN_RECORD_FLOATS / 4), pixel, width, height, 0.f, 0.f, o, d);
        const float sx = d.x * dep, sy = d.y * dep, sz = d.z * dep;
        p = Float3{o.x + sx, o.y + sy, o.z + sz};
        return true;
    }
    __device__ __forceinline__ void colour(int64_t i, uint32_t &r, uint32_t &g, uint32_t &b) const {
        Float3 c;
        uint8_t m;
        pixel_colour(images, i, bg_black, c, m);
        r = (uint32_t)rintf(255.0f * c.x);            // c in [0, 1]
        g = (uint32_t)rintf(255.0f * c.y);
        b = (uint32_t)rintf(255.0f * c.z);
    }
};

template <class Pixels>
DepthSource<Pixels> depth_source(const DepthArgs &a, const Pixels &images) {
    const int64_t hw = (int64_t)a.width * a.height;
    return DepthSource<Pixels>{reinterpret_cast<const float4 *>(a.cams), a.depth, images, a.width, a.height, a.bg_black,
                               (uint32_t)hw, a.num_views * hw > (int64_t)UINT32_MAX};
}
BytePixels byte_pixels(const DepthArgs &a) {
    const uint8_t *base = a.mip == 0 ? static_cast<const uint8_t *>(a.images) : nullptr;
    return BytePixels{base, a.channels, base && a.channels == 4 && (reinterpret_cast<uintptr_t>(base) & 3u) == 0};
}
SumPixels sum_pixels(const DepthArgs &a) {
    const uint16_t *base = static_cast<const uint16_t *>(a.images);
    return SumPixels{base, a.channels, base && a.channels == 4 && (reinterpret_cast<uintptr_t>(base) & 7u) == 0,
                     255u << (2 * a.mip)};
}

// the cell of a point (OctreeAS.quantize_pointcloud): false when a coordinate's cell is not finite, else clamped into the grid
__device__ __forceinline__ bool cell_key(const Float3 &p, int G, uint32_t &key) {
    const float fg = (float)G;
    float cx = floorf((p.x + 1.0f) * 0.5f * fg), cy = floorf((p.y + 1.0f) * 0.5f * fg), cz = floorf((p.z + 1.0f) * 0.5f * fg);
    if (!finite_bits(cx) || !finite_bits(cy) || !finite_bits(cz)) return false;
    cx = fminf(fmaxf(cx, 0.0f), fg - 1.0f);
    cy = fminf(fmaxf(cy, 0.0f), fg - 1.0f);
    cz = fminf(fmaxf(cz, 0.0f), fg - 1.0f);
    key = ((uint32_t)cx * (uint32_t)G + (uint32_t)cy) * (uint32_t)G + (uint32_t)cz;      // < 2^30
    return true;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t n = (uint32_t)__shfl_xor((int)v, off, 64);
        v = n < v ? n : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t n = (uint32_t)__shfl_xor((int)v, off, 64);
        v = n > v ? n : v;
    }
    return v;
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------------
// bounds holds ordered integers between the first and the last of the three launches
__global__ void depthcloud_bounds_init_kernel(uint32_t *__restrict__ bounds, unsigned long long *__restrict__ count) {
    const int k = threadIdx.x;
    if (k < 3) bounds[k] = 0xFF800000u;               // ordered(+inf)
    else if (k < 6) bounds[k] = 0x007FFFFFu;          // ordered(-inf)
    else if (k == 6) *count = 0ull;
}

__global__ void __launch_bounds__(kSpcBlock) depthcloud_bounds_kernel(const DepthSource<BytePixels> src, int64_t n,
                                                                      uint32_t *__restrict__ bounds,
                                                                      unsigned long long *__restrict__ count) {
    uint32_t lo0 = 0xFF800000u, lo1 = lo0, lo2 = lo0, hi0 = 0x007FFFFFu, hi1 = hi0, hi2 = hi0;
    uint32_t valid = 0;
    for (int64_t i = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSpcBlock) {
        Float3 p;
        if (!src.point(i, p)) continue;
        const uint32_t x = ordered(p.x), y = ordered(p.y), z = ordered(p.z);
        lo0 = x < lo0 ? x : lo0;
        lo1 = y < lo1 ? y : lo1;
        lo2 = z < lo2 ? z : lo2;
        hi0 = x > hi0 ? x : hi0;
        hi1 = y > hi1 ? y : hi1;
        hi2 = z > hi2 ? z : hi2;
        ++valid;
    }
    // every lane of the wavefront arrives here
    lo0 = wave_min(lo0), lo1 = wave_min(lo1), lo2 = wave_min(lo2);
    hi0 = wave_max(hi0), hi1 = wave_max(hi1), hi2 = wave_max(hi2);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) valid += (uint32_t)__shfl_xor((int)valid, off, 64);
    if ((threadIdx.x & 63) == 0 && valid > 0) {
        atomicMin(bounds + 0, lo0);
        atomicMin(bounds + 1, lo1);
        atomicMin(bounds + 2, lo2);
        atomicMax(bounds + 3, hi0);
        atomicMax(bounds + 4, hi1);
        atomicMax(bounds + 5, hi2);
        atomicAdd(count, (unsigned long long)valid);
    }
}

__global__ void depthcloud_bounds_final_kernel(uint32_t *__restrict__ bounds) {
    const int k = threadIdx.x;
    if (k < 6) bounds[k] = __float_as_uint(unordered(bounds[k]));
}

// ---- the compacted cloud --------------------------------------------------------------------------------------------------------
// kCount: write the number of valid pixels among the workgroup's 256, and nothing else
template <bool kCount, class Pixels>
__global__ void __launch_bounds__(kSpcBlock) depthcloud_points_kernel(const DepthSource<Pixels> src, int64_t n,
                                                                      int32_t *__restrict__ block_counts,
                                                                      const int64_t *__restrict__ block_offsets,
                                                                      Float3 *__restrict__ points, uint8_t *__restrict__ rgb) {
    __shared__ int32_t wave_kept[kSpcBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x;
    Float3 p = {0.f, 0.f, 0.f};
    bool keep = false;
    if (i < n) {
        if (kCount)
            keep = finite_bits(src.depth[i]);
        else
            keep = src.point(i, p);
    }
    // every lane of every wavefront arrives here
    const uint64_t kept = __ballot(keep);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0) wave_kept[wave] = __popcll(kept);
    __syncthreads();
    if (kCount) {
        if (threadIdx.x == 0) block_counts[blockIdx.x] = (wave_kept[0] + wave_kept[1]) + (wave_kept[2] + wave_kept[3]);
        return;
    }
    if (!keep) return;
    int64_t row = block_offsets[blockIdx.x];
    for (int v = 0; v < wave; ++v) row += wave_kept[v];
    row += __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
    points[row] = p;
    if (rgb) {
        uint32_t r, g, b;
        src.colour(i, r, g, b);
        uint8_t *c = rgb + row * 3;
        c[0] = (uint8_t)r;
        c[1] = (uint8_t)g;
        c[2] = (uint8_t)b;
    }
}

// ---- occupancy, slots, colours --------------------------------------------------------------------------------------------------
template <class Source>
__global__ void __launch_bounds__(kSpcBlock) spc_mark_kernel(const Source src, int64_t n, int G, uint32_t *__restrict__ words) {
    for (int64_t i = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSpcBlock) {
        Float3 p;
        uint32_t key;
        if (!src.point(i, p) || !cell_key(p, G, key)) continue;
        const uint32_t bit = 1u << (key & 31u);
        if (!(words[key >> 5] & bit)) atomicOr(words + (key >> 5), bit);      // most points land in a cell already marked
    }
}

template <class Source>
__global__ void __launch_bounds__(kSpcBlock) spc_accumulate_kernel(const Source src, int64_t n, int G,
                                                                   const uint32_t *__restrict__ words,
                                                                   const int32_t *__restrict__ rank, int64_t cells,
                                                                   unsigned long long *__restrict__ sums) {
    for (int64_t i = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSpcBlock) {
        Float3 p;
        uint32_t key;
        if (!src.point(i, p) || !cell_key(p, G, key)) continue;
        const uint32_t w = words[key >> 5], bit = 1u << (key & 31u);
        if (!(w & bit)) continue;                     // not a cell of this SPC: nothing to add to
        const int64_t slot = (int64_t)rank[key >> 5] + __popc(w & (bit - 1u));
        if (slot < 0 || slot >= cells) continue;      // `rank` is not the prefix of `words`: write nothing out of bounds
        uint32_t r, g, b;
        src.colour(i, r, g, b);
        unsigned long long *s = sums + slot * 4;
        atomicAdd(s + 0, (unsigned long long)r);
        atomicAdd(s + 1, (unsigned long long)g);
        atomicAdd(s + 2, (unsigned long long)b);
        atomicAdd(s + 3, 1ull);
    }
}

__global__ void __launch_bounds__(kSpcBlock) spc_popcount_kernel(int64_t num_words, const uint32_t *__restrict__ words,
                                                                 int32_t *__restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x; i < num_words; i += (int64_t)gridDim.x * kSpcBlock)
        counts[i] = __popc(words[i]);
}

__global__ void __launch_bounds__(kSpcBlock) spc_resolve_kernel(int64_t cells, const unsigned long long *__restrict__ sums,
                                                                uint32_t *__restrict__ colors) {
    for (int64_t i = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kSpcBlock) {
        const unsigned long long *s = sums + i * 4;
        const unsigned long long n = s[3];
        uint32_t c = 0xFF000000u;                     // A = 255; a slot nothing was added to stays black
        if (n > 0) {
            const unsigned long long r = (2ull * s[0] + n) / (2ull * n), g = (2ull * s[1] + n) / (2ull * n),
                                     b = (2ull * s[2] + n) / (2ull * n);
            c |= (uint32_t)(r & 255ull) | ((uint32_t)(g & 255ull) << 8) | ((uint32_t)(b & 255ull) << 16);
        }
        colors[i] = c;
    }
}

// ---- first hit ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSpcBlock) spc_first_hit_kernel(int64_t num_rays, const Float3 *__restrict__ origins,
                                                                  const Float3 *__restrict__ dirs, int level,
                                                                  const uint32_t *__restrict__ words,
                                                                  const int32_t *__restrict__ rank,
                                                                  const uint32_t *__restrict__ colors,
                                                                  float *__restrict__ depth, uint8_t *__restrict__ hit,
                                                                  int32_t *__restrict__ pidx, Float3 *__restrict__ rgb) {
    const int64_t r = (int64_t)blockIdx.x * kSpcBlock + threadIdx.x;
    if (r >= num_rays) return;
    const int G = 1 << level;
    const Float3 o = origins[r], d = dirs[r];
    float out_depth = 0.0f;
    int32_t out_pidx = -1;
    uint32_t out_key = 0;
    bool found = false;
    const bool finite = finite_bits(o.x) && finite_bits(o.y) && finite_bits(o.z) && finite_bits(d.x) && finite_bits(d.y) &&
                        finite_bits(d.z);
    if (finite)                                       // a ray that is not finite is a miss by contract
        grid_walk(o.x, o.y, o.z, d.x, d.y, d.z, level, [&](int cx, int cy, int cz, float t, float) {
            const uint32_t key = ((uint32_t)cx * (uint32_t)G + (uint32_t)cy) * (uint32_t)G + (uint32_t)cz;
            if (!((words[key >> 5] >> (key & 31u)) & 1u)) return false;
            found = true;
            out_depth = t;
            out_key = key;
            out_pidx = (int32_t)morton_x_major((uint32_t)cx, (uint32_t)cy, (uint32_t)cz, level);
            return true;
        });
    depth[r] = out_depth;
    hit[r] = found ? 1 : 0;
    pidx[r] = out_pidx;
    if (colors) {
        Float3 c = {0.0f, 0.0f, 0.0f};
        if (found) {
            const uint32_t w = words[out_key >> 5];
            const int64_t slot = (int64_t)rank[out_key >> 5] + __popc(w & ((1u << (out_key & 31u)) - 1u));
            const uint32_t q = colors[slot];
            c = Float3{(float)(q & 255u) / 255.0f, (float)((q >> 8) & 255u) / 255.0f, (float)((q >> 16) & 255u) / 255.0f};
        }
        rgb[r] = c;
    }
}

inline dim3 stride_grid(int64_t n) {
    const int64_t blocks = (n + kSpcBlock - 1) / kSpcBlock;
    return dim3((uint32_t)(blocks < kSpcMaxGrid ? blocks : kSpcMaxGrid));
}

}  // namespace

hipError_t depth_bounds_dispatch(const DepthArgs &a, float *bounds, int64_t *count, hipStream_t s) {
    uint32_t *b = reinterpret_cast<uint32_t *>(bounds);
    unsigned long long *c = reinterpret_cast<unsigned long long *>(count);
    const int64_t n = (int64_t)a.num_views * a.width * a.height;
    hipLaunchKernelGGL(depthcloud_bounds_init_kernel, dim3(1), dim3(64), 0, s, b, c);
    hipLaunchKernelGGL(depthcloud_bounds_kernel, stride_grid(n), dim3(kSpcBlock), 0, s,
                       depth_source(a, BytePixels{nullptr, 3, 0}), n, b, c);
    hipLaunchKernelGGL(depthcloud_bounds_final_kernel, dim3(1), dim3(64), 0, s, b);
    return hipGetLastError();
}

hipError_t depth_points_dispatch(bool count, const DepthArgs &a, int32_t *block_counts, const int64_t *block_offsets,
                                 float *points, uint8_t *rgb, hipStream_t s) {
    const int64_t n = (int64_t)a.num_views * a.width * a.height;
    const dim3 grid((uint32_t)((n + kSpcBlock - 1) / kSpcBlock)), block(kSpcBlock);
    Float3 *p = reinterpret_cast<Float3 *>(points);
    if (count)
        hipLaunchKernelGGL((depthcloud_points_kernel<true, BytePixels>), grid, block, 0, s,
                           depth_source(a, BytePixels{nullptr, 3, 0}), n, block_counts, block_offsets, p, rgb);
    else if (a.mip == 0)
        hipLaunchKernelGGL((depthcloud_points_kernel<false, BytePixels>), grid, block, 0, s, depth_source(a, byte_pixels(a)), n,
                           block_counts, block_offsets, p, rgb);
    else
        hipLaunchKernelGGL((depthcloud_points_kernel<false, SumPixels>), grid, block, 0, s, depth_source(a, sum_pixels(a)), n,
                           block_counts, block_offsets, p, rgb);
    return hipGetLastError();
}

hipError_t spc_mark_points_dispatch(int64_t n, const float *points, int level, uint32_t *words, hipStream_t s) {
    hipLaunchKernelGGL(spc_mark_kernel<CloudSource>, stride_grid(n), dim3(kSpcBlock), 0, s,
                       CloudSource{reinterpret_cast<const Float3 *>(points), nullptr}, n, 1 << level, words);
    return hipGetLastError();
}

hipError_t spc_mark_depth_dispatch(const DepthArgs &a, int level, uint32_t *words, hipStream_t s) {
    const int64_t n = (int64_t)a.num_views * a.width * a.height;
    hipLaunchKernelGGL(spc_mark_kernel<DepthSource<BytePixels>>, stride_grid(n), dim3(kSpcBlock), 0, s,
                       depth_source(a, BytePixels{nullptr, 3, 0}), n, 1 << level, words);
    return hipGetLastError();
}

hipError_t spc_popcount_dispatch(int64_t num_words, const uint32_t *words, int32_t *counts, hipStream_t s) {
    hipLaunchKernelGGL(spc_popcount_kernel, stride_grid(num_words), dim3(kSpcBlock), 0, s, num_words, words, counts);
    return hipGetLastError();
}

hipError_t spc_accumulate_points_dispatch(int64_t n, const float *points, const uint8_t *rgb, int level, const uint32_t *words,
                                          const int32_t *rank, int64_t cells, uint64_t *sums, hipStream_t s) {
    hipLaunchKernelGGL(spc_accumulate_kernel<CloudSource>, stride_grid(n), dim3(kSpcBlock), 0, s,
                       CloudSource{reinterpret_cast<const Float3 *>(points), rgb}, n, 1 << level, words, rank, cells,
                       reinterpret_cast<unsigned long long *>(sums));
    return hipGetLastError();
}

hipError_t spc_accumulate_depth_dispatch(const DepthArgs &a, int level, const uint32_t *words, const int32_t *rank, int64_t cells,
                                         uint64_t *sums, hipStream_t s) {
    const int64_t n = (int64_t)a.num_views * a.width * a.height;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(sums);
    if (a.mip == 0)
        hipLaunchKernelGGL(spc_accumulate_kernel<DepthSource<BytePixels>>, stride_grid(n), dim3(kSpcBlock), 0, s,
                           depth_source(a, byte_pixels(a)), n, 1 << level, words, rank, cells, out);
    else
        hipLaunchKernelGGL(spc_accumulate_kernel<DepthSource<SumPixels>>, stride_grid(n), dim3(kSpcBlock), 0, s,
                           depth_source(a, sum_pixels(a)), n, 1 << level, words, rank, cells, out);
    return hipGetLastError();
}

hipError_t spc_resolve_dispatch(int64_t cells, const uint64_t *sums, uint8_t *colors, hipStream_t s) {
    hipLaunchKernelGGL(spc_resolve_kernel, stride_grid(cells), dim3(kSpcBlock), 0, s, cells,
                       reinterpret_cast<const unsigned long long *>(sums), reinterpret_cast<uint32_t *>(colors));
    return hipGetLastError();
}

hipError_t spc_first_hit_dispatch(int64_t num_rays, const float *origins, const float *dirs, int level, const uint32_t *words,
                                  const int32_t *rank, const uint8_t *colors, float *depth, uint8_t *hit, int32_t *pidx,
                                  float *rgb, hipStream_t s) {
    const dim3 grid((uint32_t)((num_rays + kSpcBlock - 1) / kSpcBlock)), block(kSpcBlock);
    hipLaunchKernelGGL(spc_first_hit_kernel, grid, block, 0, s, num_rays, reinterpret_cast<const Float3 *>(origins),
                       reinterpret_cast<const Float3 *>(dirs), level, words, rank, reinterpret_cast<const uint32_t *>(colors),
                       depth, hit, pidx, reinterpret_cast<Float3 *>(rgb));
    return hipGetLastError();
}

}  // namespace shacira
