// render.hip -- the steps either side of the hash-grid path in the NeRF pipeline (gfx950; SURVEY.md section 8 "next" f2):
// sample generation on a dense occupancy grid and volume integration over variable-length packs.
//
// Reference: the reference does these through un-vendored kaolin 0.13 CUDA (`spc_render.exponential_integration`,
// `sum_reduce`, `unbatched_raytrace`, `unbatched_query`) driven by its own Python
// (wisp/tracers/packed_rf_tracer.py:109-151, wisp/accelstructs/octree_as.py:171-290). kaolin's exponential_integration is
// a chain of five ATen/kaolin kernels with a TODO "this should be a fused kernel"; here it is one.
//
// A pack = the consecutive samples of one ray, [pack_start[r], pack_start[r+1]). One 64-lane wave walks one pack in
// chunks of 64 samples: loads are coalesced, the running optical depth is a wave scan plus a carry.
#include "grid_walk.h"
#include "internal.h"
#include "philox.h"

namespace shacira {

constexpr int kPackWaves = 4;   // packs per 256-thread workgroup

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float n = __shfl_up(v, off, 64);
        if (lane >= off) v += n;
    }
    return v;
}
__device__ __forceinline__ float wave_incl_scan_rev(float v, int lane) {   // suffix sums: lane i gets sum_{k >= i}
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float n = __shfl_down(v, off, 64);
        if (lane + off < 64) v += n;
    }
    return v;
}
// The exclusive sums are the neighbour lane's inclusive sum, never `incl - v`: when one sample dwarfs the ones before it
// (an opaque sample behind thin ones) the subtraction reads the small prefix back out of a sum whose ulp is as large as the
// prefix itself, and with v = inf it is inf - inf.
__device__ __forceinline__ float wave_excl_from_incl(float incl, int lane) {
    const float n = __shfl_up(incl, 1, 64);
    return lane == 0 ? 0.0f : n;
}
__device__ __forceinline__ float wave_excl_from_incl_rev(float incl_rev, int lane) {   // lane i gets sum_{k > i}
    const float n = __shfl_down(incl_rev, 1, 64);
    return lane == 63 ? 0.0f : n;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ray_feats[r, c] = sum_i w_i feats[i, c];  w_i = exp(-sum_{j<i} tau_j) * (1 - exp(-tau_i))   (weights out)
template <int C>
__global__ __launch_bounds__(64 * kPackWaves) void pack_integrate_fwd_kernel(const float *__restrict__ feats,
                                                                             const float *__restrict__ tau,
                                                                             const int64_t *__restrict__ pack_start,
                                                                             float *__restrict__ ray_feats,
                                                                             float *__restrict__ weights, int64_t R,
                                                                             int channels) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (r >= R) return;
    const int nc = C > 0 ? C : channels;
    const int64_t begin = pack_start[r], end = pack_start[r + 1];
    float carry = 0.0f;
    float acc[C > 0 ? C : 16];
#pragma unroll
    for (int c = 0; c < (C > 0 ? C : 16); ++c) acc[c] = 0.0f;
    for (int64_t base = begin; base < end; base += 64) {
        const int64_t i = base + lane;
        const bool live = i < end;
        const float t = live ? tau[i] : 0.0f;
        const float incl = wave_incl_scan(t, lane);
        const float excl = carry + wave_excl_from_incl(incl, lane);
        const float w = live ? expf(-excl) * (1.0f - expf(-t)) : 0.0f;
        if (live) {
            weights[i] = w;
#pragma unroll
            for (int c = 0; c < (C > 0 ? C : 16); ++c)
                if (c < nc) acc[c] = fmaf(w, feats[i * nc + c], acc[c]);
        }
        carry += __shfl(incl, 63, 64);
    }
#pragma unroll
    for (int c = 0; c < (C > 0 ? C : 16); ++c) {
        if (c < nc) {
            const float s = wave_sum(acc[c]);
            if (lane == 0) ray_feats[r * nc + c] = s;
        }
    }
}

// Backward. G_i = gw_i + sum_c gray[r, c] f[i, c];  g_f[i, c] = w_i gray[r, c];
// g_tau[i] = G_i exp(-(excl_i + tau_i)) - sum_{k > i} G_k w_k.   Pass 1 (forward) leaves excl_i in g_tau; pass 2
// walks the chunks backwards so the suffix sum is accumulated in order.
template <int C>
__global__ __launch_bounds__(64 * kPackWaves) void pack_integrate_bwd_kernel(
    const float *__restrict__ feats, const float *__restrict__ tau, const int64_t *__restrict__ pack_start,
    const float *__restrict__ g_ray, const float *__restrict__ g_w, float *__restrict__ g_feats,
    float *__restrict__ g_tau, int64_t R, int channels) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (r >= R) return;
    const int nc = C > 0 ? C : channels;
    const int64_t begin = pack_start[r], end = pack_start[r + 1];
    if (end <= begin) return;
    float gr[C > 0 ? C : 16];
#pragma unroll
    for (int c = 0; c < (C > 0 ? C : 16); ++c) gr[c] = (c < nc) ? g_ray[r * nc + c] : 0.0f;
    float carry = 0.0f;
    for (int64_t base = begin; base < end; base += 64) {
        const int64_t i = base + lane;
        const bool live = i < end;
        const float t = live ? tau[i] : 0.0f;
        const float incl = wave_incl_scan(t, lane);
        const float excl = carry + wave_excl_from_incl(incl, lane);
        if (live) g_tau[i] = excl;
        carry += __shfl(incl, 63, 64);
    }
    const int64_t nchunks = (end - begin + 63) / 64;
    float suffix = 0.0f;   // sum of G_k w_k over the chunks after this one
    for (int64_t ch = nchunks - 1; ch >= 0; --ch) {
        const int64_t i = begin + ch * 64 + lane;
        const bool live = i < end;
        float gw_term = 0.0f, e_term = 0.0f, w = 0.0f;
        if (live) {
            const float t = tau[i];
            const float excl = g_tau[i];
            const float T = expf(-excl), et = expf(-t);
            w = T * (1.0f - et);
            float G = g_w ? g_w[i] : 0.0f;
#pragma unroll
            for (int c = 0; c < (C > 0 ? C : 16); ++c) {
                if (c < nc) {
                    G = fmaf(gr[c], feats[i * nc + c], G);
                    g_feats[i * nc + c] = w * gr[c];
                }
            }
            gw_term = G * w;
            e_term = G * T * et;
        }
        const float incl_rev = wave_incl_scan_rev(gw_term, lane);   // sum_{k >= i} within the chunk
        const float after = wave_excl_from_incl_rev(incl_rev, lane);   // sum_{k > i} within the chunk
        if (live) g_tau[i] = e_term - (suffix + after);
        suffix += __shfl(incl_rev, 0, 64);
    }
}

// out[r, c] = sum_i x[i, c]          (kaolin sum_reduce)
__global__ __launch_bounds__(64 * kPackWaves) void pack_sum_kernel(const float *__restrict__ x,
                                                                   const int64_t *__restrict__ pack_start,
                                                                   float *__restrict__ out, int64_t R, int nc) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t begin = pack_start[r] * nc, end = pack_start[r + 1] * nc;
    // lanes walk the flat [samples * nc] range; lane l only ever meets channels (l + 64 k) % nc
    for (int c = 0; c < nc; ++c) {
        float acc = 0.0f;
        for (int64_t e = begin + c + (int64_t)lane * nc; e < end; e += (int64_t)64 * nc) acc += x[e];
        acc = wave_sum(acc);
        if (lane == 0) out[r * nc + c] = acc;
    }
}

// out[i, c] = per_pack[r(i), c]       (gradient of sum_reduce)
__global__ __launch_bounds__(64 * kPackWaves) void pack_broadcast_kernel(const float *__restrict__ per_pack,
                                                                         const int64_t *__restrict__ pack_start,
                                                                         float *__restrict__ out, int64_t R, int nc) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (r >= R) return;
    const int64_t begin = pack_start[r] * nc, end = pack_start[r + 1] * nc;
    for (int64_t e = begin + lane; e < end; e += 64) out[e] = per_pack[r * nc + (int)((e - begin) % nc)];
}

// ---------------------------------------------------------------------------------------------- sample generation
__device__ __forceinline__ int quantize_axis(float x, int G) {
    // kaolin's float query: cell = floor(res * (x + 1) / 2); a cell outside [0, res) does not exist (spc identify returns
    // -1 out of bounds), so a point outside the cube -- or a NaN -- belongs to no cell: -1
    const float v = floorf((float)G * (x + 1.0f) / 2.0f);
    return (v >= 0.0f && v < (float)G) ? (int)v : -1;
}

__device__ __forceinline__ bool occupied(const uint8_t *__restrict__ occ, int G, int x, int y, int z) {
    return occ[((size_t)x * G + y) * G + z] != 0;
}

// 'ray' marcher (octree_as.py:257-290): sample j of ray r sits at depth (lin[j] + jitter[r, j] / ns) * (far - near) +
// near and survives when its cell is occupied. EMIT = false: counts[r] = survivors. EMIT = true: writes them at
// offsets[r]... in sample order. One wave per ray, lanes = samples.
template <bool EMIT>
__global__ __launch_bounds__(64 * kPackWaves) void raymarch_ray_kernel(
    int64_t num_rays, int ns, const float *__restrict__ origins, const float *__restrict__ dirs, float dist_min,
    float dist_max, const float *__restrict__ lin, const float *__restrict__ jitter, const uint8_t *__restrict__ occ,
    int G, int32_t *__restrict__ counts, const int64_t *__restrict__ offsets, int64_t *__restrict__ ridx,
    float *__restrict__ samples, float *__restrict__ depth_out, float *__restrict__ deltas,
    uint8_t *__restrict__ boundary, int64_t capacity) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kPackWaves + (threadIdx.x >> 6);
    if (r >= num_rays) return;
    const float ox = origins[r * 3], oy = origins[r * 3 + 1], oz = origins[r * 3 + 2];
    const float dx = dirs[r * 3], dy = dirs[r * 3 + 1], dz = dirs[r * 3 + 2];
    const float span = dist_max - dist_min;
    int64_t out = EMIT ? offsets[r] : 0;
    const int64_t first = out;
    int total = 0;
    for (int base = 0; base < ns; base += 64) {
        const int j = base + lane;
        const bool live = j < ns;
        float depth = 0.0f, prev = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
        bool keep = false;
        if (live) {
            depth = (lin[j] + jitter[r * ns + j] / (float)ns) * span + dist_min;
            prev = (j == 0) ? dist_min : (lin[j - 1] + jitter[r * ns + j - 1] / (float)ns) * span + dist_min;
            px = fmaf(dx, depth, ox);
            py = fmaf(dy, depth, oy);
            pz = fmaf(dz, depth, oz);
            const int qx = quantize_axis(px, G), qy = quantize_axis(py, G), qz = quantize_axis(pz, G);
            keep = qx >= 0 && qy >= 0 && qz >= 0 && occupied(occ, G, qx, qy, qz);
        }
        const unsigned long long m = __ballot(keep);
        if constexpr (EMIT) {
            const int64_t k = out + __popcll(m & ((1ull << lane) - 1ull));
            // (capacity: rows of the caller's fixed-size buffers -- a step captured into a HIP graph cannot size them from
            // the count; survivors beyond it are dropped, the caller clamps its pack offsets the same way)
            if (keep && k < capacity) {
                ridx[k] = r;
                samples[k * 3] = px;
                samples[k * 3 + 1] = py;
                samples[k * 3 + 2] = pz;
                depth_out[k] = depth;
                deltas[k] = depth - prev;
                boundary[k] = (k == first) ? 1 : 0;
            }
            out += __popcll(m);
        } else {
            total += __popcll(m);
        }
    }
    if constexpr (!EMIT)
        if (lane == 0) counts[r] = total;
}

// Ray / occupied-cell intersections on the dense grid, ordered by depth (the walk of grid_walk.h); thread per ray.
// EMIT = false: counts[r]; EMIT = true: ridx / pidx (Morton index of the cell, x most significant) / depth [K, 2]
// (entry clipped to 0 for rays starting inside the volume).
template <bool EMIT>
__global__ __launch_bounds__(256) void raytrace_dense_kernel(int64_t num_rays, const float *__restrict__ origins,
                                                             const float *__restrict__ dirs,
                                                             const uint8_t *__restrict__ occ, int level,
                                                             int32_t *__restrict__ counts,
                                                             const int64_t *__restrict__ offsets,
                                                             int32_t *__restrict__ ridx, int32_t *__restrict__ pidx,
                                                             float *__restrict__ depth) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= num_rays) return;
    const int G = 1 << level;
    int32_t n = 0;
    int64_t out = EMIT ? offsets[r] : 0;
    grid_walk(origins[r * 3], origins[r * 3 + 1], origins[r * 3 + 2], dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2], level,
              [&](int cx, int cy, int cz, float t, float texit) {
                  if (!occupied(occ, G, cx, cy, cz)) return false;
                  if constexpr (EMIT) {
                      ridx[out] = (int32_t)r;
                      pidx[out] = (int32_t)morton_x_major((uint32_t)cx, (uint32_t)cy, (uint32_t)cz, level);
                      depth[out * 2] = t;
                      depth[out * 2 + 1] = texit;
                      ++out;
                  }
                  ++n;
                  return false;
              });
    if constexpr (!EMIT) counts[r] = n;
}

// 'voxel' marcher (octree_as.py:171-233), seeded: `ns` jittered samples inside every occupied crossing. Two passes over the
// scanned counts of raytrace_dense_kernel<false>. Pass 1, thread per ray: the walk again, writing the compact nuggets (ray,
// entry, exit) of the rays into the caller's workspace; a nugget whose index is >= nug_cap has no row below the capacity and
// is dropped.
__global__ __launch_bounds__(256) void raymarch_voxel_nuggets_kernel(int64_t num_rays, const float *__restrict__ origins,
                                                                     const float *__restrict__ dirs,
                                                                     const uint8_t *__restrict__ occ, int level,
                                                                     const int64_t *__restrict__ offsets, int64_t nug_cap,
                                                                     uint32_t *__restrict__ nug_ray,
                                                                     float *__restrict__ nug_t0, float *__restrict__ nug_t1) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= num_rays) return;
    const int G = 1 << level;
    int64_t out = offsets[r];
    if (out >= nug_cap) return;
    grid_walk(origins[r * 3], origins[r * 3 + 1], origins[r * 3 + 2], dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2], level,
              [&](int cx, int cy, int cz, float t, float texit) {
                  if (!occupied(occ, G, cx, cy, cz)) return false;
                  nug_ray[out] = (uint32_t)r;
                  nug_t0[out] = t;
                  nug_t1[out] = texit;
                  return ++out >= nug_cap;
              });
}

// the jitter of sample j of nugget i of ray r: word j & 3 of Philox4x32-10 on counter (r, i, j >> 2, step), key = seed
__device__ __forceinline__ float voxel_jitter(uint32_t r, uint32_t i, uint32_t j, uint32_t step, uint32_t k0, uint32_t k1) {
    uint32_t w[4];
    philox4x32_10(r, i, j >> 2, step, k0, k1, w);
    const uint32_t lo = (j & 1u) ? w[1] : w[0], hi = (j & 1u) ? w[3] : w[2];      // selects: no private segment
    return unit_open_above((j & 2u) ? hi : lo);
}

// depth of sample j between t0 and t1, every operator rounded to fp32 on its own (sampling.py:49-55 runs them as separate
// torch operators; hipcc would contract the last two into an fma)
__device__ __forceinline__ float voxel_depth(float t0, float t1, uint32_t j, float u, float inv_ns) {
    return __fadd_rn(t0, __fmul_rn(__fsub_rn(t1, t0), __fmul_rn(__fadd_rn((float)j, u), inv_ns)));
}

// Pass 2, thread per output row (row = nugget * ns + j): consecutive lanes write consecutive rows of every output.
__global__ __launch_bounds__(256) void raymarch_voxel_expand_kernel(
    int64_t num_rays, int ns, float inv_ns, const float *__restrict__ origins, const float *__restrict__ dirs,
    const int64_t *__restrict__ offsets, const uint32_t *__restrict__ nug_ray, const float *__restrict__ nug_t0,
    const float *__restrict__ nug_t1, uint32_t k0, uint32_t k1, int64_t step, const int64_t *__restrict__ step_dev,
    int64_t capacity, int64_t *__restrict__ ridx, float *__restrict__ samples, float *__restrict__ depth_out,
    float *__restrict__ deltas, uint8_t *__restrict__ boundary) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= capacity) return;
    const int64_t k = row / ns;
    if (k >= offsets[num_rays]) return;                      // behind the last nugget: the row is left untouched
    const uint32_t j = (uint32_t)(row - k * ns);
    const int64_t r = nug_ray[k];
    if (r >= num_rays) return;
    const uint32_t i = (uint32_t)(k - offsets[r]);
    const uint32_t st = (uint32_t)(uint64_t)(step + (step_dev ? *step_dev : 0));
    const float t0 = nug_t0[k], t1 = nug_t1[k];
    const float depth = voxel_depth(t0, t1, j, voxel_jitter((uint32_t)r, i, j, st, k0, k1), inv_ns);
    const float prev = j == 0 ? t0 : voxel_depth(t0, t1, j - 1, voxel_jitter((uint32_t)r, i, j - 1, st, k0, k1), inv_ns);
    ridx[row] = r;
    samples[row * 3] = fmaf(dirs[r * 3], depth, origins[r * 3]);
    samples[row * 3 + 1] = fmaf(dirs[r * 3 + 1], depth, origins[r * 3 + 1]);
    samples[row * 3 + 2] = fmaf(dirs[r * 3 + 2], depth, origins[r * 3 + 2]);
    depth_out[row] = depth;
    deltas[row] = __fsub_rn(depth, prev);
    boundary[row] = (i == 0 && j == 0) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------ host side
static inline uint32_t pack_blocks(int64_t R) { return (uint32_t)((R + kPackWaves - 1) / kPackWaves); }

hipError_t pack_integrate_launch(bool bwd, int64_t R, int C, const float *feats, const float *tau,
                                 const int64_t *pack_start, float *ray_feats, float *weights, const float *g_ray,
                                 const float *g_w, float *g_feats, float *g_tau, hipStream_t s) {
    if (R == 0) return hipSuccess;
    const dim3 grid(pack_blocks(R)), block(64 * kPackWaves);
#define SHACIRA_PACK(CC)                                                                                           \
    do {                                                                                                           \
        if (!bwd)                                                                                                  \
            hipLaunchKernelGGL((pack_integrate_fwd_kernel<CC>), grid, block, 0, s, feats, tau, pack_start, ray_feats, \
                               weights, R, C);                                                                     \
        else                                                                                                       \
            hipLaunchKernelGGL((pack_integrate_bwd_kernel<CC>), grid, block, 0, s, feats, tau, pack_start, g_ray,  \
                               g_w, g_feats, g_tau, R, C);                                                         \
    } while (0)
    switch (C) {
        case 1: SHACIRA_PACK(1); break;
        case 3: SHACIRA_PACK(3); break;
        case 4: SHACIRA_PACK(4); break;
        default: SHACIRA_PACK(0); break;
    }
#undef SHACIRA_PACK
    return hipGetLastError();
}

hipError_t pack_sum_launch(bool broadcast, int64_t R, int C, const float *in, const int64_t *pack_start, float *out,
                           hipStream_t s) {
    if (R == 0) return hipSuccess;
    if (!broadcast)
        hipLaunchKernelGGL(pack_sum_kernel, dim3(pack_blocks(R)), dim3(64 * kPackWaves), 0, s, in, pack_start, out, R, C);
    else
        hipLaunchKernelGGL(pack_broadcast_kernel, dim3(pack_blocks(R)), dim3(64 * kPackWaves), 0, s, in, pack_start, out,
                           R, C);
    return hipGetLastError();
}

hipError_t raymarch_ray_launch(bool emit, int64_t num_rays, int ns, const float *origins, const float *dirs,
                               float dist_min, float dist_max, const float *lin, const float *jitter,
                               const uint8_t *occ, int level, int32_t *counts, const int64_t *offsets, int64_t *ridx,
                               float *samples, float *depth, float *deltas, uint8_t *boundary, int64_t capacity,
                               hipStream_t s) {
    if (num_rays == 0) return hipSuccess;
    const dim3 grid(pack_blocks(num_rays)), block(64 * kPackWaves);
    if (!emit)
        hipLaunchKernelGGL(raymarch_ray_kernel<false>, grid, block, 0, s, num_rays, ns, origins, dirs, dist_min, dist_max,
                           lin, jitter, occ, 1 << level, counts, offsets, ridx, samples, depth, deltas, boundary, capacity);
    else
        hipLaunchKernelGGL(raymarch_ray_kernel<true>, grid, block, 0, s, num_rays, ns, origins, dirs, dist_min, dist_max,
                           lin, jitter, occ, 1 << level, counts, offsets, ridx, samples, depth, deltas, boundary, capacity);
    return hipGetLastError();
}

hipError_t raytrace_dense_launch(bool emit, int64_t num_rays, const float *origins, const float *dirs,
                                 const uint8_t *occ, int level, int32_t *counts, const int64_t *offsets, int32_t *ridx,
                                 int32_t *pidx, float *depth, hipStream_t s) {
    if (num_rays == 0) return hipSuccess;
    const dim3 grid((uint32_t)((num_rays + 255) / 256)), block(256);
    if (!emit)
        hipLaunchKernelGGL(raytrace_dense_kernel<false>, grid, block, 0, s, num_rays, origins, dirs, occ, level, counts,
                           offsets, ridx, pidx, depth);
    else
        hipLaunchKernelGGL(raytrace_dense_kernel<true>, grid, block, 0, s, num_rays, origins, dirs, occ, level, counts,
                           offsets, ridx, pidx, depth);
    return hipGetLastError();
}

hipError_t raymarch_voxel_launch(int64_t num_rays, int ns, const float *origins, const float *dirs, const uint8_t *occ,
                                 int level, const int64_t *offsets, uint64_t seed, int64_t step, const int64_t *step_dev,
                                 int64_t capacity, void *workspace, int64_t *ridx, float *samples, float *depth,
                                 float *deltas, uint8_t *boundary, hipStream_t s) {
    if (num_rays == 0 || capacity == 0) return hipSuccess;
    const int64_t nug_cap = (capacity + ns - 1) / ns;
    uint32_t *nug_ray = (uint32_t *)workspace;
    float *nug_t0 = (float *)(nug_ray + nug_cap), *nug_t1 = nug_t0 + nug_cap;
    hipLaunchKernelGGL(raymarch_voxel_nuggets_kernel, dim3((uint32_t)((num_rays + 255) / 256)), dim3(256), 0, s, num_rays,
                       origins, dirs, occ, level, offsets, nug_cap, nug_ray, nug_t0, nug_t1);
    const float inv_ns = (float)(1.0 / (double)ns);          // the fp32 value of Python's 1.0 / num_samples
    hipLaunchKernelGGL(raymarch_voxel_expand_kernel, dim3((uint32_t)((capacity + 255) / 256)), dim3(256), 0, s, num_rays, ns,
                       inv_ns, origins, dirs, offsets, nug_ray, nug_t0, nug_t1, (uint32_t)seed, (uint32_t)(seed >> 32), step,
                       step_dev, capacity, ridx, samples, depth, deltas, boundary);
    return hipGetLastError();
}

}  // namespace shacira
