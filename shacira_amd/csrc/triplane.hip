// triplane.hip -- TriplanarGrid sampling (gfx950): forward, plane gradients and coordinate gradient of the reference's
// per-LOD `grid_sample(bilinear, align_corners=True, padding_mode='reflection')` on the three planes fmx (y, z), fmy (x, z),
// fmz (x, y). The contract and the evaluation orders: include/shacira_hip.h above shacira_triplane_forward. DESIGN.md 4.7.
//
//   forward          one launch, lane per sample, every selected LOD and all three planes; reads an HWC copy of the
//                    planes that one transpose launch writes into the workspace (the rule, 3x faster), or with option
//                    "triplane_layout" = 0 the NCHW parameters in place (F loads per corner); profiles/triplane.md
//   plane backward   no scattered global atomics on the bulk: the samples are counting-sorted (block_sort.h) by a 3-D
//                    block of the reflected cube (one sort serves all three planes: a block's projection on each plane is
//                    a square window); a workgroup takes up to kTriChunk samples of one block, accumulates each LOD's
//                    three windows in LDS and flushes the non-zero texels with coalesced global adds. Corners that miss
//                    the window (rounding at a block face) and LODs whose windows exceed the LDS budget add straight to
//                    global memory.
//   coord backward   a gather, lane per sample, no atomics (reads the planes: only when the coordinate gradient is asked)
#include <cfloat>
#include <climits>

#include "block_sort.h"
#include "internal.h"

namespace shacira {

#ifndef SHACIRA_TRI_CHUNK
#define SHACIRA_TRI_CHUNK 512
#endif
constexpr int kTriChunk = SHACIRA_TRI_CHUNK;   // samples per accumulation unit (one workgroup); profiles/triplane.md
constexpr int kTriLdsBytes = 64 * 1024;    // LDS budget of the three windows of one LOD (two workgroups per CU)

// ---- the index math of ATen/native/cuda/GridSampler.cuh (align_corners = true, reflection), fp32 --------------------------
__device__ __forceinline__ float tri_unnormalize(float c, int size) { return ((c + 1.f) / 2) * (float)(size - 1); }

__device__ __forceinline__ float tri_reflect(float in, int size, float *grad) {
    // reflect_coordinates(in, 0, 2 * (size - 1)) [and its _set_grad twin]; size >= 2 always (2^lod + 1 texels)
    const float span = (float)(2 * (size - 1)) / 2;
    float mult = 1.0f;
    if (grad) {
        if (in < 0.0f) {
            mult = -1.0f;
            in = -in;
        }
    } else {
        in = fabsf(in);
    }
    const float extra = fmodf(in, span);
    const int flips = (int)floorf(in / span);
    if (flips % 2 == 0) {
        if (grad) *grad = mult;
        return extra;
    }
    if (grad) *grad = -mult;
    return span - extra;
}

__device__ __forceinline__ float tri_downgrade(float x) {
    if (x > (float)(INT_MAX - 1) || x < (float)INT_MIN || !isfinite(x)) return -100.0f;
    return x;
}

// forward source index: clip_coordinates (fmaxf / fminf: a NaN becomes 0, as ::max / ::min do on the device)
__device__ __forceinline__ float tri_source_index(float c, int size) {
    float x = tri_unnormalize(c, size);
    x = tri_reflect(x, size, nullptr);
    x = fminf((float)(size - 1), fmaxf(x, 0.0f));
    return tri_downgrade(x);
}

// backward source index and d(index)/d(coord): clip_coordinates_set_grad (both borders: gradient 0; NaN passes, -> -100)
__device__ __forceinline__ float tri_source_index_grad(float c, int size, float *gmult) {
    const float gun = (float)(size - 1) / 2;
    float x = tri_unnormalize(c, size);
    float grefl, gclip;
    x = tri_reflect(x, size, &grefl);
    if (x <= 0.0f) {
        gclip = 0.0f;
        x = 0.0f;
    } else if (x >= (float)(size - 1)) {
        gclip = 0.0f;
        x = (float)(size - 1);
    } else {
        gclip = 1.0f;
    }
    *gmult = gun * grefl * gclip;
    return tri_downgrade(x);
}

// bilinear corners of one plane: nw = (x0, y0), ne = (x0 + 1, y0), sw = (x0, y0 + 1), se = (x0 + 1, y0 + 1)
struct TriCorners {
    int x0, y0;
    float w[4];      // nw, ne, sw, se
    float ix, iy;
};
__device__ __forceinline__ void tri_corners(float ix, float iy, TriCorners &c) {
    c.ix = ix;
    c.iy = iy;
    c.x0 = (int)floorf(ix);
    c.y0 = (int)floorf(iy);
    const float x1 = (float)(c.x0 + 1), y1 = (float)(c.y0 + 1), x0 = (float)c.x0, y0 = (float)c.y0;
    c.w[0] = (x1 - ix) * (y1 - iy);
    c.w[1] = (ix - x0) * (y1 - iy);
    c.w[2] = (x1 - ix) * (iy - y0);
    c.w[3] = (ix - x0) * (iy - y0);
}
__device__ __forceinline__ bool tri_inb(int x, int y, int S) { return x >= 0 && x < S && y >= 0 && y < S; }

// plane p of a sample (x, y, z): width coordinate, height coordinate
__device__ __forceinline__ void tri_plane_coords(int p, const float (&c)[3], float &u, float &v) {
    u = p == 0 ? c[1] : c[0];
    v = p == 2 ? c[1] : c[2];
}

// ---- forward ----------------------------------------------------------------------------------------------------------
// out_acc = 0, then += value * weight for nw, ne, sw, se (in-bounds corners only): the reference kernel's order. 'sum':
// s = v_0, then s = s + v_l for l ascending. F > 0: compile-time feature dim (registers); F == 0: runtime, 'sum' adds up in
// the output row itself.
template <bool HWC, int F, bool SUM>
__global__ __launch_bounds__(256) void triplane_fwd_kernel(TriplaneArgs a, const float *__restrict__ coords,
                                                           const float *__restrict__ hwc, float *__restrict__ feats,
                                                           int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int Fr = F > 0 ? F : a.fdim;
    const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
    const int K = SUM ? 3 * Fr : a.num_lods * 3 * Fr;
    float *orow = feats + i * (int64_t)K;
    float acc[3][F > 0 ? F : 1];
#pragma unroll 1
    for (int l = 0; l < a.num_lods; ++l) {
        const int S = a.side[l];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            float u, v;
            tri_plane_coords(p, c, u, v);
            TriCorners cr;
            tri_corners(tri_source_index(u, S), tri_source_index(v, S), cr);
            const bool in[4] = {tri_inb(cr.x0, cr.y0, S), tri_inb(cr.x0 + 1, cr.y0, S), tri_inb(cr.x0, cr.y0 + 1, S),
                                tri_inb(cr.x0 + 1, cr.y0 + 1, S)};
            const int64_t t[4] = {(int64_t)cr.y0 * S + cr.x0, (int64_t)cr.y0 * S + cr.x0 + 1,
                                  (int64_t)(cr.y0 + 1) * S + cr.x0, (int64_t)(cr.y0 + 1) * S + cr.x0 + 1};
            const float *plane = HWC ? hwc + a.hwc_off[3 * l + p] : a.plane[3 * l + p];
            const int64_t cs = HWC ? 1 : (int64_t)S * S;     // channel stride
            const int64_t ts = HWC ? Fr : 1;                // texel stride
            if constexpr (F > 0) {
                float val[F];
#pragma unroll
                for (int j = 0; j < F; ++j) val[j] = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!in[k]) continue;
                    const float *src = plane + t[k] * ts;
                    float cv[F];
                    if constexpr (HWC && F % 4 == 0) {
#pragma unroll
                        for (int j = 0; j < F; j += 4) {
                            const float4 q = *reinterpret_cast<const float4 *>(src + j);
                            cv[j] = q.x; cv[j + 1] = q.y; cv[j + 2] = q.z; cv[j + 3] = q.w;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < F; ++j) cv[j] = src[j * cs];
                    }
#pragma unroll
                    for (int j = 0; j < F; ++j) val[j] = val[j] + cv[j] * cr.w[k];
                }
#pragma unroll
                for (int j = 0; j < F; ++j) {
                    if constexpr (SUM) acc[p][j] = (l == 0) ? val[j] : acc[p][j] + val[j];
                    else orow[(l * 3 + p) * F + j] = val[j];
                }
            } else {
                for (int j = 0; j < Fr; ++j) {
                    float val = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (in[k]) val = val + plane[t[k] * ts + j * cs] * cr.w[k];
                    if constexpr (SUM) orow[p * Fr + j] = (l == 0) ? val : orow[p * Fr + j] + val;
                    else orow[(l * 3 + p) * Fr + j] = val;
                }
            }
        }
    }
    if constexpr (SUM && F > 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < F; ++j) orow[p * F + j] = acc[p][j];
    }
}

// NCHW planes -> one HWC copy per call (texel-major, channel-minor), planes back to back at a.hwc_off[]; blockIdx.y = plane
__global__ __launch_bounds__(256) void triplane_to_hwc_kernel(TriplaneArgs a, float *__restrict__ hwc) {
    const int q = blockIdx.y;
    const int F = a.fdim;
    const int64_t SS = (int64_t)a.side[q / 3] * a.side[q / 3];
    const float *src = a.plane[q];
    float *dst = hwc + a.hwc_off[q];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < SS * F; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t texel = e / F;
        const int j = (int)(e - texel * F);
        dst[e] = src[j * SS + texel];
    }
}

// ---- plane backward ---------------------------------------------------------------------------------------------------
// block of a sample (the sort's BlockOf, block_sort.h): its texel cell of the finest LOD over the block edge, x fastest
struct TriBlockOf {
    int32_t sort_side, cells, nb;
    __device__ uint32_t operator()(const float *coords, int64_t i) const {
        uint32_t b = 0, mul = 1;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float g;
            const float x = tri_source_index_grad(coords[i * 3 + d], sort_side, &g);
            int q = x < 0.0f ? 0 : (int)x / cells;
            q = q < 0 ? 0 : (q >= nb ? nb - 1 : q);
            b += (uint32_t)q * mul;
            mul *= (uint32_t)nb;
        }
        return b;
    }
};

// zero the plane gradients and the block histogram
__global__ __launch_bounds__(256) void triplane_zero_kernel(TriplaneArgs a, uint32_t *__restrict__ hist, int nbins) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int q = 0; q < 3 * a.num_lods; ++q) {
        const int64_t n = (int64_t)a.side[q / 3] * a.side[q / 3] * a.fdim;
        float *g = a.grad[q];
        for (int64_t e = t0; e < n; e += stride) g[e] = 0.0f;
    }
    if (hist)
        for (int64_t e = t0; e < nbins; e += stride) hist[e] = 0u;
}

// A unit = up to kTriChunk sorted samples of one block. Per LOD: zero the three windows, LDS-add every corner that falls
// inside its window (the rest: global adds), flush non-zero texels with global adds ([plane][channel][y][x]: consecutive
// lanes, consecutive x).
__global__ __launch_bounds__(256) void triplane_accum_kernel(TriplaneArgs a, TriBwdPlan bp, const float *__restrict__ coords,
                                                             const float *__restrict__ grad_out,
                                                             const uint32_t *__restrict__ sorted,
                                                             const uint32_t *__restrict__ start,
                                                             const uint32_t *__restrict__ ustart, int64_t N) {
    extern __shared__ float win[];
    int b;
    uint32_t s0, s1;
    if (!block_sort_unit<kTriChunk>(blockIdx.x, bp.nbins, start, ustart, b, s0, s1)) return;
    const int bq[3] = {b % bp.nb, (b / bp.nb) % bp.nb, b / (bp.nb * bp.nb)};
    const int F = a.fdim;
    const int gstride = bp.sum ? 3 * F : a.num_lods * 3 * F;
#pragma unroll 1
    for (int l = 0; l < a.num_lods; ++l) {
        const int S = a.side[l];
        const int R = S - 1;
        const int ww = bp.win[l];             // window side (texels), 0: no window (global adds)
        int org[3];                           // window origin per cube axis
#pragma unroll
        for (int d = 0; d < 3; ++d) org[d] = R >= bp.nb ? bq[d] * (R / bp.nb) : (bq[d] * R) / bp.nb;
        const int wsz = ww * ww * F;
        if (ww > 0) {
            for (int e = threadIdx.x; e < 3 * wsz; e += blockDim.x) win[e] = 0.0f;
            __syncthreads();
        }
        for (uint32_t s = s0 + threadIdx.x; s < s1; s += blockDim.x) {
            const int64_t i = sorted[s];
            const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
            const float *g = grad_out + i * (int64_t)gstride + (bp.sum ? 0 : l * 3 * F);
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                float u, v, gu, gv;
                tri_plane_coords(p, c, u, v);
                TriCorners cr;
                tri_corners(tri_source_index_grad(u, S, &gu), tri_source_index_grad(v, S, &gv), cr);
                const int ox = org[p == 0 ? 1 : 0], oy = org[p == 2 ? 1 : 2];
                float *gp = a.grad[3 * l + p];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = cr.x0 + (k & 1), y = cr.y0 + (k >> 1);
                    if (!tri_inb(x, y, S)) continue;
                    const bool local = ww > 0 && (unsigned)(x - ox) < (unsigned)ww && (unsigned)(y - oy) < (unsigned)ww;
                    for (int j = 0; j < F; ++j) {
                        const float add = cr.w[k] * g[p * F + j];
                        if (local) atomicAdd(&win[p * wsz + (j * ww + (y - oy)) * ww + (x - ox)], add);
                        else atomicAdd(&gp[((int64_t)j * S + y) * S + x], add);
                    }
                }
            }
        }
        if (ww > 0) {
            __syncthreads();
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const int ox = org[p == 0 ? 1 : 0], oy = org[p == 2 ? 1 : 2];
                float *gp = a.grad[3 * l + p];
                for (int e = threadIdx.x; e < wsz; e += blockDim.x) {
                    const float val = win[p * wsz + e];
                    if (val == 0.0f) continue;
                    const int j = e / (ww * ww);
                    const int r = e - j * ww * ww;
                    const int y = r / ww + oy, x = r % ww + ox;
                    if (x < S && y < S) atomicAdd(&gp[((int64_t)j * S + y) * S + x], val);
                }
            }
            __syncthreads();
        }
    }
}

// ---- coordinate backward (gather) -------------------------------------------------------------------------------------
// Per plane, the reference kernel's gix / giy: from 0, channel by channel, corners nw, ne, sw, se, in-bounds only:
//   gix -= nw_v * (y1 - iy) * g; giy -= nw_v * (x1 - ix) * g;  gix += ne_v * (y1 - iy) * g; giy -= ne_v * (ix - x0) * g;
//   gix -= sw_v * (iy - y0) * g; giy += sw_v * (x1 - ix) * g;  gix += se_v * (iy - y0) * g; giy += se_v * (ix - x0) * g;
// then d/du = mult_u * gix, d/dv = mult_v * giy. grad[a] = 0, then += those terms for l ascending, planes x, y, z.
__global__ __launch_bounds__(256) void triplane_coord_grad_kernel(TriplaneArgs a, int sum, const float *__restrict__ coords,
                                                                  const float *__restrict__ grad_out,
                                                                  float *__restrict__ grad_coords, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int F = a.fdim;
    const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
    const int gstride = sum ? 3 * F : a.num_lods * 3 * F;
    float grad[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int l = 0; l < a.num_lods; ++l) {
        const int S = a.side[l];
        const float *g = grad_out + i * (int64_t)gstride + (sum ? 0 : l * 3 * F);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            float u, v, mu, mv;
            tri_plane_coords(p, c, u, v);
            TriCorners cr;
            tri_corners(tri_source_index_grad(u, S, &mu), tri_source_index_grad(v, S, &mv), cr);
            const float ix = cr.ix, iy = cr.iy;
            const float x0 = (float)cr.x0, y0 = (float)cr.y0, x1 = (float)(cr.x0 + 1), y1 = (float)(cr.y0 + 1);
            const bool in[4] = {tri_inb(cr.x0, cr.y0, S), tri_inb(cr.x0 + 1, cr.y0, S), tri_inb(cr.x0, cr.y0 + 1, S),
                                tri_inb(cr.x0 + 1, cr.y0 + 1, S)};
            const float *plane = a.plane[3 * l + p];
            const int64_t SS = (int64_t)S * S;
            const int64_t t00 = (int64_t)cr.y0 * S + cr.x0;
            float gix = 0.0f, giy = 0.0f;
            for (int j = 0; j < F; ++j) {
                const float go = g[p * F + j];
                const float *pj = plane + j * SS;
                if (in[0]) {
                    const float val = pj[t00];
                    gix -= val * (y1 - iy) * go;
                    giy -= val * (x1 - ix) * go;
                }
                if (in[1]) {
                    const float val = pj[t00 + 1];
                    gix += val * (y1 - iy) * go;
                    giy -= val * (ix - x0) * go;
                }
                if (in[2]) {
                    const float val = pj[t00 + S];
                    gix -= val * (iy - y0) * go;
                    giy += val * (x1 - ix) * go;
                }
                if (in[3]) {
                    const float val = pj[t00 + S + 1];
                    gix += val * (iy - y0) * go;
                    giy += val * (ix - x0) * go;
                }
            }
            const int au = p == 0 ? 1 : 0, av = p == 2 ? 1 : 2;
            grad[au] += mu * gix;
            grad[av] += mv * giy;
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) grad_coords[i * 3 + d] = grad[d];
}

// ------------------------------------------------------------------------------------------------------- host side
static int tri_layout_hwc(const TriplaneArgs &a) {
    const int v = opt().triplane_layout;
    return v < 0 ? kTriDefaultHwc : v;
}

size_t triplane_forward_workspace(const TriplaneArgs &a, int64_t n) {
    if (n <= 0 || !tri_layout_hwc(a)) return 0;
    int64_t total = 0;
    for (int l = 0; l < a.num_lods; ++l) total += 3 * (int64_t)a.side[l] * a.side[l] * a.fdim;
    return (size_t)total * sizeof(float);
}

template <bool HWC, bool SUM>
static void launch_fwd(const TriplaneArgs &a, const float *coords, const float *hwc, float *feats, int64_t n,
                       hipStream_t s) {
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
    switch (a.fdim) {
#define TRI_F(FV) \
    case FV: hipLaunchKernelGGL((triplane_fwd_kernel<HWC, FV, SUM>), grid, block, 0, s, a, coords, hwc, feats, n); return;
        TRI_F(1) TRI_F(2) TRI_F(4) TRI_F(8) TRI_F(16)
#undef TRI_F
        default: hipLaunchKernelGGL((triplane_fwd_kernel<HWC, 0, SUM>), grid, block, 0, s, a, coords, hwc, feats, n);
    }
}

hipError_t triplane_forward_dispatch(TriplaneArgs a, const float *coords, int sum, float *feats, void *workspace,
                                     int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    float *hwc = nullptr;
    if (tri_layout_hwc(a)) {
        hwc = static_cast<float *>(workspace);
        int64_t off = 0;
        for (int q = 0; q < 3 * a.num_lods; ++q) {
            a.hwc_off[q] = off;
            off += (int64_t)a.side[q / 3] * a.side[q / 3] * a.fdim;
        }
        const int64_t most = (int64_t)a.side[a.num_lods - 1] * a.side[a.num_lods - 1] * a.fdim;   // (sides grow with l)
        const uint32_t blocks = (uint32_t)std::min<int64_t>((most + 255) / 256, 1024);
        hipLaunchKernelGGL(triplane_to_hwc_kernel, dim3(blocks, 3 * a.num_lods), dim3(256), 0, s, a, hwc);
        if (sum) launch_fwd<true, true>(a, coords, hwc, feats, n, s);
        else launch_fwd<true, false>(a, coords, hwc, feats, n, s);
    } else {
        if (sum) launch_fwd<false, true>(a, coords, nullptr, feats, n, s);
        else launch_fwd<false, false>(a, coords, nullptr, feats, n, s);
    }
    return hipGetLastError();
}

// the sort's block grid and every LOD's window (host, from the shape alone)
void triplane_backward_plan(const TriplaneArgs &a, int sum, TriBwdPlan &bp) {
    int rmax = 1;
    for (int l = 0; l < a.num_lods; ++l) rmax = std::max(rmax, a.side[l] - 1);
    const auto fits = [&](int w) { return (int64_t)3 * w * w * a.fdim * (int64_t)sizeof(float) <= kTriLdsBytes; };
    int cells = rmax;   // largest power-of-two block edge (texels of the finest LOD) whose windows fit
    while (cells > 1 && !fits(cells + 1)) cells >>= 1;
    int nb = rmax / cells;
    if (nb > kBlockSortMaxBlocksAxis) nb = kBlockSortMaxBlocksAxis;
    bp.nb = nb;
    bp.nbins = nb * nb * nb;
    bp.sort_side = rmax + 1;
    bp.cells = rmax / nb;
    bp.sum = sum;
    for (int l = 0; l < a.num_lods; ++l) {
        const int R = a.side[l] - 1;
        const int w = R >= nb ? R / nb + 1 : 2;
        bp.win[l] = fits(w) ? w : 0;
    }
}

size_t triplane_backward_workspace(const TriplaneArgs &a, int sum, int64_t n) {
    if (n <= 0) return 0;
    TriBwdPlan bp;
    triplane_backward_plan(a, sum, bp);
    return block_sort_workspace_bytes(bp.nbins, n);
}

hipError_t triplane_backward_dispatch(const TriplaneArgs &a, const float *coords, const float *grad_out, int sum,
                                      bool planes, float *grad_coords, void *workspace, int64_t n, hipStream_t s) {
    if (n <= 0) {
        if (!planes) return hipSuccess;
        hipLaunchKernelGGL(triplane_zero_kernel, dim3(1024), dim3(256), 0, s, a, nullptr, 0);
        return hipGetLastError();
    }
    if (grad_coords) {
        hipLaunchKernelGGL(triplane_coord_grad_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, a, sum, coords,
                           grad_out, grad_coords, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (!planes) return hipSuccess;
    TriBwdPlan bp;
    triplane_backward_plan(a, sum, bp);
    const BlockSortBuffers buf = block_sort_carve(workspace, bp.nbins);
    hipLaunchKernelGGL(triplane_zero_kernel, dim3(1024), dim3(256), 0, s, a, buf.hist, bp.nbins);
    const uint32_t units =
        block_sort_launch<kTriChunk>(TriBlockOf{bp.sort_side, bp.cells, bp.nb}, coords, n, bp.nbins, buf, s);
    int wmax = 0;
    for (int l = 0; l < a.num_lods; ++l) wmax = std::max(wmax, bp.win[l]);
    const size_t lds = (size_t)3 * wmax * wmax * a.fdim * sizeof(float);
    static PerDeviceOnce once;
    if (hipError_t e = once.run([] {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(triplane_accum_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kTriLdsBytes);
        }))
        return e;
    hipLaunchKernelGGL(triplane_accum_kernel, dim3(units), dim3(256), lds, s, a, bp, coords, grad_out, buf.sorted,
                       buf.start, buf.ustart, n);
    return hipGetLastError();
}

}  // namespace shacira
