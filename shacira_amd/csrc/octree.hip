// octree.hip -- OctreeGrid / CodebookOctreeGrid feature lookup (gfx950): forward, feature gradients and coordinate gradient
// of the trilinear blend of the eight corner rows of an occupied octree cell, every requested level in one call. The
// contract: include/shacira_hip.h above shacira_octree_forward. DESIGN.md 4.3c.
//
//   index            per level an occupancy bit grid over the cells and a corner bit grid over the lattice points with a
//                    row count before every 32-bit word: row = count + popcount(bits below). Rows ascend with the lattice
//                    key (x * S + y) * S + z, so the z and z + 1 corners of a cell edge are rows r and r + 1: four index
//                    reads and four reads of 2F contiguous floats per sample and level.
//   forward          one launch, lane per sample, every level; writes the 'cat' or the summed 'sum' row itself
//   feature backward no scattered global atomics on the coarse levels: the samples are counting-sorted (block_sort.h)
//                    by a block of cells of the finest level (cells nest exactly across levels: p_l is p_fine scaled by a
//                    power of two); a workgroup takes up to kOctChunk samples of one block, one lane per (sample, corner),
//                    adds into one LDS window per level and flushes the non-zero entries with global adds (consecutive
//                    lanes, consecutive floats of consecutive rows). A level whose window does not fit adds straight to
//                    memory.
//   coord backward   a gather, lane per sample, no atomics (reads the tables: only when the coordinate gradient is asked)
#include "block_sort.h"
#include "internal.h"

namespace shacira {

constexpr int kOctChunk = 512;             // samples per accumulation unit (one workgroup)
constexpr int kOctLdsBytes = 64 * 1024;    // LDS budget of one unit's windows (two workgroups per CU at the limit)
constexpr int kOctMaxCellsLog2 = 4;        // largest block edge: 16 cells of the finest level

struct OctCell {
    int x, y, z;
    float tx, ty, tz;
};

// p = (c + 1) * (G / 2): G / 2 is a power of two, only the addition rounds. false: outside [0, G)^3 or not finite.
__device__ __forceinline__ bool oct_locate(int level, const float (&c)[3], OctCell &q) {
    const float g = (float)(1 << level);
    const float h = g * 0.5f;
    const float px = (c[0] + 1.0f) * h, py = (c[1] + 1.0f) * h, pz = (c[2] + 1.0f) * h;
    if (!(px >= 0.0f && px < g && py >= 0.0f && py < g && pz >= 0.0f && pz < g)) return false;
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    q.x = (int)fx;
    q.y = (int)fy;
    q.z = (int)fz;
    q.tx = px - fx;
    q.ty = py - fy;
    q.tz = pz - fz;
    return true;
}

__device__ __forceinline__ bool oct_occupied(const uint32_t *__restrict__ occ, int level, const OctCell &q) {
    const uint32_t key = ((((uint32_t)q.x << level) + (uint32_t)q.y) << level) + (uint32_t)q.z;
    return (occ[key >> 5] >> (key & 31u)) & 1u;
}

// table row of lattice point (x, y, z), 0 <= x, y, z <= G; -1 where it is no corner of an occupied cell
__device__ __forceinline__ int64_t oct_row(const uint2 *__restrict__ corner, int level, int x, int y, int z) {
    const uint32_t S = (1u << level) + 1u;
    const uint32_t key = ((uint32_t)x * S + (uint32_t)y) * S + (uint32_t)z;
    const uint2 e = corner[key >> 5];
    const uint32_t b = key & 31u;
    if (!((e.x >> b) & 1u)) return -1;
    return (int64_t)e.y + __popc(e.x & ((1u << b) - 1u));
}

// rows of the four z-edges of the cell, r[dx * 2 + dy] = row of (x + dx, y + dy, z); (.., z + 1) is the next row.
// false where the index disagrees with the occupancy or the row count (never for an index built from the occupancy).
__device__ __forceinline__ bool oct_edge_rows(const OctreeArgs &a, int l, const OctCell &q, int64_t (&r)[4]) {
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = oct_row(a.corner[l], a.level[l], q.x + (e >> 1), q.y + (e & 1), q.z);
        ok = ok && r[e] >= 0 && r[e] + 1 < a.rows[l];
    }
    return ok;
}

__device__ __forceinline__ float oct_weight(const OctCell &q, int k) {
    const float wx = (k & 4) ? q.tx : 1.0f - q.tx;
    const float wy = (k & 2) ? q.ty : 1.0f - q.ty;
    const float wz = (k & 1) ? q.tz : 1.0f - q.tz;
    return wx * wy * wz;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
// value = 0, then += w_k * row_k for k = 0..7. 'sum': s = value_0, then s = s + value_l. F > 0: compile-time feature dim
// (registers); F == 0: runtime, 'sum' adds up in the output row itself.
template <int F, bool SUM>
__global__ __launch_bounds__(256) void octree_fwd_kernel(OctreeArgs a, const float *__restrict__ coords,
                                                         float *__restrict__ feats, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int Fr = F > 0 ? F : a.fdim;
    const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
    float *orow = feats + i * (int64_t)(SUM ? Fr : a.num_levels * Fr);
    float acc[F > 0 ? F : 1];
#pragma unroll 1
    for (int l = 0; l < a.num_levels; ++l) {
        OctCell q;
        int64_t r[4];
        const bool hit = oct_locate(a.level[l], c, q) && oct_occupied(a.occ[l], a.level[l], q) && oct_edge_rows(a, l, q, r);
        const float *tab = a.table[l];
        if constexpr (F > 0) {
            float val[F];
#pragma unroll
            for (int j = 0; j < F; ++j) val[j] = 0.0f;
            if (hit) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float *src = tab + r[e] * F;   // rows r and r + 1: 2F contiguous floats
                    float cv[2 * F];
                    if constexpr (F % 4 == 0) {
#pragma unroll
                        for (int j = 0; j < 2 * F; j += 4) {
                            const float4 v = *reinterpret_cast<const float4 *>(src + j);
                            cv[j] = v.x; cv[j + 1] = v.y; cv[j + 2] = v.z; cv[j + 3] = v.w;
                        }
                    } else if constexpr (F % 2 == 0) {
#pragma unroll
                        for (int j = 0; j < 2 * F; j += 2) {
                            const float2 v = *reinterpret_cast<const float2 *>(src + j);
                            cv[j] = v.x; cv[j + 1] = v.y;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 2 * F; ++j) cv[j] = src[j];
                    }
                    const float w0 = oct_weight(q, 2 * e), w1 = oct_weight(q, 2 * e + 1);
#pragma unroll
                    for (int j = 0; j < F; ++j) val[j] = val[j] + w0 * cv[j];
#pragma unroll
                    for (int j = 0; j < F; ++j) val[j] = val[j] + w1 * cv[F + j];
                }
            }
#pragma unroll
            for (int j = 0; j < F; ++j) {
                if constexpr (SUM) acc[j] = (l == 0) ? val[j] : acc[j] + val[j];
                else orow[l * F + j] = val[j];
            }
        } else {
            for (int j = 0; j < Fr; ++j) {
                float val = 0.0f;
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) val = val + oct_weight(q, k) * tab[(r[k >> 1] + (k & 1)) * Fr + j];
                }
                if constexpr (SUM) orow[j] = (l == 0) ? val : orow[j] + val;
                else orow[l * Fr + j] = val;
            }
        }
    }
    if constexpr (SUM && F > 0) {
#pragma unroll
        for (int j = 0; j < F; ++j) orow[j] = acc[j];
    }
}

// ---- feature backward ---------------------------------------------------------------------------------------------------
// block of a sample (the sort's BlockOf, block_sort.h): its cell of the finest level (clamped into the cube; not finite
// -> 0) over the block edge, z fastest
struct OctBlockOf {
    int32_t fine, cells_log2, nb;
    __device__ uint32_t operator()(const float *coords, int64_t i) const {
        const float g = (float)(1 << fine);
        const float h = g * 0.5f;
        uint32_t b = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float p = (coords[i * 3 + d] + 1.0f) * h;
            int cell = (p >= 0.0f && p < g) ? (int)floorf(p) : (p >= g ? (1 << fine) - 1 : 0);
            int q = cell >> cells_log2;
            q = q < 0 ? 0 : (q >= nb ? nb - 1 : q);
            b = b * (uint32_t)nb + (uint32_t)q;
        }
        return b;
    }
};

// zero the table gradients (padding rows included) and the block histogram
__global__ __launch_bounds__(256) void octree_zero_kernel(OctreeArgs a, uint32_t *__restrict__ hist, int nbins) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int l = 0; l < a.num_levels; ++l) {
        const int64_t n = (a.rows[l] + 1) * a.fdim;
        float *g = a.grad[l];
        for (int64_t e = t0; e < n; e += stride) g[e] = 0.0f;
    }
    if (hist)
        for (int64_t e = t0; e < nbins; e += stride) hist[e] = 0u;
}

// A unit = up to kOctChunk sorted samples of one block. Zero the windows; one lane per (sample, corner) adds w_k * g into
// the level's window (a level without one, and a corner outside its window, add to memory); flush the non-zero entries.
__global__ __launch_bounds__(256) void octree_accum_kernel(OctreeArgs a, OctBwdPlan bp, const float *__restrict__ coords,
                                                           const float *__restrict__ grad_out,
                                                           const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ start,
                                                           const uint32_t *__restrict__ ustart) {
    extern __shared__ float win[];
    int b;
    uint32_t s0, s1;
    if (!block_sort_unit<kOctChunk>(blockIdx.x, bp.nbins, start, ustart, b, s0, s1)) return;
    // the block's first cell of the finest level, per axis
    const int org[3] = {(b / (bp.nb * bp.nb)) << bp.cells_log2, ((b / bp.nb) % bp.nb) << bp.cells_log2,
                        (b % bp.nb) << bp.cells_log2};
    const int F = a.fdim;
    const int gstride = bp.sum ? F : a.num_levels * F;
    for (int e = threadIdx.x; e < bp.wtotal; e += blockDim.x) win[e] = 0.0f;
    __syncthreads();
    const uint32_t items = (s1 - s0) * 8u;
    for (uint32_t it = threadIdx.x; it < items; it += blockDim.x) {
        const int64_t i = sorted[s0 + (it >> 3)];
        const int k = (int)(it & 7u);
        const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
#pragma unroll 1
        for (int l = 0; l < a.num_levels; ++l) {
            const int lev = a.level[l];
            OctCell q;
            if (!oct_locate(lev, c, q) || !oct_occupied(a.occ[l], lev, q)) continue;
            const float w = oct_weight(q, k);
            const float *g = grad_out + i * (int64_t)gstride + (bp.sum ? 0 : l * F);
            const int x = q.x + (k >> 2 & 1), y = q.y + (k >> 1 & 1), z = q.z + (k & 1);
            const int ws = bp.wside[l];
            const int sh = bp.fine - lev;
            const int wx = x - (org[0] >> sh), wy = y - (org[1] >> sh), wz = z - (org[2] >> sh);
            if (ws > 0 && (unsigned)wx < (unsigned)ws && (unsigned)wy < (unsigned)ws && (unsigned)wz < (unsigned)ws) {
                float *dst = win + bp.woff[l] + ((wx * ws + wy) * ws + wz) * F;
                for (int j = 0; j < F; ++j) atomicAdd(&dst[j], w * g[j]);
            } else {
                const int64_t row = oct_row(a.corner[l], lev, x, y, z);
                if (row < 0 || row >= a.rows[l]) continue;
                float *dst = a.grad[l] + row * F;
                for (int j = 0; j < F; ++j) atomicAdd(&dst[j], w * g[j]);
            }
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < a.num_levels; ++l) {
        const int ws = bp.wside[l];
        if (ws == 0) continue;
        const int lev = a.level[l];
        const int sh = bp.fine - lev;
        const int G = 1 << lev;
        const float *wl = win + bp.woff[l];
        for (int e = threadIdx.x; e < ws * ws * ws * F; e += blockDim.x) {
            const float val = wl[e];
            if (val == 0.0f) continue;
            const int pt = e / F, j = e - pt * F;
            const int wz = pt % ws, wy = (pt / ws) % ws, wx = pt / (ws * ws);
            const int x = (org[0] >> sh) + wx, y = (org[1] >> sh) + wy, z = (org[2] >> sh) + wz;
            if (x > G || y > G || z > G) continue;
            const int64_t row = oct_row(a.corner[l], lev, x, y, z);
            if (row < 0 || row >= a.rows[l]) continue;
            atomicAdd(&a.grad[l][row * F + j], val);
        }
    }
}

// ---- coordinate backward (gather) -------------------------------------------------------------------------------------
// grad = 0; per level, d_k = <row_k, g> (channels ascending), then per axis grad += (G / 2) * sum_k sign_k * (the other two
// axes' weights) * d_k, k ascending.
__global__ __launch_bounds__(256) void octree_coord_grad_kernel(OctreeArgs a, int sum, const float *__restrict__ coords,
                                                                const float *__restrict__ grad_out,
                                                                float *__restrict__ grad_coords, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int F = a.fdim;
    const float c[3] = {coords[i * 3], coords[i * 3 + 1], coords[i * 3 + 2]};
    const int gstride = sum ? F : a.num_levels * F;
    float grad[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int l = 0; l < a.num_levels; ++l) {
        OctCell q;
        int64_t r[4];
        if (!(oct_locate(a.level[l], c, q) && oct_occupied(a.occ[l], a.level[l], q) && oct_edge_rows(a, l, q, r))) continue;
        const float *g = grad_out + i * (int64_t)gstride + (sum ? 0 : l * F);
        const float *tab = a.table[l];
        float d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float *src = tab + (r[k >> 1] + (k & 1)) * F;
            float s = 0.0f;
            for (int j = 0; j < F; ++j) s += src[j] * g[j];
            d[k] = s;
        }
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float wx = (k & 4) ? q.tx : 1.0f - q.tx;
            const float wy = (k & 2) ? q.ty : 1.0f - q.ty;
            const float wz = (k & 1) ? q.tz : 1.0f - q.tz;
            gx += ((k & 4) ? d[k] : -d[k]) * (wy * wz);
            gy += ((k & 2) ? d[k] : -d[k]) * (wx * wz);
            gz += ((k & 1) ? d[k] : -d[k]) * (wx * wy);
        }
        const float h = (float)(1 << a.level[l]) * 0.5f;
        grad[0] += h * gx;
        grad[1] += h * gy;
        grad[2] += h * gz;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) grad_coords[i * 3 + d] = grad[d];
}

// ------------------------------------------------------------------------------------------------------- host side
template <bool SUM>
static void launch_fwd(const OctreeArgs &a, const float *coords, float *feats, int64_t n, hipStream_t s) {
    const dim3 grid((uint32_t)((n + 255) / 256)), block(256);
    switch (a.fdim) {
#define OCT_F(FV) \
    case FV: hipLaunchKernelGGL((octree_fwd_kernel<FV, SUM>), grid, block, 0, s, a, coords, feats, n); return;
        OCT_F(1) OCT_F(2) OCT_F(4) OCT_F(5) OCT_F(8) OCT_F(16)
#undef OCT_F
        default: hipLaunchKernelGGL((octree_fwd_kernel<0, SUM>), grid, block, 0, s, a, coords, feats, n);
    }
}

hipError_t octree_forward_dispatch(const OctreeArgs &a, const float *coords, int sum, float *feats, int64_t n,
                                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (sum) launch_fwd<true>(a, coords, feats, n, s);
    else launch_fwd<false>(a, coords, feats, n, s);
    return hipGetLastError();
}

// the sort's block grid and every level's window (host, from the shape alone)
void octree_backward_plan(const OctreeArgs &a, int sum, OctBwdPlan &bp) {
    int fine = 0;
    for (int l = 0; l < a.num_levels; ++l) fine = std::max(fine, a.level[l]);
    const int64_t budget = kOctLdsBytes / (int64_t)sizeof(float);
    const auto side = [&](int l, int c) { return std::max(1, (1 << c) >> (fine - a.level[l])) + 1; };
    const auto total = [&](int c) {
        int64_t t = 0;
        for (int l = 0; l < a.num_levels; ++l) t += (int64_t)side(l, c) * side(l, c) * side(l, c) * a.fdim;
        return t;
    };
    int c = std::min(fine, kOctMaxCellsLog2);   // the largest block whose windows all fit ...
    while (c > 0 && total(c) > budget) --c;
    int nb = 1 << (fine - c);
    if (nb > kBlockSortMaxBlocksAxis) {         // ... unless that makes more blocks than the sort takes
        nb = kBlockSortMaxBlocksAxis;
        c = fine - 6;
    }
    bp.fine = fine;
    bp.cells_log2 = c;
    bp.nb = nb;
    bp.nbins = nb * nb * nb;
    bp.sum = sum;
    // windows coarsest level first (the most additions per entry); what does not fit adds to memory
    int order[SHACIRA_OCTREE_MAX_LEVELS];
    for (int l = 0; l < a.num_levels; ++l) order[l] = l;
    std::stable_sort(order, order + a.num_levels, [&](int x, int y) { return a.level[x] < a.level[y]; });
    int64_t used = 0;
    for (int o = 0; o < a.num_levels; ++o) {
        const int l = order[o];
        const int w = side(l, c);
        const int64_t need = (int64_t)w * w * w * a.fdim;
        if (used + need <= budget) {
            bp.wside[l] = w;
            bp.woff[l] = (int32_t)used;
            used += need;
        } else {
            bp.wside[l] = 0;
            bp.woff[l] = 0;
        }
    }
    bp.wtotal = (int32_t)used;
}

size_t octree_backward_workspace(const OctreeArgs &a, int sum, int64_t n) {
    if (n <= 0) return 0;
    OctBwdPlan bp;
    octree_backward_plan(a, sum, bp);
    return block_sort_workspace_bytes(bp.nbins, n);
}

hipError_t octree_backward_dispatch(const OctreeArgs &a, const float *coords, const float *grad_out, int sum,
                                    bool features, float *grad_coords, void *workspace, int64_t n, hipStream_t s) {
    if (n <= 0) {
        if (!features) return hipSuccess;
        hipLaunchKernelGGL(octree_zero_kernel, dim3(1024), dim3(256), 0, s, a, nullptr, 0);
        return hipGetLastError();
    }
    if (grad_coords) {
        hipLaunchKernelGGL(octree_coord_grad_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, a, sum, coords,
                           grad_out, grad_coords, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (!features) return hipSuccess;
    OctBwdPlan bp;
    octree_backward_plan(a, sum, bp);
    const BlockSortBuffers buf = block_sort_carve(workspace, bp.nbins);
    hipLaunchKernelGGL(octree_zero_kernel, dim3(1024), dim3(256), 0, s, a, buf.hist, bp.nbins);
    const uint32_t units =
        block_sort_launch<kOctChunk>(OctBlockOf{bp.fine, bp.cells_log2, bp.nb}, coords, n, bp.nbins, buf, s);
    static PerDeviceOnce once;
    if (hipError_t e = once.run([] {
            return hipFuncSetAttribute(reinterpret_cast<const void *>(octree_accum_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kOctLdsBytes);
        }))
        return e;
    hipLaunchKernelGGL(octree_accum_kernel, dim3(units), dim3(256), (size_t)bp.wtotal * sizeof(float), s, a, bp, coords,
                       grad_out, buf.sorted, buf.start, buf.ustart);
    return hipGetLastError();
}

}  // namespace shacira
