// hashgrid_coord_grad2.hip -- backward of the coordinate backward of the hash-grid lookup (gfx950): second order, opt-in.
//
// The node differentiated is shacira_hashgrid_coords_backward, gc[n,a] = sum_l s_l,a sum_f g[n,l,f] sum_k sigma_a(k) W_a(k) t[k,f].
// Given v = dL/dgc (fp32 [N, dim]) the three results are (contract and evaluation order: include/shacira_hip.h above
// shacira_hashgrid_coords_backward2):
//   (1) grad_grad_output[n,l,f] = sum_a v_a s_l,a sum_k sigma_a(k) W_a(k) t[k,f]              gather, no atomics
//   (2) grad_codebook[first_l + row_k, f] += g[n,l,f] * sum_a v_a s_l,a sigma_a(k) W_a(k)     scatter-add (float atomics)
//   (3) grad_coords[n,b] = sum_l sum_{a != b} v_a s_l,a s_l,b sum_f g[n,l,f] sum_k sigma_a(k) sigma_b(k) W_ab(k) t[k,f]   gather
// (1) and (3) share one gather kernel (lane = sample, every level in turn; one or both outputs); with the batch's plan a 3-D
// call walks the samples in the order of the plan's sorted records. Both orders and every instantiation evaluate the same
// expression trees (hashgrid_coord_terms.h + the chains below): a sample's result depends on that sample alone.
// (2) has the lane-group form of hashgrid_bwd.hip: lanes = (sample, level, x offset, feature), the adds of one row leave as
// one request. Measurements: profiles/coord_grad2.md.
#include "hashgrid_coord_terms.h"
#include "hashgrid_rows.h"
#include "internal.h"

namespace shacira {

// one output row as a single vector store where the row is a whole piece (compile-time F), the half values rounded from
// the finished fp32 value (Scalar<__half>::store's two-step rounding)
template <typename T, int F> __device__ __forceinline__ void store_row(T *p, const float (&v)[F]) {
    if constexpr (sizeof(T) == 4 && F == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else if constexpr (sizeof(T) == 4 && F == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (sizeof(T) == 2 && F == 2) {
        *reinterpret_cast<__half2 *>(p) = __halves2half2(__float2half_rn(Scalar<__half>::rounded_fp32(v[0])),
                                                         __float2half_rn(Scalar<__half>::rounded_fp32(v[1])));
    } else {
#pragma unroll
        for (int j = 0; j < F; ++j) Scalar<T>::store(p + j, v[j]);
    }
}

// (1), one feature: R = c_0 * D[0], then fmaf(c_a, D[a], R) for a ascending; c_a = v_a * s_l,a.
template <int DIM> __device__ __forceinline__ float directional_feature(const float (&c)[DIM], const float (&D)[DIM]) {
    float r = c[0] * D[0];
#pragma unroll
    for (int a = 1; a < DIM; ++a) r = fmaf(c[a], D[a], r);
    return r;
}

// (3), one level: inner[b] = c_a * P[pair(a, b)] over a != b ascending (first a product, then fmaf), then
// out[b] = fmaf(s_l,b, inner[b], out[b]).
template <int DIM>
__device__ __forceinline__ void mixed_level_chain(const float (&c)[DIM], const float (&s)[DIM],
                                                  const float (&P)[AxisPairs<DIM>::N], float (&out)[DIM]) {
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
        float inner = 0.0f;
        bool first = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            if (a == b) continue;
            const float p = P[a < b ? axis_pair(a, b) : axis_pair(b, a)];
            inner = first ? c[a] * p : fmaf(c[a], p, inner);
            first = false;
        }
        out[b] = fmaf(s[b], inner, out[b]);
    }
}

// Gather kernel of (1) and (3). G1 / G3: which outputs are written. F > 0: compile-time feature_dim, vector row accesses;
// F == 0: runtime feature_dim (any even value, or rows not aligned to a whole piece), scalar accesses. SORTED: samples in the
// order of the plan's records {x, y, z, bit pattern of the sample's index}; every row read or written is that index's.
template <int DIM, typename T, int F, bool G1, bool G3, bool SORTED>
__global__ __launch_bounds__(256) void hashgrid_coord_grad2_kernel(LevelTable lt, const int32_t *__restrict__ first_idx,
                                                                   const float *__restrict__ coords,
                                                                   const float4 *__restrict__ sorted4,
                                                                   const T *__restrict__ table,
                                                                   const T *__restrict__ grad_out,
                                                                   const float *__restrict__ vv, T *__restrict__ ggo,
                                                                   float *__restrict__ grad_coords, int64_t N) {
    constexpr int NC = 1 << DIM;
    constexpr int NP = AxisPairs<DIM>::N;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double t[DIM];
    int64_t n = i;
    if constexpr (SORTED) {
        const float4 c4 = sorted4[i];
        t[0] = axis_unit(c4.x);
        t[1] = axis_unit(c4.y);
        if constexpr (DIM == 3) t[2] = axis_unit(c4.z);
        n = (int64_t)__builtin_bit_cast(uint32_t, c4.w);
    } else {
        load_unit_coords<DIM>(coords, i, N, t);
    }
    float v[DIM], out[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        v[a] = vv[n * DIM + a];
        out[a] = 0.0f;
    }
    const int L = lt.num_lods;
    const int Fr = F > 0 ? F : lt.feature_dim;
    const int64_t rowbase = n * (int64_t)L * Fr;
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        Corners<DIM> cn;
        float f[DIM], g[DIM], s[DIM], c[DIM];
        compute_corners<DIM>(t, lt.res[l], lt.hi[l], lt.dense[l] != 0, lt.mask, cn, f, g);
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            s[a] = axis_slope(t[a], lt.res[l], lt.hi[l]);
            c[a] = v[a] * s[a];
        }
        const int64_t base = (int64_t)first_idx[l];
        float P[NP];
        if constexpr (F > 0) {
            float cv[NC][F], go[F], r[F];
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int64_t row = base + (int64_t)cn.row[k];
                gather_row<T, F>(table, row, (uint64_t)row < (uint64_t)lt.table_rows, cv[k]);
            }
            if constexpr (G3) load_row<T, F>(grad_out + rowbase + (int64_t)l * F, go);
#pragma unroll
            for (int j = 0; j < F; ++j) {
                float col[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) col[k] = cv[k][j];
                if constexpr (G1) {
                    float D[DIM];
                    coord_feature_diffs<DIM>(f, g, col, D);
                    r[j] = directional_feature<DIM>(c, D);
                }
                if constexpr (G3) {
                    float M[NP];
                    coord_feature_mixed<DIM>(f, g, col, M);
#pragma unroll
                    for (int p = 0; p < NP; ++p) P[p] = (j == 0) ? go[j] * M[p] : fmaf(go[j], M[p], P[p]);
                }
            }
            if constexpr (G1) store_row<T, F>(ggo + rowbase + (int64_t)l * F, r);
        } else {
            for (int j = 0; j < Fr; ++j) {
                float col[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int64_t row = base + (int64_t)cn.row[k];
                    col[k] = ((uint64_t)row < (uint64_t)lt.table_rows) ? Scalar<T>::load(table + row * Fr + j) : 0.0f;
                }
                if constexpr (G1) {
                    float D[DIM];
                    coord_feature_diffs<DIM>(f, g, col, D);
                    Scalar<T>::store(ggo + rowbase + (int64_t)l * Fr + j, directional_feature<DIM>(c, D));
                }
                if constexpr (G3) {
                    float M[NP];
                    coord_feature_mixed<DIM>(f, g, col, M);
                    const float gj = Scalar<T>::load(grad_out + rowbase + (int64_t)l * Fr + j);
#pragma unroll
                    for (int p = 0; p < NP; ++p) P[p] = (j == 0) ? gj * M[p] : fmaf(gj, M[p], P[p]);
                }
            }
        }
        if constexpr (G3) mixed_level_chain<DIM>(c, s, P, out);
    }
    if constexpr (G3) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) grad_coords[n * DIM + a] = out[a];
    }
}

// (2): the directional derivative of every corner weight, dw[k] = sum_a c_a sigma_a(k) W_a(k), c_a = v_a * s_l,a.
template <int DIM>
__device__ __forceinline__ void directional_weights(const float (&f)[DIM], const float (&g)[DIM], const float (&c)[DIM],
                                                    float (&dw)[1 << DIM]) {
#pragma unroll
    for (int k = 0; k < (1 << DIM); ++k) {
        float acc = 0.0f;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            float w = c[a];
#pragma unroll
            for (int b = 0; b < DIM; ++b)
                if (b != a) w *= (k & (1 << (DIM - 1 - b))) ? f[b] : g[b];
            acc += (k & (1 << (DIM - 1 - a))) ? w : -w;
        }
        dw[k] = acc;
    }
}

// The same for the corners of one x offset only (the lane-group scatter: a lane owns x or x + 1): wx = the x weight of that
// offset, sx = its sigma_x; q runs over the other axes' corner bits.
template <int DIM>
__device__ __forceinline__ void directional_weights_x(const float (&f)[DIM], const float (&g)[DIM], const float (&c)[DIM],
                                                      float wx, float sx, float (&dw)[1 << (DIM - 1)]) {
#pragma unroll
    for (int q = 0; q < (1 << (DIM - 1)); ++q) {
        float acc = 0.0f;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            float w = c[a];
#pragma unroll
            for (int b = 0; b < DIM; ++b)
                if (b != a) w *= (b == 0) ? wx : ((q & (1 << (DIM - 1 - b))) ? f[b] : g[b]);
            acc += (a == 0) ? sx * w : ((q & (1 << (DIM - 1 - a))) ? w : -w);
        }
        dw[q] = acc;
    }
}

// the level table in LDS: the level is a per-lane index here (hashgrid_bwd.hip does the same)
struct LevelLds {
    int32_t res[SHACIRA_MAX_LODS];
    float hi[SHACIRA_MAX_LODS];
    int32_t first[SHACIRA_MAX_LODS];
    uint32_t dense[SHACIRA_MAX_LODS];
};
__device__ __forceinline__ void stage_levels(const LevelTable &lt, const int32_t *__restrict__ first_idx, LevelLds &sl) {
    if (threadIdx.x < (uint32_t)lt.num_lods) {
        sl.res[threadIdx.x] = lt.res[threadIdx.x];
        sl.hi[threadIdx.x] = lt.hi[threadIdx.x];
        sl.dense[threadIdx.x] = lt.dense[threadIdx.x];
        sl.first[threadIdx.x] = first_idx[threadIdx.x];
    }
    __syncthreads();
}

template <int DIM>
__device__ __forceinline__ void sample_level_weights(int32_t res, float hi, bool dense, uint32_t mask,
                                                     const float *__restrict__ coords, const float *__restrict__ vv,
                                                     int64_t i, Corners<DIM> &cn, float (&dw)[1 << DIM]) {
    double t[DIM];
    float f[DIM], g[DIM], c[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) t[a] = axis_unit(coords[i * DIM + a]);
    compute_corners<DIM>(t, res, hi, dense, mask, cn, f, g);
#pragma unroll
    for (int a = 0; a < DIM; ++a) c[a] = vv[i * DIM + a] * axis_slope(t[a], res, hi);
    directional_weights<DIM>(f, g, c, dw);
}

// F = 2 / 4: 2 F lanes per (sample, level) = (x offset, feature); the grid covers every lane (launch_scatter2 keeps
// items * 2 F below 2^31). A zero weight (clamped axes, v = 0) adds nothing and is skipped: untouched rows stay exactly 0.
template <int DIM, typename T, int F>
__global__ __launch_bounds__(256) void hashgrid_coord_grad2_scatter_kernel(LevelTable lt,
                                                                           const int32_t *__restrict__ first_idx,
                                                                           const float *__restrict__ coords,
                                                                           const T *__restrict__ grad_out,
                                                                           const float *__restrict__ vv,
                                                                           float *__restrict__ acc, int64_t sample0,
                                                                           uint32_t num_items) {
    constexpr int NC = 1 << DIM;
    static_assert(F == 2 || F == 4, "2 F lanes per (sample, level)");
    constexpr uint32_t LOGF = (F == 2) ? 1u : 2u;
    const uint32_t L = (uint32_t)lt.num_lods;
    __shared__ LevelLds sl;
    stage_levels(lt, first_idx, sl);
    const uint32_t t2 = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t w = t2 >> (LOGF + 1u), dx = (t2 >> LOGF) & 1u, j = t2 & (uint32_t)(F - 1);
    if (w >= num_items) return;
    const uint32_t sm = w / L;
    const uint32_t lvl = w - sm * L;
    const int64_t i = sample0 + sm;
    const int32_t res = sl.res[lvl];
    const float hi = sl.hi[lvl];
    double t[DIM];
    float f[DIM], g[DIM], c[DIM], dw[NC / 2];
    Corners<DIM> cn;
#pragma unroll
    for (int a = 0; a < DIM; ++a) t[a] = axis_unit(coords[i * DIM + a]);
    compute_corners<DIM>(t, res, hi, sl.dense[lvl] != 0, lt.mask, cn, f, g);
#pragma unroll
    for (int a = 0; a < DIM; ++a) c[a] = vv[i * DIM + a] * axis_slope(t[a], res, hi);
    directional_weights_x<DIM>(f, g, c, dx ? f[0] : g[0], dx ? 1.0f : -1.0f, dw);
    const int64_t base = (int64_t)sl.first[lvl];
    const float gj = Scalar<T>::load(grad_out + (i * L + lvl) * F + j);
#pragma unroll
    for (int q = 0; q < NC / 2; ++q) {   // corner bit (DIM - 1) is the x offset
        const uint32_t r = dx ? cn.row[q | (NC / 2)] : cn.row[q];
        const int64_t row = base + (int64_t)r;
        if ((uint64_t)row < (uint64_t)lt.table_rows && dw[q] != 0.0f) unsafeAtomicAdd(acc + row * F + j, gj * dw[q]);
    }
}

// any other (even) feature count: one lane per (sample, level)
template <int DIM, typename T>
__global__ __launch_bounds__(256) void hashgrid_coord_grad2_scatter_any_kernel(LevelTable lt,
                                                                               const int32_t *__restrict__ first_idx,
                                                                               const float *__restrict__ coords,
                                                                               const T *__restrict__ grad_out,
                                                                               const float *__restrict__ vv,
                                                                               float *__restrict__ acc, int64_t sample0,
                                                                               uint32_t num_items) {
    constexpr int NC = 1 << DIM;
    const uint32_t L = (uint32_t)lt.num_lods;
    const int Fr = lt.feature_dim;
    __shared__ LevelLds sl;
    stage_levels(lt, first_idx, sl);
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= num_items) return;
    const uint32_t sm = w / L;
    const uint32_t lvl = w - sm * L;
    const int64_t i = sample0 + sm;
    Corners<DIM> cn;
    float dw[NC];
    sample_level_weights<DIM>(sl.res[lvl], sl.hi[lvl], sl.dense[lvl] != 0, lt.mask, coords, vv, i, cn, dw);
    const int64_t base = (int64_t)sl.first[lvl];
    const T *grow = grad_out + (i * L + lvl) * Fr;
    for (int j = 0; j < Fr; ++j) {
        const float gj = Scalar<T>::load(grow + j);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int64_t row = base + (int64_t)cn.row[k];
            if ((uint64_t)row < (uint64_t)lt.table_rows && dw[k] != 0.0f) unsafeAtomicAdd(acc + row * Fr + j, gj * dw[k]);
        }
    }
}

__global__ __launch_bounds__(256) void coord_grad2_f32_to_f16_kernel(const float *__restrict__ src, __half *__restrict__ dst,
                                                                     int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = __float2half_rn(src[i]);
}

// ----------------------------------------------------------------------------------------------- host side
struct Grad2Args {
    const int32_t *first_idx;
    const float *coords;
    const void *table, *grad_out;
    const float *vv;
    void *ggo;
    float *gc;
    int64_t n;
};

template <int DIM, typename T, int F, bool SORTED>
static hipError_t launch_gather2(const LevelTable &lt, const Grad2Args &a, const float4 *sorted4, hipStream_t s) {
    const dim3 grid((uint32_t)((a.n + 255) / 256)), block(256);
    const T *tab = static_cast<const T *>(a.table);
    const T *go = static_cast<const T *>(a.grad_out);
    T *ggo = static_cast<T *>(a.ggo);
    if (a.ggo != nullptr && a.gc != nullptr)
        hipLaunchKernelGGL((hashgrid_coord_grad2_kernel<DIM, T, F, true, true, SORTED>), grid, block, 0, s, lt, a.first_idx,
                           a.coords, sorted4, tab, go, a.vv, ggo, a.gc, a.n);
    else if (a.ggo != nullptr)
        hipLaunchKernelGGL((hashgrid_coord_grad2_kernel<DIM, T, F, true, false, SORTED>), grid, block, 0, s, lt, a.first_idx,
                           a.coords, sorted4, tab, go, a.vv, ggo, a.gc, a.n);
    else
        hipLaunchKernelGGL((hashgrid_coord_grad2_kernel<DIM, T, F, false, true, SORTED>), grid, block, 0, s, lt, a.first_idx,
                           a.coords, sorted4, tab, go, a.vv, ggo, a.gc, a.n);
    return hipGetLastError();
}

template <int DIM, typename T>
static hipError_t dispatch_gather2(const LevelTable &lt, const Grad2Args &a, const SortedBatch *sb, hipStream_t s) {
    // vector row accesses need rows of whole pieces: a view that starts off a piece boundary takes the scalar path
    const size_t piece = (size_t)lt.feature_dim * sizeof(T);
    const bool aligned = (reinterpret_cast<uintptr_t>(a.grad_out) % piece) == 0 && (reinterpret_cast<uintptr_t>(a.ggo) % piece) == 0;
    const int F = aligned ? lt.feature_dim : 0;
    if constexpr (DIM == 3) {
        // the sorted walk is the coordinate backward's rule for 3-D calls with a plan (profiles/coord_grad2.md)
        if (sb != nullptr && F == 2) return launch_gather2<3, T, 2, true>(lt, a, sb->sorted4, s);
        if (sb != nullptr && F == 4) return launch_gather2<3, T, 4, true>(lt, a, sb->sorted4, s);
    }
    if (F == 2) return launch_gather2<DIM, T, 2, false>(lt, a, nullptr, s);
    if (F == 4) return launch_gather2<DIM, T, 4, false>(lt, a, nullptr, s);
    return launch_gather2<DIM, T, 0, false>(lt, a, nullptr, s);
}

template <int DIM, typename T>
static hipError_t launch_scatter2(const LevelTable &lt, const Grad2Args &a, float *acc, hipStream_t s) {
    const int64_t L = lt.num_lods;
    const int F = lt.feature_dim;
    const int64_t max_samples = ((int64_t)1 << (F == 2 ? 29 : F == 4 ? 28 : 31)) / L - 1;
    const T *go = static_cast<const T *>(a.grad_out);
    for (int64_t s0 = 0; s0 < a.n; s0 += max_samples) {
        const int64_t ns = (a.n - s0 < max_samples) ? (a.n - s0) : max_samples;
        const uint32_t items = (uint32_t)(ns * L);
        if (F == 2 || F == 4) {
            const uint32_t blocks = (uint32_t)(((uint64_t)items * (2u * (uint32_t)F) + 255u) / 256u);
            if (F == 2)
                hipLaunchKernelGGL((hashgrid_coord_grad2_scatter_kernel<DIM, T, 2>), dim3(blocks), dim3(256), 0, s, lt,
                                   a.first_idx, a.coords, go, a.vv, acc, s0, items);
            else
                hipLaunchKernelGGL((hashgrid_coord_grad2_scatter_kernel<DIM, T, 4>), dim3(blocks), dim3(256), 0, s, lt,
                                   a.first_idx, a.coords, go, a.vv, acc, s0, items);
        } else {
            hipLaunchKernelGGL((hashgrid_coord_grad2_scatter_any_kernel<DIM, T>), dim3((items + 255u) / 256u), dim3(256), 0, s,
                               lt, a.first_idx, a.coords, go, a.vv, acc, s0, items);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t hashgrid_coord_grad2_dispatch(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                         const float *coords, const void *table, const void *grad_out, const float *vv,
                                         void *ggo, void *grad_table, float *grad_coords, void *workspace, int64_t n,
                                         hipStream_t s, const void *plan) {
    const bool half = dtype == SHACIRA_F16;
    const int64_t numel = lt.table_rows * lt.feature_dim;
    hipError_t e = hipSuccess;
    // (2) overwrites its output: zeroed first, like shacira_hashgrid_backward (fp16: the fp32 image in the workspace; with
    // nothing to add, the half table itself -- feature_dim is even, so it is a whole number of floats)
    float *acc = nullptr;
    if (grad_table != nullptr) {
        const bool adds = n > 0 && numel > 0;
        acc = (half && adds) ? static_cast<float *>(workspace) : static_cast<float *>(grad_table);
        e = zero_fill_async(acc, (half && !adds) ? numel / 2 : numel, s);
        if (e != hipSuccess) return e;
    }
    if (n <= 0) return hipSuccess;
    const int64_t row = (int64_t)lt.num_lods * lt.feature_dim;
    if (lt.table_rows == 0) {   // no corner inside the table: every term is zero (and the masked gathers must not run)
        if (ggo != nullptr) e = zero_fill_async(static_cast<float *>(ggo), half ? n * row / 2 : n * row, s);
        if (e == hipSuccess && grad_coords != nullptr) e = zero_fill_async(grad_coords, n * dim, s);
        return e;
    }
    const Grad2Args a{first_idx, coords, table, grad_out, vv, ggo, grad_coords, n};
    if (ggo != nullptr || grad_coords != nullptr) {
        SortedBatch sbv{};
        if (plan != nullptr) sample_plan_view(dim, n, plan, sbv);
        const SortedBatch *sb = plan != nullptr ? &sbv : nullptr;
        if (dim == 3)
            e = half ? dispatch_gather2<3, __half>(lt, a, sb, s) : dispatch_gather2<3, float>(lt, a, sb, s);
        else
            e = half ? dispatch_gather2<2, __half>(lt, a, nullptr, s) : dispatch_gather2<2, float>(lt, a, nullptr, s);
        if (e != hipSuccess) return e;
    }
    if (grad_table != nullptr) {
        if (dim == 3)
            e = half ? launch_scatter2<3, __half>(lt, a, acc, s) : launch_scatter2<3, float>(lt, a, acc, s);
        else
            e = half ? launch_scatter2<2, __half>(lt, a, acc, s) : launch_scatter2<2, float>(lt, a, acc, s);
        if (e != hipSuccess) return e;
        if (half) {
            int64_t blocks = (numel + 255) / 256;
            if (blocks > 4096) blocks = 4096;
            hipLaunchKernelGGL(coord_grad2_f32_to_f16_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, acc,
                               static_cast<__half *>(grad_table), numel);
            e = hipGetLastError();
        }
    }
    return e;
}

}  // namespace shacira
