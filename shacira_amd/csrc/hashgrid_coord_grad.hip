// hashgrid_coord_grad.hip -- gradient of the hash-grid features with respect to the input coordinates (gfx950).
//
// grad_coords[n, a] = sum_l s_l,a * sum_f g[n,l,f] * sum_{corner pairs (k0, k1 = k0 + axis a)} W_a(k0) * (t[k1,f] - t[k0,f])
// (the contract and its evaluation order: include/shacira_hip.h above shacira_hashgrid_coords_backward). A gather with no
// atomics: the corner rows of the forward plus one grad_output row per sample in, DIM floats per sample out. Every kernel
// below evaluates the same expression tree (coord_level_sums + the level chain), so the result for a sample depends on that
// sample alone and all variants agree bit for bit (coord_feature_diffs: hashgrid_coord_terms.h):
//   variant 0  lane = sample, every level in turn; any even F (runtime F), fp64 tables   [default: calls without a plan]
//   variant 3  lane pair = sample: lane dx gathers the corners x + dx (one request for the x / x+1 pair, the forward's
//              variant 3), the partner's values come over DPP  (measured slower than 0 on every shape: kept for A/B)
//   variant 8  variant 3 over the sorted records of the batch's plan (the forward's rows kernel order: neighbouring samples
//              share coarse-level lines in L1), results go to grad_coords[perm[i]]         [default: 3-D calls with a plan]
// (option "coord_variant"; -1 = the rule above, measured in profiles/coord_grad.md. DESIGN.md 4.3a.)
#include "hashgrid_coord_terms.h"
#include "hashgrid_rows.h"
#include "internal.h"

namespace shacira {

// One level, F features: S[a] = g0 * D0[a], then S[a] = fmaf(g_f, D_f[a], S[a]) for f ascending.
template <int DIM, int F>
__device__ __forceinline__ void coord_level_sums(const float (&f)[DIM], const float (&g)[DIM], const float (&cv)[1 << DIM][F],
                                                 const float (&go)[F], float (&S)[DIM]) {
#pragma unroll
    for (int j = 0; j < F; ++j) {
        float col[1 << DIM], D[DIM];
#pragma unroll
        for (int k = 0; k < (1 << DIM); ++k) col[k] = cv[k][j];
        coord_feature_diffs<DIM>(f, g, col, D);
#pragma unroll
        for (int a = 0; a < DIM; ++a) S[a] = (j == 0) ? go[j] * D[a] : fmaf(go[j], D[a], S[a]);
    }
}

// The level chain: grad[a] = fmaf(s_l,a, S_l,a, grad[a]) from grad = 0, levels ascending.
template <int DIM>
__device__ __forceinline__ void coord_level_chain(const double (&t)[DIM], int32_t res, float hi, const float (&S)[DIM],
                                                  float (&grad)[DIM]) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) grad[a] = fmaf(axis_slope(t[a], res, hi), S[a], grad[a]);
}

// Variant 0: one lane per sample. F > 0: compile-time feature_dim, vector row loads; F == 0: runtime feature_dim (any even
// value; fp64 tables; grad_output not aligned to a whole row piece), scalar loads.
template <int DIM, typename T, int F>
__global__ __launch_bounds__(256) void hashgrid_coord_grad_kernel(LevelTable lt, const int32_t *__restrict__ first_idx,
                                                                  const float *__restrict__ coords,
                                                                  const T *__restrict__ table,
                                                                  const T *__restrict__ grad_out,
                                                                  float *__restrict__ grad_coords, int64_t N) {
    constexpr int NC = 1 << DIM;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double t[DIM];
    load_unit_coords<DIM>(coords, i, N, t);
    const int L = lt.num_lods;
    const int Fr = F > 0 ? F : lt.feature_dim;
    const T *grow = grad_out + i * (int64_t)L * Fr;
    float grad[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) grad[a] = 0.0f;
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        Corners<DIM> c;
        float f[DIM], g[DIM];
        compute_corners<DIM>(t, lt.res[l], lt.hi[l], lt.dense[l] != 0, lt.mask, c, f, g);
        const int64_t base = (int64_t)first_idx[l];
        float S[DIM];
        if constexpr (F > 0) {
            float cv[NC][F], go[F];
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int64_t row = base + (int64_t)c.row[k];
                gather_row<T, F>(table, row, (uint64_t)row < (uint64_t)lt.table_rows, cv[k]);
            }
            load_row<T, F>(grow + (int64_t)l * F, go);
            coord_level_sums<DIM, F>(f, g, cv, go, S);
        } else {
            for (int j = 0; j < Fr; ++j) {
                float col[NC], D[DIM];
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const int64_t row = base + (int64_t)c.row[k];
                    col[k] = ((uint64_t)row < (uint64_t)lt.table_rows) ? Scalar<T>::load(table + row * Fr + j) : 0.0f;
                }
                coord_feature_diffs<DIM>(f, g, col, D);
                const float gj = Scalar<T>::load(grow + (int64_t)l * Fr + j);
#pragma unroll
                for (int a = 0; a < DIM; ++a) S[a] = (j == 0) ? gj * D[a] : fmaf(gj, D[a], S[a]);
            }
        }
        coord_level_chain<DIM>(t, lt.res[l], lt.hi[l], S, grad);
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) grad_coords[i * DIM + a] = grad[a];
}

// Variants 3 / 8: two adjacent lanes per sample, lane dx gathers the corners whose x bit is dx (x and x + 1 of a cell are
// neighbouring rows on dense levels and rows that differ in low bits on hashed ones: one wave request serves both). The even
// lane pulls its partner's values with DPP (quad_perm [1,0,3,2]) and evaluates the level. SORTED: samples in the order of
// the plan's records {x, y, z, bit pattern of the sample's index}, the result row goes to that index.
template <int DIM, typename T, int F, bool SORTED>
__global__ __launch_bounds__(256) void hashgrid_coord_grad_pair_kernel(LevelTable lt, const int32_t *__restrict__ first_idx,
                                                                       const float *__restrict__ coords,
                                                                       const float4 *__restrict__ sorted4,
                                                                       const T *__restrict__ table,
                                                                       const T *__restrict__ grad_out,
                                                                       float *__restrict__ grad_coords, int64_t N) {
    constexpr int NC = 1 << DIM;
    constexpr int NH = NC / 2;
    const int dx = threadIdx.x & 1;
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
    const bool live = i < N;   // (dead lanes run on: their partner's DPP needs them; nothing of theirs is stored)
    double t[DIM];
    int64_t n;
    if constexpr (SORTED) {
        const float4 c4 = sorted4[live ? i : N - 1];
        t[0] = axis_unit(c4.x);
        t[1] = axis_unit(c4.y);
        if constexpr (DIM == 3) t[2] = axis_unit(c4.z);
        n = (int64_t)__builtin_bit_cast(uint32_t, c4.w);
    } else {
        load_unit_coords<DIM>(coords, i, N, t);
        n = live ? i : N - 1;
    }
    const int L = lt.num_lods;
    const T *grow = grad_out + n * (int64_t)L * F;
    float grad[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) grad[a] = 0.0f;
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        Corners<DIM> c;
        float f[DIM], g[DIM];
        compute_corners<DIM>(t, lt.res[l], lt.hi[l], lt.dense[l] != 0, lt.mask, c, f, g);
        const int64_t base = (int64_t)first_idx[l];
        float v[NH][F], go[F];
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            const int64_t row = base + (int64_t)c.row[dx * NH + q];
            gather_row<T, F>(table, row, live && (uint64_t)row < (uint64_t)lt.table_rows, v[q]);
        }
        load_row<T, F>(grow + (int64_t)l * F, go);
        float pv[NH][F];
#pragma unroll
        for (int q = 0; q < NH; ++q)
#pragma unroll
            for (int j = 0; j < F; ++j)
                pv[q][j] = __builtin_bit_cast(
                    float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v[q][j]), 0xB1, 0xF, 0xF, true));
        if (dx == 0) {
            float cv[NC][F], S[DIM];
#pragma unroll
            for (int q = 0; q < NH; ++q)
#pragma unroll
                for (int j = 0; j < F; ++j) {
                    cv[q][j] = v[q][j];
                    cv[NH + q][j] = pv[q][j];
                }
            coord_level_sums<DIM, F>(f, g, cv, go, S);
            coord_level_chain<DIM>(t, lt.res[l], lt.hi[l], S, grad);
        }
    }
    if (dx == 0 && live) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) grad_coords[n * DIM + a] = grad[a];
    }
}

// ----------------------------------------------------------------------------------------------- host side
template <int DIM, typename T, int F>
static hipError_t launch_coord_grad(const LevelTable &lt, const int32_t *first_idx, const float *coords,
                                    const SortedBatch *sb, const void *table, const void *grad_out, float *grad_coords,
                                    int64_t n, hipStream_t s) {
    const T *tab = static_cast<const T *>(table);
    const T *go = static_cast<const T *>(grad_out);
    const int v = opt().coord_variant;
    if constexpr (F > 0) {
        // measured (tools/coord_grad_ab.py): the sorted walk wins where a plan exists (S1 0.89 vs 1.21 ms for variant 0, the
        // nerf_lego table 0.50 vs 0.78); without one, lane pairs lose to a lane per sample (S1 1.30 vs 1.21, config B
        // 0.092 vs 0.071, config D at 65 536 0.088 vs 0.066)
        const bool sorted = sb != nullptr && (v == 8 || (v < 0 && DIM == 3));
        if (sorted || v == 3 || v == 8) {
            const uint32_t blocks = (uint32_t)((2 * n + 255) / 256);
            if (sorted)
                hipLaunchKernelGGL((hashgrid_coord_grad_pair_kernel<DIM, T, F, true>), dim3(blocks), dim3(256), 0, s, lt,
                                   first_idx, coords, sb->sorted4, tab, go, grad_coords, n);
            else
                hipLaunchKernelGGL((hashgrid_coord_grad_pair_kernel<DIM, T, F, false>), dim3(blocks), dim3(256), 0, s, lt,
                                   first_idx, coords, nullptr, tab, go, grad_coords, n);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((hashgrid_coord_grad_kernel<DIM, T, F>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, lt,
                       first_idx, coords, tab, go, grad_coords, n);
    return hipGetLastError();
}

template <int DIM, typename T>
static hipError_t dispatch_coord_f(const LevelTable &lt, const int32_t *first_idx, const float *coords,
                                   const SortedBatch *sb, const void *table, const void *grad_out, float *grad_coords,
                                   int64_t n, hipStream_t s) {
    // the vector row loads of grad_output need rows of whole pieces: a caller's view that starts off a piece boundary
    // takes the scalar path
    const size_t piece = (size_t)lt.feature_dim * sizeof(T);
    const bool aligned = (reinterpret_cast<uintptr_t>(grad_out) % piece) == 0;
    if (aligned && lt.feature_dim == 2)
        return launch_coord_grad<DIM, T, 2>(lt, first_idx, coords, sb, table, grad_out, grad_coords, n, s);
    if (aligned && lt.feature_dim == 4)
        return launch_coord_grad<DIM, T, 4>(lt, first_idx, coords, sb, table, grad_out, grad_coords, n, s);
    return launch_coord_grad<DIM, T, 0>(lt, first_idx, coords, sb, table, grad_out, grad_coords, n, s);
}

hipError_t hashgrid_coord_grad_dispatch(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                        const float *coords, const void *table, const void *grad_out,
                                        float *grad_coords, int64_t n, hipStream_t s, const void *plan) {
    if (n <= 0) return hipSuccess;
    // an empty table has no corner inside it: every difference is zero (and the masked gathers, which read row 0 on behalf
    // of lanes without a row, must not run)
    if (lt.table_rows == 0) return zero_fill_async(grad_coords, n * dim, s);
    SortedBatch sb{};
    if (plan != nullptr) sample_plan_view(dim, n, plan, sb);
    const SortedBatch *psb = plan != nullptr ? &sb : nullptr;
    if (dtype == SHACIRA_F64)
        return dim == 3 ? launch_coord_grad<3, double, 0>(lt, first_idx, coords, nullptr, table, grad_out, grad_coords, n, s)
                        : launch_coord_grad<2, double, 0>(lt, first_idx, coords, nullptr, table, grad_out, grad_coords, n, s);
    if (dim == 3)
        return dtype == SHACIRA_F32
                   ? dispatch_coord_f<3, float>(lt, first_idx, coords, psb, table, grad_out, grad_coords, n, s)
                   : dispatch_coord_f<3, __half>(lt, first_idx, coords, psb, table, grad_out, grad_coords, n, s);
    return dtype == SHACIRA_F32
               ? dispatch_coord_f<2, float>(lt, first_idx, coords, psb, table, grad_out, grad_coords, n, s)
               : dispatch_coord_f<2, __half>(lt, first_idx, coords, psb, table, grad_out, grad_coords, n, s);
}

}  // namespace shacira
