// mesh_sample.hip -- training points on, near and around a mesh, each a pure function of (seed, sample index) (contract in
// include/shacira_hip.h, shacira_mesh_sample / shacira_mesh_sample_count). One lane makes one sample:
//   make_sample   eight Philox4x32-10 words from the counter (index, draw, segment) -- or the caller's eight words --, the face
//                 by an integer binary search in the area CDF, the point in fp32 with one rounding per operator, and the
//                 narrowband test against the packed occupancy of one octree level.
//   count         a workgroup makes 256 consecutive samples and writes how many it keeps.
//   write         makes the same samples again and stores the kept ones at block_offsets[block] + rank, the rank from the
//                 wavefront's ballot and a four-entry LDS prefix: a stable compaction with no intermediate array. Without
//                 block_offsets sample i goes to row i and nothing is ranked.
// Both kernels call the one make_sample, so they cannot disagree on what is kept. The library is built with
// -ffp-contract=off: every product, sum and difference below is rounded once, as written. All address arithmetic is 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"
#include "philox.h"

namespace shacira {

namespace {

constexpr int kSampleBlock = SHACIRA_MESH_SAMPLE_BLOCK;
static_assert(kSampleBlock == 256, "four wavefronts: the LDS prefix has four entries");

struct Float3 {      // 12 bytes, 4-byte aligned: stored as one dwordx3
    float x, y, z;
};

struct Sample {
    float p[3];
    float nrm[3];
    int32_t face;
    bool keep;
};

// the face of word w: the first t with cdf[t] > min(w, cdf[T - 1] - 1), never beyond T - 1. Integers only
__device__ __forceinline__ int32_t face_of(const uint32_t *__restrict__ cdf, int32_t T, uint32_t w) {
    const uint32_t top = cdf[T - 1] - 1u;        // a zero total wraps to 0xFFFFFFFF: nothing is found, the clamp below holds
    w = w < top ? w : top;
    int32_t lo = 0, hi = T - 1;                  // the answer is in [lo, hi]
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > w)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ Sample make_sample(const MeshSampleArgs &a, int64_t i) {
    Sample s;
    s.face = -1;
    s.nrm[0] = s.nrm[1] = s.nrm[2] = 0.0f;
    const int64_t idx = a.index_base + i;
    uint32_t w[4];
    if (a.words) {
        const uint32_t *src = a.words + i * 8;
        w[0] = src[0], w[1] = src[1], w[2] = src[2], w[3] = src[3];
    } else {
        philox4x32_10((uint32_t)idx, (uint32_t)((uint64_t)idx >> 32), 0u, a.segment, a.key0, a.key1, w);
    }
    if (a.mode == SHACIRA_MESH_SAMPLE_CUBE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.p[k] = unit_open_above(w[k]) * 2.0f - 1.0f;
    } else if (a.mode == SHACIRA_MESH_SAMPLE_CELLS) {
        const int64_t cell = (int64_t)((uint32_t)i / (uint32_t)a.samples_per_cell);      // n < 2^31
        const int16_t *c = a.corners + cell * 3;
        const float width = 2.0f / (float)(1 << a.cell_level);                            // exact
#pragma unroll
        for (int k = 0; k < 3; ++k) s.p[k] = ((float)c[k] * width - 1.0f) + unit_open_above(w[k]) * width;
    } else {
        const int32_t t = face_of(a.cdf, (int32_t)a.num_triangles, w[0]);
        s.face = t;
        const float *v = a.triangles + (int64_t)t * 9;
        float va[3], vb[3], vc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) va[k] = v[k], vb[k] = v[3 + k], vc[k] = v[6 + k];
        const float u = sqrtf(unit_open_above(w[1])), vv = unit_open_above(w[2]);
        const float wa = 1.0f - u, wb = u * (1.0f - vv), wc = u * vv;
#pragma unroll
        for (int k = 0; k < 3; ++k) s.p[k] = (wa * va[k] + wb * vb[k]) + wc * vc[k];
        const float x[3] = {va[0] - vb[0], va[1] - vb[1], va[2] - vb[2]};
        const float y[3] = {vb[0] - vc[0], vb[1] - vc[1], vb[2] - vc[2]};
        s.nrm[0] = x[1] * y[2] - x[2] * y[1];
        s.nrm[1] = x[2] * y[0] - x[0] * y[2];
        s.nrm[2] = x[0] * y[1] - x[1] * y[0];
        if (a.mode == SHACIRA_MESH_SAMPLE_NEAR) {
            uint32_t g[4];
            if (a.words) {
                const uint32_t *src = a.words + i * 8 + 4;
                g[0] = src[0], g[1] = src[1], g[2] = src[2], g[3] = src[3];
            } else {
                philox4x32_10((uint32_t)idx, (uint32_t)((uint64_t)idx >> 32), 1u, a.segment, a.key0, a.key1, g);
            }
            float z[3];
            box_muller3(g, z);
            s.p[0] = s.p[0] + a.sigma * z[0];
            s.p[1] = s.p[1] + a.sigma * z[1];
            s.p[2] = s.p[2] + a.sigma * z[2];
        }
    }
    s.keep = true;
    if (a.occupancy) {
        const int32_t G = 1 << a.occupancy_level;
        const float fg = (float)G;
        bool in = true;
        int32_t q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float cell = floorf((fg * (s.p[k] + 1.0f)) / 2.0f);
            in = in && cell >= 0.0f && cell < fg;            // false for NaN
            q[k] = in ? (int32_t)cell : 0;
        }
        const uint32_t key = ((uint32_t)q[0] * (uint32_t)G + (uint32_t)q[1]) * (uint32_t)G + (uint32_t)q[2];   // < 2^30
        s.keep = in && ((a.occupancy[key >> 5] >> (key & 31u)) & 1u);
    }
    return s;
}

// kCount: write the number of kept samples of the workgroup's 256 indices, and nothing else
template <bool kCount>
__global__ void __launch_bounds__(kSampleBlock) mesh_sample_kernel(const MeshSampleArgs a, int32_t *__restrict__ block_counts,
                                                                   const int64_t *__restrict__ block_offsets,
                                                                   Float3 *__restrict__ points, Float3 *__restrict__ normals,
                                                                   int32_t *__restrict__ face_idx,
                                                                   int64_t *__restrict__ source_idx) {
    __shared__ int32_t wave_kept[kSampleBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kSampleBlock + threadIdx.x;
    const bool live = i < a.n;
    Sample s;
    s.keep = false;
    if (live) s = make_sample(a, i);
    if (!kCount && !block_offsets) {                       // uniform: the unfiltered form, row i
        if (live) {
            points[i] = Float3{s.p[0], s.p[1], s.p[2]};
            if (normals) normals[i] = Float3{s.nrm[0], s.nrm[1], s.nrm[2]};
            if (face_idx) face_idx[i] = s.face;
            if (source_idx) source_idx[i] = i;
        }
        return;
    }
    // every lane of every wavefront arrives here
    const uint64_t kept = __ballot(live && s.keep);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (lane == 0) wave_kept[wave] = __popcll(kept);
    __syncthreads();
    if (kCount) {
        if (threadIdx.x == 0) block_counts[blockIdx.x] = (wave_kept[0] + wave_kept[1]) + (wave_kept[2] + wave_kept[3]);
        return;
    }
    if (!(live && s.keep)) return;
    int64_t row = block_offsets[blockIdx.x];
    for (int v = 0; v < wave; ++v) row += wave_kept[v];
    row += __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
    points[row] = Float3{s.p[0], s.p[1], s.p[2]};
    if (normals) normals[row] = Float3{s.nrm[0], s.nrm[1], s.nrm[2]};
    if (face_idx) face_idx[row] = s.face;
    if (source_idx) source_idx[row] = i;
}

}  // namespace

hipError_t mesh_sample_count_dispatch(const MeshSampleArgs &a, int32_t *block_counts, hipStream_t s) {
    const dim3 grid((uint32_t)((a.n + kSampleBlock - 1) / kSampleBlock)), block(kSampleBlock);
    hipLaunchKernelGGL(mesh_sample_kernel<true>, grid, block, 0, s, a, block_counts, (const int64_t *)nullptr,
                       (Float3 *)nullptr, (Float3 *)nullptr, (int32_t *)nullptr, (int64_t *)nullptr);
    return hipGetLastError();
}

hipError_t mesh_sample_write_dispatch(const MeshSampleArgs &a, const int64_t *block_offsets, float *points, float *normals,
                                      int32_t *face_idx, int64_t *source_idx, hipStream_t s) {
    const dim3 grid((uint32_t)((a.n + kSampleBlock - 1) / kSampleBlock)), block(kSampleBlock);
    hipLaunchKernelGGL(mesh_sample_kernel<false>, grid, block, 0, s, a, (int32_t *)nullptr, block_offsets,
                       reinterpret_cast<Float3 *>(points), reinterpret_cast<Float3 *>(normals), face_idx, source_idx);
    return hipGetLastError();
}

}  // namespace shacira
