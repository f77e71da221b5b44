// mesh_voxelize.hip -- a triangle soup rasterised into the dense occupancy bits of one octree level (contract in
// include/shacira_hip.h, shacira_mesh_voxelize): cell (i, j, k) is set iff a valid triangle overlaps the closed cube of
// half-extent 0.5 + margin around the cell's centre, by the separating-axis test in its projected form (integer bounding box,
// plane slab, three 2-D edge-function triples). The predicate is a function of one (cell, triangle) pair and the combine is an
// OR, so the partition below -- triangle passes, column words, lanes -- cannot change a bit.
//
//   prologue   one thread per triangle writes its VoxRecord (grid-unit vertices, normal, plane radius, nine edge functions,
//              the clipped integer bounding box) and the number of work units of the triangle. Triangles are processed in
//              passes of kVoxPass records so that the record array is bounded (kVoxPass * sizeof(VoxRecord) = 6 MiB).
//   scan       one workgroup turns the pass's unit counts into exclusive 64-bit offsets; the host reads the total back.
//   pair       the work unit is a COLUMN WORD: one (x, y) column of a triangle's bounding box crossed with one 32-bit word
//              of the occupancy (32 z cells; at G < 32 the whole column, which then shares its word with other columns).
//              Every lane takes one unit, finds its triangle by binary search in the offsets, evaluates what is constant along
//              z once, walks the at most 32 cells of the word inside the bounding box and issues at most one atomicOr. A mesh
//              of many triangles smaller than a cell and one triangle spanning the grid take the same path.
//   finish     optional: the uint8 [G][G][G] grid expanded from the words.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "internal.h"

namespace shacira {

namespace {

constexpr int kVoxBlock = 256;
constexpr int kVoxPass = SHACIRA_MESH_VOXELIZE_PASS_TRIANGLES;
constexpr int kVoxScanBlock = 1024;
constexpr int kVoxScanPerThread = kVoxPass / kVoxScanBlock;
constexpr uint64_t kVoxLaunchUnits = 1ull << 30;     // units per pair launch: the grid stays below 2^22 workgroups
static_assert(kVoxPass % kVoxScanBlock == 0, "the scan gives every thread the same number of counts");

struct VoxRecord {                // 48 dwords, 16-byte aligned
    float v[3][3];                // a, b, c in grid units
    float n[3];                   // cross(e0, e1)
    float rn;                     // H * ((|nx| + |ny|) + |nz|)
    float m[3][3][3];             // [projection k][edge i]: mu, mv, r
    int32_t lo[3], hi[3];         // the clipped bounding box in cells, lo > hi on some axis: nothing to mark
    int32_t pad[2];
};
static_assert(sizeof(VoxRecord) == 192, "record layout");

// the contract's fixed shapes; the library is built with -ffp-contract=off, so each operator rounds once
__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// everything of the contract that depends on the triangle alone; returns its number of column words
__device__ __forceinline__ uint64_t vox_setup(const float *__restrict__ t, int level, float margin, VoxRecord &r) {
    const int32_t G = 1 << level;
    const float half = 0.5f * (float)G;
    const float H = 0.5f + margin;
    // the record flag of mesh_sdf.hip on the vertices as given: a non-zero n = cross(b - a, a - c)
    const float e0[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]};
    const float e2[3] = {t[0] - t[6], t[1] - t[7], t[2] - t[8]};
    const float n0 = e0[1] * e2[2] - e0[2] * e2[1];
    const float n1 = e0[2] * e2[0] - e0[0] * e2[2];
    const float n2 = e0[0] * e2[1] - e0[1] * e2[0];
    bool valid = n0 != 0.f || n1 != 0.f || n2 != 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r.v[j][c] = (t[3 * j + c] + 1.0f) * half;
            valid = valid && fabsf(r.v[j][c]) < INFINITY;      // false for a NaN, too
        }
    float e[3][3];                // e0 = b - a, e1 = c - b, e2 = a - c in grid units
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        e[0][c] = r.v[1][c] - r.v[0][c];
        e[1][c] = r.v[2][c] - r.v[1][c];
        e[2][c] = r.v[0][c] - r.v[2][c];
    }
    r.n[0] = e[0][1] * e[1][2] - e[0][2] * e[1][1];
    r.n[1] = e[0][2] * e[1][0] - e[0][0] * e[1][2];
    r.n[2] = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    r.rn = H * ((fabsf(r.n[0]) + fabsf(r.n[1])) + fabsf(r.n[2]));
    // projection k drops axis k: (u, v) = (y, z), (z, x), (x, y); the inward normal of edge i is sigma * (-e_v, e_u)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int u = (k + 1) % 3, w = (k + 2) % 3;
        const bool ccw = r.n[k] >= 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float mu = ccw ? -e[i][w] : e[i][w];
            const float mv = ccw ? e[i][u] : -e[i][u];
            r.m[k][i][0] = mu;
            r.m[k][i][1] = mv;
            r.m[k][i][2] = H * (fabsf(mu) + fabsf(mv));
        }
    }
    // the three cube axes: cell i passes iff lo <= i <= hi, the integers with i + 0.5 inside [min - H, max + H], clipped
    bool empty = !valid;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = fmaxf(ceilf((min3(r.v[0][c], r.v[1][c], r.v[2][c]) - H) - 0.5f), 0.f);
        const float hi = fminf(floorf((max3(r.v[0][c], r.v[1][c], r.v[2][c]) + H) - 0.5f), (float)(G - 1));
        const bool none = !(lo <= hi);
        empty = empty || none;
        r.lo[c] = none ? 1 : (int32_t)lo;        // both inside [0, G - 1] when there is a cell
        r.hi[c] = none ? 0 : (int32_t)hi;
    }
    r.pad[0] = r.pad[1] = 0;
    if (empty) {
        r.lo[0] = 1;
        r.hi[0] = 0;
        return 0;
    }
    const uint64_t words = (uint64_t)((r.hi[2] >> 5) - (r.lo[2] >> 5) + 1);
    return (uint64_t)(r.hi[0] - r.lo[0] + 1) * (uint64_t)(r.hi[1] - r.lo[1] + 1) * words;
}

__global__ void __launch_bounds__(kVoxBlock) vox_prologue_kernel(const float *__restrict__ tris, int level, float margin,
                                                                 VoxRecord *__restrict__ rec, uint64_t *__restrict__ offsets,
                                                                 int32_t count) {
    const int32_t t = (int32_t)(blockIdx.x * kVoxBlock + threadIdx.x);
    if (t >= count) return;
    VoxRecord r;
    offsets[t] = vox_setup(tris + (size_t)t * 9, level, margin, r);
    rec[t] = r;
}

// offsets[0 .. count) hold the counts: replaced by their exclusive prefix sums, offsets[count] = the total. One workgroup;
// thread i owns the kVoxScanPerThread counts from i * kVoxScanPerThread on
__global__ void __launch_bounds__(kVoxScanBlock) vox_scan_kernel(uint64_t *__restrict__ offsets, int32_t count) {
    __shared__ uint64_t part[kVoxScanBlock];
    const int32_t first = (int32_t)threadIdx.x * kVoxScanPerThread;
    uint64_t sum = 0;
    for (int32_t j = 0; j < kVoxScanPerThread; ++j)
        if (first + j < count) sum += offsets[first + j];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int32_t d = 1; d < kVoxScanBlock; d <<= 1) {
        const uint64_t add = (int32_t)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - sum;
    for (int32_t j = 0; j < kVoxScanPerThread; ++j)
        if (first + j < count) {
            const uint64_t c = offsets[first + j];
            offsets[first + j] = run;
            run += c;
        }
    if (threadIdx.x == kVoxScanBlock - 1) offsets[count] = part[kVoxScanBlock - 1];
}

// edge function i of projection K at the cell centre (cu, cv): (mu * (cu - pu) + mv * (cv - pv)) + r, closed: >= 0 passes
#define VOX_EDGE(K, I, U, W, cu, cv) \
    ((r.m[K][I][0] * ((cu) - r.v[I][U]) + r.m[K][I][1] * ((cv) - r.v[I][W])) + r.m[K][I][2])

// units [unit_base, unit_base + gridDim.x * kVoxBlock) of the pass, clipped to its total offsets[count]
__global__ void __launch_bounds__(kVoxBlock) vox_pair_kernel(const VoxRecord *__restrict__ rec,
                                                             const uint64_t *__restrict__ offsets, int32_t count,
                                                             uint64_t unit_base, int level, uint32_t *__restrict__ words) {
    const uint64_t unit = unit_base + (uint64_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (unit >= offsets[count]) return;
    // the triangle of the unit: the last t with offsets[t] <= unit (triangles without units share their successor's offset)
    int32_t a = 0, b = count;     // offsets[a] <= unit < offsets[b]
    while (b - a > 1) {
        const int32_t mid = (a + b) >> 1;
        if (offsets[mid] <= unit) a = mid;
        else b = mid;
    }
    const VoxRecord &r = rec[a];
    const uint32_t local = (uint32_t)(unit - offsets[a]);       // < G^2 * ceil(G / 32) <= 2^25
    const int32_t w0 = r.lo[2] >> 5;
    const uint32_t nw = (uint32_t)((r.hi[2] >> 5) - w0 + 1);
    const uint32_t ny = (uint32_t)(r.hi[1] - r.lo[1] + 1);
    const uint32_t column = local / nw;
    const int32_t w = w0 + (int32_t)(local - column * nw);
    const int32_t x = r.lo[0] + (int32_t)(column / ny);
    const int32_t y = r.lo[1] + (int32_t)(column % ny);
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    // projection 2, (u, v) = (x, y), does not depend on z
    if (!(VOX_EDGE(2, 0, 0, 1, cx, cy) >= 0.f) || !(VOX_EDGE(2, 1, 0, 1, cx, cy) >= 0.f) ||
        !(VOX_EDGE(2, 2, 0, 1, cx, cy) >= 0.f))
        return;
    const int32_t z0 = max(r.lo[2], w << 5), z1 = min(r.hi[2], (w << 5) + 31);
    const float dx = cx - r.v[0][0], dy = cy - r.v[0][1];
    const uint32_t key0 = (((uint32_t)x << level) + (uint32_t)y) << level;     // G^3 <= 2^30
    uint32_t mask = 0;
    for (int32_t z = z0; z <= z1; ++z) {
        const float cz = (float)z + 0.5f;
        const float s = (r.n[0] * dx + r.n[1] * dy) + r.n[2] * (cz - r.v[0][2]);
        bool in = s >= -r.rn && s <= r.rn;
        // projection 0: (u, v) = (y, z); projection 1: (u, v) = (z, x)
        in = in && VOX_EDGE(0, 0, 1, 2, cy, cz) >= 0.f && VOX_EDGE(0, 1, 1, 2, cy, cz) >= 0.f &&
             VOX_EDGE(0, 2, 1, 2, cy, cz) >= 0.f;
        in = in && VOX_EDGE(1, 0, 2, 0, cz, cx) >= 0.f && VOX_EDGE(1, 1, 2, 0, cz, cx) >= 0.f &&
             VOX_EDGE(1, 2, 2, 0, cz, cx) >= 0.f;
        mask |= in ? 1u << ((key0 + (uint32_t)z) & 31u) : 0u;
    }
    if (mask) atomicOr(words + ((key0 + (uint32_t)z0) >> 5), mask);
}
#undef VOX_EDGE

// cells >= 32: thread i expands the 16 bits of half (i & 1) of word i >> 1 into 16 bytes; below: one byte per thread
__global__ void __launch_bounds__(kVoxBlock) vox_finish_kernel(const uint32_t *__restrict__ words, uint8_t *__restrict__ grid,
                                                               int64_t cells) {
    const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (cells < 32) {
        if (i < cells) grid[i] = (uint8_t)((words[0] >> i) & 1u);
        return;
    }
    if (i * 16 >= cells) return;
    const uint32_t bits = (words[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t b = bits >> (4 * q);
        o[q] = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
    }
    reinterpret_cast<uint4 *>(grid)[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

size_t vox_record_bytes(int64_t t) { return (size_t)(t < kVoxPass ? t : kVoxPass) * sizeof(VoxRecord); }

}  // namespace

// the records of one pass, then its offsets (one more than records)
size_t mesh_voxelize_workspace(int64_t t) {
    return t <= 0 ? 0 : vox_record_bytes(t) + (size_t)((t < kVoxPass ? t : kVoxPass) + 1) * sizeof(uint64_t);
}

hipError_t mesh_voxelize_dispatch(int64_t t, const float *tris, int level, float margin, uint32_t *words, uint8_t *grid,
                                  void *workspace, hipStream_t s) {
    const int64_t cells = (int64_t)1 << (3 * level);
    if (hipError_t e = hipMemsetAsync(words, 0, (size_t)((cells + 31) / 32) * sizeof(uint32_t), s)) return e;
    VoxRecord *rec = static_cast<VoxRecord *>(workspace);
    uint64_t *offsets = reinterpret_cast<uint64_t *>(static_cast<char *>(workspace) + vox_record_bytes(t));
    for (int64_t first = 0; first < t; first += kVoxPass) {
        const int32_t count = (int32_t)(t - first < kVoxPass ? t - first : kVoxPass);
        hipLaunchKernelGGL(vox_prologue_kernel, dim3((uint32_t)((count + kVoxBlock - 1) / kVoxBlock)), dim3(kVoxBlock), 0, s,
                           tris + (size_t)first * 9, level, margin, rec, offsets, count);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(vox_scan_kernel, dim3(1), dim3(kVoxScanBlock), 0, s, offsets, count);
        if (hipError_t e = hipGetLastError()) return e;
        uint64_t total = 0;
        if (hipError_t e = hipMemcpyAsync(&total, offsets + count, sizeof(total), hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipStreamSynchronize(s)) return e;
        for (uint64_t base = 0; base < total; base += kVoxLaunchUnits) {
            const uint64_t units = total - base < kVoxLaunchUnits ? total - base : kVoxLaunchUnits;
            hipLaunchKernelGGL(vox_pair_kernel, dim3((uint32_t)((units + kVoxBlock - 1) / kVoxBlock)), dim3(kVoxBlock), 0, s,
                               rec, offsets, count, base, level, words);
            if (hipError_t e = hipGetLastError()) return e;
        }
    }
    if (grid) {
        const int64_t threads = cells < 32 ? cells : cells / 16;
        hipLaunchKernelGGL(vox_finish_kernel, dim3((uint32_t)((threads + kVoxBlock - 1) / kVoxBlock)), dim3(kVoxBlock), 0, s,
                           words, grid, cells);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace shacira
