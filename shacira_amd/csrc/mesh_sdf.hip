// mesh_sdf.hip -- signed distance of N points to a triangle soup (shacira_mesh_sdf, contract in include/shacira_hip.h):
// brute force over the N x T pairs, unsigned distance to the nearest non-degenerate triangle and a 13-direction ray-stabbing
// sign. The minimum and the 26 stab flags are order-free and every other value is a function of one triangle or of one
// (point, triangle) pair, so the partition below -- triangle passes, chunks per pass, lanes per point -- cannot change a bit.
//
//   prologue   one thread per triangle writes its TriRecord (edges, normal, edge planes, reciprocals, and per direction the
//              Moeller-Trumbore w = cross(dir, g), 1 / det and the parallel-ray skip bit) once per call; the pair kernel's
//              inner loop then holds only what depends on the point. Triangles are processed in passes of kMeshPass records
//              so that the record array is bounded (kMeshPass * sizeof(TriRecord) = 5.5 MiB).
//   pair       lanes hold points (kMeshPPL per lane, independent instruction streams), blockIdx.y walks triangle chunks.
//              The triangle index is wave-uniform: the record arrives through scalar loads and costs no vector memory
//              traffic or VGPRs; the skip bits are a scalar branch around a whole direction. 13 directions fully unrolled,
//              pos / neg are 26 bits of one register, nothing is indexed dynamically.
//   combine    per (point, chunk) one atomicMin on the bit pattern of the non-negative d^2 minimum (non-negative floats order
//              like their bits) and one atomicOr of the flags into 8 bytes per point, initialised by the call; a last kernel
//              takes the square root and applies the sign. A call with a single chunk finishes inside the pair kernel.
//
// shacira_mesh_closest (further down) is the same pair loop keeping the winning triangle as well: one compare and two selects
// more per pair, a 64-bit atomicMin on (bits(d2), index) to combine, and a finish kernel that derives the closest point from
// the winner. Templated on SIGNED: the unsigned instantiation carries no stab code.
//
// -DMESH_SDF_PLAIN=1 (make variant) builds the comparison kernel instead: one lane per point, no prologue, every
// per-triangle quantity recomputed per pair from the vertices in global memory -- the shape of the reference's kernel. Same
// bits; tools/mesh_sdf_ab.py times one against the other.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "internal.h"

#ifndef MESH_SDF_PLAIN
#define MESH_SDF_PLAIN 0
#endif
#ifndef MESH_SDF_PPL
#define MESH_SDF_PPL 2
#endif

namespace shacira {

namespace {

constexpr int kMeshPPL = MESH_SDF_PPL;               // points per lane
constexpr int kMeshBlock = 256;
constexpr int kMeshPointsPerBlock = kMeshBlock * kMeshPPL;
constexpr int kMeshPass = SHACIRA_MESH_SDF_PASS_TRIANGLES;
constexpr int kMeshGranule = SHACIRA_MESH_SDF_CHUNK_GRANULE;
constexpr int kMeshTargetBlocks = 2048;              // 256 CUs x 8 blocks: what the chunk count fills for small N
constexpr uint32_t kAllFlags = (1u << 26) - 1u;
constexpr uint32_t kInfBits = 0x7f800000u;

constexpr float kH = 0.707106781f, kK = 0.577350269f;
constexpr float kDirX[13] = {1.f, 0.f, 0.f, 0.f, kH, kH, 0.f, kH, kH, kK, -kK, kK, kK};
constexpr float kDirY[13] = {0.f, 1.f, 0.f, kH, 0.f, kH, kH, 0.f, -kH, kK, kK, -kK, kK};
constexpr float kDirZ[13] = {0.f, 0.f, 1.f, kH, kH, 0.f, -kH, -kH, 0.f, kK, kK, kK, -kK};

struct TriRecord {                // 88 dwords, 16-byte aligned
    float a[3], b[3], c[3];
    float e0[3], e1[3], e2[3];
    float n[3];
    float m0[3], m1[3], m2[3];
    float r0, r1, r2, rn;
    uint32_t valid;               // n has a non-zero component
    uint32_t skip;                // bit i: direction i is parallel to the triangle (|det| < 1e-8)
    float w[13][4];               // cross(dir, g) and 1 / det
};
static_assert(sizeof(TriRecord) == 352, "record layout");

// the contract's fixed shapes; the library is built with -ffp-contract=off, so each operator rounds once
__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) {
    return (x0 * y0 + x1 * y1) + x2 * y2;
}
__device__ __forceinline__ float clamp01(float x) { return fmaxf(0.f, fminf(x, 1.f)); }
__device__ __forceinline__ float sgn(float x) { return copysignf(1.f, x); }
// |e * x - p|^2
__device__ __forceinline__ float edge_d2(const float *e, float x, float p0, float p1, float p2) {
    const float t0 = e[0] * x - p0, t1 = e[1] * x - p1, t2 = e[2] * x - p2;
    return (t0 * t0 + t1 * t1) + t2 * t2;
}

// dot(dir_I, q) without the terms whose direction component is a literal 0 (and without the multiply by a literal 1): for
// finite q the dropped terms are +-0, which changes at most the sign of a zero result, and no comparison below sees that
template <int I> __device__ __forceinline__ float dir_dot(float q0, float q1, float q2) {
    constexpr float dx = kDirX[I], dy = kDirY[I], dz = kDirZ[I];
    if constexpr (dy == 0.f && dz == 0.f) return q0;
    else if constexpr (dx == 0.f && dz == 0.f) return q1;
    else if constexpr (dx == 0.f && dy == 0.f) return q2;
    else if constexpr (dx == 0.f) return dy * q1 + dz * q2;
    else if constexpr (dy == 0.f) return dx * q0 + dz * q2;
    else if constexpr (dz == 0.f) return dx * q0 + dy * q1;
    else return (dx * q0 + dy * q1) + dz * q2;
}

// everything of the contract that depends on the triangle alone
__device__ __forceinline__ void tri_setup(const float *__restrict__ v, TriRecord &r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.a[k] = v[k];
        r.b[k] = v[3 + k];
        r.c[k] = v[6 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.e0[k] = r.b[k] - r.a[k];
        r.e1[k] = r.c[k] - r.b[k];
        r.e2[k] = r.a[k] - r.c[k];
    }
#define MESH_CROSS(dst, x, y)                    \
    dst[0] = x[1] * y[2] - x[2] * y[1];          \
    dst[1] = x[2] * y[0] - x[0] * y[2];          \
    dst[2] = x[0] * y[1] - x[1] * y[0];
    MESH_CROSS(r.n, r.e0, r.e2)
    MESH_CROSS(r.m0, r.e0, r.n)
    MESH_CROSS(r.m1, r.e1, r.n)
    MESH_CROSS(r.m2, r.e2, r.n)
    r.r0 = 1.0f / dot3(r.e0[0], r.e0[1], r.e0[2], r.e0[0], r.e0[1], r.e0[2]);
    r.r1 = 1.0f / dot3(r.e1[0], r.e1[1], r.e1[2], r.e1[0], r.e1[1], r.e1[2]);
    r.r2 = 1.0f / dot3(r.e2[0], r.e2[1], r.e2[2], r.e2[0], r.e2[1], r.e2[2]);
    r.rn = 1.0f / dot3(r.n[0], r.n[1], r.n[2], r.n[0], r.n[1], r.n[2]);
    r.valid = (r.n[0] != 0.f || r.n[1] != 0.f || r.n[2] != 0.f) ? 1u : 0u;
    const float g[3] = {-r.e2[0], -r.e2[1], -r.e2[2]};
    uint32_t skip = 0;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const float d[3] = {kDirX[i], kDirY[i], kDirZ[i]};
        float w[3];
        MESH_CROSS(w, d, g)
        const float det = dot3(r.e0[0], r.e0[1], r.e0[2], w[0], w[1], w[2]);
        const double dd = (double)det;
        if (dd > -1e-8 && dd < 1e-8) skip |= 1u << i;
        r.w[i][0] = w[0];
        r.w[i][1] = w[1];
        r.w[i][2] = w[2];
        r.w[i][3] = 1.0f / det;
    }
#undef MESH_CROSS
    r.skip = skip;
}

struct PointState {
    float p[3];
    float m;          // running fminf of d^2
    uint32_t flags;   // bit i: pos[i], bit 13 + i: neg[i]
};

// what the 13 directions share for one (point, triangle) pair
struct StabInput {
    float p0[3], q[3], tau;
};

// d2 of one (point, triangle) pair for a triangle with a non-zero n; p0 = p - a
__device__ __forceinline__ float pair_d2(const TriRecord &r, const float (&p)[3], float p00, float p01, float p02) {
    const float p10 = p[0] - r.b[0], p11 = p[1] - r.b[1], p12 = p[2] - r.b[2];
    const float p20 = p[0] - r.c[0], p21 = p[1] - r.c[1], p22 = p[2] - r.c[2];
    const float sum = (sgn(dot3(r.m0[0], r.m0[1], r.m0[2], p00, p01, p02)) +
                       sgn(dot3(r.m1[0], r.m1[1], r.m1[2], p10, p11, p12))) +
                      sgn(dot3(r.m2[0], r.m2[1], r.m2[2], p20, p21, p22));
    float d2;
    if (sum < 2.f) {
        const float x0 = clamp01(dot3(r.e0[0], r.e0[1], r.e0[2], p00, p01, p02) * r.r0);
        const float x1 = clamp01(dot3(r.e1[0], r.e1[1], r.e1[2], p10, p11, p12) * r.r1);
        const float x2 = clamp01(dot3(r.e2[0], r.e2[1], r.e2[2], p20, p21, p22) * r.r2);
        d2 = fminf(edge_d2(r.e0, x0, p00, p01, p02),
                   fminf(edge_d2(r.e1, x1, p10, p11, p12), edge_d2(r.e2, x2, p20, p21, p22)));
    } else {
        const float h = dot3(r.n[0], r.n[1], r.n[2], p00, p01, p02);
        d2 = (h * h) * r.rn;
    }
    if (d2 < 0.f) d2 = 0.f;
    return d2;
}

// the pair's q = cross(p0, e0), tau = dot(g, q) with g = -e2
__device__ __forceinline__ void stab_input(const TriRecord &r, float p00, float p01, float p02, StabInput &in) {
    in.p0[0] = p00;
    in.p0[1] = p01;
    in.p0[2] = p02;
    in.q[0] = p01 * r.e0[2] - p02 * r.e0[1];
    in.q[1] = p02 * r.e0[0] - p00 * r.e0[2];
    in.q[2] = p00 * r.e0[1] - p01 * r.e0[0];
    in.tau = dot3(-r.e2[0], -r.e2[1], -r.e2[2], in.q[0], in.q[1], in.q[2]);
}

// the distance part of one (point, triangle) pair, and what its 13 directions share
__device__ __forceinline__ void pair_distance(const TriRecord &r, PointState &s, StabInput &in) {
    const float p00 = s.p[0] - r.a[0], p01 = s.p[1] - r.a[1], p02 = s.p[2] - r.a[2];
    if (r.valid) s.m = fminf(s.m, pair_d2(r, s.p, p00, p01, p02));
    stab_input(r, p00, p01, p02, in);
}

template <int I> __device__ __forceinline__ void stab(const TriRecord &r, const StabInput &in, uint32_t &flags) {
    const float inv = r.w[I][3];
    const float u = dot3(in.p0[0], in.p0[1], in.p0[2], r.w[I][0], r.w[I][1], r.w[I][2]) * inv;
    const float v = dir_dot<I>(in.q[0], in.q[1], in.q[2]) * inv;
    const float t = in.tau * inv;
    const bool hit = !(u < 0.f || u > 1.f) && !(v < 0.f || u + v > 1.f);
    const uint32_t bit = (t >= 0.f) ? (1u << I) : (1u << (13 + I));
    flags |= hit ? bit : 0u;
}

// direction I for the P points of a lane: the skip bit is wave-uniform, one scalar branch around the whole direction
template <int I, int P, class S> __device__ __forceinline__ void stab_all(const TriRecord &r, const StabInput (&in)[P],
                                                                          S (&s)[P]) {
    if (!((r.skip >> I) & 1u)) {
#pragma unroll
        for (int j = 0; j < P; ++j) stab<I>(r, in[j], s[j].flags);
    }
    if constexpr (I + 1 < 13) stab_all<I + 1, P, S>(r, in, s);
}

// triangle r against the P points of a lane
template <int P> __device__ __forceinline__ void pair_update(const TriRecord &r, PointState (&s)[P]) {
    StabInput in[P];
#pragma unroll
    for (int j = 0; j < P; ++j) pair_distance(r, s[j], in[j]);
    stab_all<0, P, PointState>(r, in, s);
}

__device__ __forceinline__ float finish(float m, uint32_t flags) {
    const float dist = sqrtf(m);
    return (flags & kAllFlags) == kAllFlags ? -dist : dist;
}

__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_fill_kernel(float *__restrict__ sdf, uint2 *__restrict__ acc,
                                                                   int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    if (acc) acc[i] = make_uint2(kInfBits, 0u);
    else sdf[i] = INFINITY;
}

__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_prologue_kernel(const float *__restrict__ tris,
                                                                       TriRecord *__restrict__ rec, int32_t count) {
    const int32_t t = (int32_t)(blockIdx.x * kMeshBlock + threadIdx.x);
    if (t >= count) return;
    TriRecord r;
    tri_setup(tris + (size_t)t * 9, r);
    rec[t] = r;
}

#if !MESH_SDF_PLAIN

__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_finish_kernel(const uint2 *__restrict__ acc, float *__restrict__ sdf,
                                                                     int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 a = acc[i];
    sdf[i] = finish(__uint_as_float(a.x), a.y);
}

// rec: the records of this pass (count of them); blockIdx.y = chunk, triangles [chunk * chunk_len, +chunk_len) of the pass.
// FINAL: the call has one pass of one chunk, the result is written here; else the chunk's minimum and flags are merged into acc
template <bool FINAL>
__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_pair_kernel(const float *__restrict__ points,
                                                                   const TriRecord *__restrict__ rec, int32_t count,
                                                                   int32_t chunk_len, uint2 *__restrict__ acc,
                                                                   float *__restrict__ sdf, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * kMeshPointsPerBlock + threadIdx.x;
    PointState s[kMeshPPL];
#pragma unroll
    for (int j = 0; j < kMeshPPL; ++j) {
        const int64_t i = base + (int64_t)j * kMeshBlock;
        const int64_t ld = i < n ? i : n - 1;        // idle lanes repeat the last point and store nothing
        s[j].p[0] = points[ld * 3 + 0];
        s[j].p[1] = points[ld * 3 + 1];
        s[j].p[2] = points[ld * 3 + 2];
        s[j].m = INFINITY;
        s[j].flags = 0u;
    }
    const int32_t t0 = (int32_t)blockIdx.y * chunk_len;
    const int32_t t1 = min(t0 + chunk_len, count);
    for (int32_t t = t0; t < t1; ++t) {
        const TriRecord &r = rec[t];
        pair_update<kMeshPPL>(r, s);
    }
#pragma unroll
    for (int j = 0; j < kMeshPPL; ++j) {
        const int64_t i = base + (int64_t)j * kMeshBlock;
        if (i >= n) continue;
        if (FINAL) {
            sdf[i] = finish(s[j].m, s[j].flags);
        } else {
            uint32_t *a = reinterpret_cast<uint32_t *>(acc + i);
            atomicMin(a, __float_as_uint(s[j].m));   // m >= +0 or +inf: ordered like its bits
            if (s[j].flags) atomicOr(a + 1, s[j].flags);
        }
    }
}

#else  // MESH_SDF_PLAIN

__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_plain_kernel(const float *__restrict__ points,
                                                                    const float *__restrict__ tris, int32_t count,
                                                                    float *__restrict__ sdf, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    PointState s[1];
    s[0].p[0] = points[i * 3 + 0];
    s[0].p[1] = points[i * 3 + 1];
    s[0].p[2] = points[i * 3 + 2];
    s[0].m = INFINITY;
    s[0].flags = 0u;
    for (int32_t t = 0; t < count; ++t) {
        TriRecord r;
        tri_setup(tris + (size_t)t * 9, r);
        pair_update<1>(r, s);
    }
    sdf[i] = finish(s[0].m, s[0].flags);
}

#endif

// ---- closest point (shacira_mesh_closest): the same pair loop keeping the winner ----------------------------------------------
// Per point 16 bytes of workspace: the key (bits(d2) << 32) | triangle index, merged with ONE 64-bit atomicMin per (point,
// chunk) -- non-negative floats order like their bits and the low word breaks ties towards the lowest mesh-wide index -- and
// the 26 stab flags (SIGNED only). The finish kernel reads the one winning triangle back and derives dist, hit, tidx from it.
struct ClosestState {
    float p[3];
    float m;          // least d^2 so far: replaced iff d2 < m, so a NaN never wins and the first of equals stays
    int32_t idx;      // its index within the pass, -1: none
    uint32_t flags;
};

constexpr uint32_t kNoTriangle = 0xffffffffu;

__global__ void __launch_bounds__(kMeshBlock) mesh_closest_fill_kernel(uint4 *__restrict__ acc, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i < n) acc[i] = make_uint4(kNoTriangle, kInfBits, 0u, 0u);   // key = (+inf, -1), flags = 0
}

template <bool SIGNED, int P>
__device__ __forceinline__ void closest_update(const TriRecord &r, int32_t t, ClosestState (&s)[P]) {
    [[maybe_unused]] StabInput in[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const float p00 = s[j].p[0] - r.a[0], p01 = s[j].p[1] - r.a[1], p02 = s[j].p[2] - r.a[2];
        if (r.valid) {
            const float d2 = pair_d2(r, s[j].p, p00, p01, p02);
            const bool better = d2 < s[j].m;
            s[j].m = better ? d2 : s[j].m;
            s[j].idx = better ? t : s[j].idx;
        }
        if constexpr (SIGNED) stab_input(r, p00, p01, p02, in[j]);
    }
    if constexpr (SIGNED) stab_all<0, P, ClosestState>(r, in, s);
}

// as mesh_sdf_pair_kernel; `first` is the mesh-wide index of the pass's first triangle
template <bool SIGNED>
__global__ void __launch_bounds__(kMeshBlock) mesh_closest_pair_kernel(const float *__restrict__ points,
                                                                       const TriRecord *__restrict__ rec, int32_t count,
                                                                       int32_t chunk_len, int32_t first,
                                                                       uint4 *__restrict__ acc, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * kMeshPointsPerBlock + threadIdx.x;
    ClosestState s[kMeshPPL];
#pragma unroll
    for (int j = 0; j < kMeshPPL; ++j) {
        const int64_t i = base + (int64_t)j * kMeshBlock;
        const int64_t ld = i < n ? i : n - 1;        // idle lanes repeat the last point and store nothing
        s[j].p[0] = points[ld * 3 + 0];
        s[j].p[1] = points[ld * 3 + 1];
        s[j].p[2] = points[ld * 3 + 2];
        s[j].m = INFINITY;
        s[j].idx = -1;
        s[j].flags = 0u;
    }
    const int32_t t0 = (int32_t)blockIdx.y * chunk_len;
    const int32_t t1 = min(t0 + chunk_len, count);
    for (int32_t t = t0; t < t1; ++t) {
        const TriRecord &r = rec[t];
        closest_update<SIGNED, kMeshPPL>(r, t, s);
    }
#pragma unroll
    for (int j = 0; j < kMeshPPL; ++j) {
        const int64_t i = base + (int64_t)j * kMeshBlock;
        if (i >= n) continue;
        if (s[j].idx >= 0) {
            const unsigned long long key =
                ((unsigned long long)__float_as_uint(s[j].m) << 32) | (uint32_t)(first + s[j].idx);
            atomicMin(reinterpret_cast<unsigned long long *>(acc + i), key);
        }
        if (SIGNED && s[j].flags) atomicOr(reinterpret_cast<uint32_t *>(acc + i) + 2, s[j].flags);
    }
}

template <bool SIGNED>
__global__ void __launch_bounds__(kMeshBlock) mesh_closest_finish_kernel(const float *__restrict__ points,
                                                                         const float *__restrict__ tris,
                                                                         const uint4 *__restrict__ acc,
                                                                         float *__restrict__ dist, float *__restrict__ hit,
                                                                         int32_t *__restrict__ tidx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    const uint4 a = acc[i];
    const float p[3] = {points[i * 3 + 0], points[i * 3 + 1], points[i * 3 + 2]};
    float h[3] = {p[0], p[1], p[2]};
    if (a.x != kNoTriangle) {
        TriRecord r;
        tri_setup(tris + (size_t)a.x * 9, r);
        const float p0[3] = {p[0] - r.a[0], p[1] - r.a[1], p[2] - r.a[2]};
        const float p1[3] = {p[0] - r.b[0], p[1] - r.b[1], p[2] - r.b[2]};
        const float p2[3] = {p[0] - r.c[0], p[1] - r.c[1], p[2] - r.c[2]};
        const float sum = (sgn(dot3(r.m0[0], r.m0[1], r.m0[2], p0[0], p0[1], p0[2])) +
                           sgn(dot3(r.m1[0], r.m1[1], r.m1[2], p1[0], p1[1], p1[2]))) +
                          sgn(dot3(r.m2[0], r.m2[1], r.m2[2], p2[0], p2[1], p2[2]));
        if (sum >= 2.f) {
            const float k = dot3(r.n[0], r.n[1], r.n[2], p0[0], p0[1], p0[2]) * r.rn;
#pragma unroll
            for (int j = 0; j < 3; ++j) h[j] = p[j] - r.n[j] * k;
        } else {
            const float x0 = clamp01(dot3(r.e0[0], r.e0[1], r.e0[2], p0[0], p0[1], p0[2]) * r.r0);
            const float x1 = clamp01(dot3(r.e1[0], r.e1[1], r.e1[2], p1[0], p1[1], p1[2]) * r.r1);
            const float x2 = clamp01(dot3(r.e2[0], r.e2[1], r.e2[2], p2[0], p2[1], p2[2]) * r.r2);
            const float E0 = edge_d2(r.e0, x0, p0[0], p0[1], p0[2]);
            const float E1 = edge_d2(r.e1, x1, p1[0], p1[1], p1[2]);
            const float E2 = edge_d2(r.e2, x2, p2[0], p2[1], p2[2]);
            const bool first = E0 <= E1 && E0 <= E2, second = E1 <= E2;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float v = first ? r.a[j] : second ? r.b[j] : r.c[j];
                const float e = first ? r.e0[j] : second ? r.e1[j] : r.e2[j];
                const float x = first ? x0 : second ? x1 : x2;
                h[j] = v + e * x;
            }
        }
    }
    dist[i] = finish(__uint_as_float(a.y), SIGNED ? a.z : 0u);
    hit[i * 3 + 0] = h[0];
    hit[i * 3 + 1] = h[1];
    hit[i * 3 + 2] = h[2];
    tidx[i] = (int32_t)a.x;
}

// chunks of one pass of `count` triangles for n points: as many as bring the grid to kMeshTargetBlocks workgroups when n is
// small, one (no atomics beyond a pair per point and pass) once the point blocks alone reach that
void mesh_chunks(int64_t n, int32_t count, int32_t &chunk_len, int32_t &chunks) {
    const int64_t bx = (n + kMeshPointsPerBlock - 1) / kMeshPointsPerBlock;
    int64_t want = (kMeshTargetBlocks + bx - 1) / bx;
    const int64_t most = (count + kMeshGranule - 1) / kMeshGranule;
    if (want > most) want = most;
    if (want < 1) want = 1;
    int64_t len = (count + want - 1) / want;
    len = (len + kMeshGranule - 1) / kMeshGranule * kMeshGranule;
    chunk_len = (int32_t)len;
    chunks = (int32_t)((count + len - 1) / len);
}

}  // namespace

size_t mesh_sdf_workspace(int64_t n, int64_t t) {
    if (n <= 0 || t <= 0) return 0;
    const int64_t recs = t < kMeshPass ? t : kMeshPass;
    return (size_t)recs * sizeof(TriRecord) + (size_t)n * sizeof(uint2);
}

hipError_t mesh_sdf_dispatch(int64_t n, int64_t t, const float *points, const float *tris, float *sdf, void *workspace,
                             hipStream_t s) {
    const dim3 block(kMeshBlock);
    const dim3 per_point((uint32_t)((n + kMeshBlock - 1) / kMeshBlock));
    if (t == 0) {
        hipLaunchKernelGGL(mesh_sdf_fill_kernel, per_point, block, 0, s, sdf, (uint2 *)nullptr, n);
        return hipGetLastError();
    }
#if MESH_SDF_PLAIN
    hipLaunchKernelGGL(mesh_sdf_plain_kernel, per_point, block, 0, s, points, tris, (int32_t)t, sdf, n);
    return hipGetLastError();
#else
    const int64_t recs = t < kMeshPass ? t : kMeshPass;
    TriRecord *rec = static_cast<TriRecord *>(workspace);
    uint2 *acc = reinterpret_cast<uint2 *>(static_cast<char *>(workspace) + (size_t)recs * sizeof(TriRecord));
    const uint32_t bx = (uint32_t)((n + kMeshPointsPerBlock - 1) / kMeshPointsPerBlock);
    int32_t chunk_len = 0, chunks = 0;
    mesh_chunks(n, (int32_t)recs, chunk_len, chunks);
    const bool final_in_pair = t <= kMeshPass && chunks == 1;
    if (!final_in_pair) {
        hipLaunchKernelGGL(mesh_sdf_fill_kernel, per_point, block, 0, s, sdf, acc, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    for (int64_t first = 0; first < t; first += kMeshPass) {
        const int32_t count = (int32_t)(t - first < kMeshPass ? t - first : kMeshPass);
        hipLaunchKernelGGL(mesh_sdf_prologue_kernel, dim3((uint32_t)((count + kMeshBlock - 1) / kMeshBlock)), block, 0, s,
                           tris + (size_t)first * 9, rec, count);
        if (hipError_t e = hipGetLastError()) return e;
        mesh_chunks(n, count, chunk_len, chunks);
        const dim3 grid(bx, (uint32_t)chunks);
        if (final_in_pair)
            hipLaunchKernelGGL(mesh_sdf_pair_kernel<true>, grid, block, 0, s, points, rec, count, chunk_len, acc, sdf, n);
        else
            hipLaunchKernelGGL(mesh_sdf_pair_kernel<false>, grid, block, 0, s, points, rec, count, chunk_len, acc, sdf, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (!final_in_pair) {
        hipLaunchKernelGGL(mesh_sdf_finish_kernel, per_point, block, 0, s, acc, sdf, n);
        return hipGetLastError();
    }
    return hipSuccess;
#endif
}

size_t mesh_closest_workspace(int64_t n, int64_t t) {
    if (n <= 0) return 0;
    const int64_t recs = t < kMeshPass ? t : kMeshPass;
    return (size_t)recs * sizeof(TriRecord) + (size_t)n * sizeof(uint4);
}

hipError_t mesh_closest_dispatch(int64_t n, int64_t t, const float *points, const float *tris, bool is_signed, float *dist,
                                 float *hit, int32_t *tidx, void *workspace, hipStream_t s) {
    const dim3 block(kMeshBlock);
    const dim3 per_point((uint32_t)((n + kMeshBlock - 1) / kMeshBlock));
    const int64_t recs = t < kMeshPass ? t : kMeshPass;
    TriRecord *rec = static_cast<TriRecord *>(workspace);
    uint4 *acc = reinterpret_cast<uint4 *>(static_cast<char *>(workspace) + (size_t)recs * sizeof(TriRecord));
    const uint32_t bx = (uint32_t)((n + kMeshPointsPerBlock - 1) / kMeshPointsPerBlock);
    hipLaunchKernelGGL(mesh_closest_fill_kernel, per_point, block, 0, s, acc, n);
    if (hipError_t e = hipGetLastError()) return e;
    for (int64_t first = 0; first < t; first += kMeshPass) {
        const int32_t count = (int32_t)(t - first < kMeshPass ? t - first : kMeshPass);
        hipLaunchKernelGGL(mesh_sdf_prologue_kernel, dim3((uint32_t)((count + kMeshBlock - 1) / kMeshBlock)), block, 0, s,
                           tris + (size_t)first * 9, rec, count);
        if (hipError_t e = hipGetLastError()) return e;
        int32_t chunk_len = 0, chunks = 0;
        mesh_chunks(n, count, chunk_len, chunks);
        const dim3 grid(bx, (uint32_t)chunks);
        if (is_signed)
            hipLaunchKernelGGL(mesh_closest_pair_kernel<true>, grid, block, 0, s, points, rec, count, chunk_len,
                               (int32_t)first, acc, n);
        else
            hipLaunchKernelGGL(mesh_closest_pair_kernel<false>, grid, block, 0, s, points, rec, count, chunk_len,
                               (int32_t)first, acc, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (is_signed)
        hipLaunchKernelGGL(mesh_closest_finish_kernel<true>, per_point, block, 0, s, points, tris, acc, dist, hit, tidx, n);
    else
        hipLaunchKernelGGL(mesh_closest_finish_kernel<false>, per_point, block, 0, s, points, tris, acc, dist, hit, tidx, n);
    return hipGetLastError();
}

}  // namespace shacira
