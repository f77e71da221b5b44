// mesh_sdf.hip -- N points against a triangle soup, brute force over the N x T pairs (contracts in include/shacira_hip.h):
// shacira_mesh_sdf, the unsigned distance to the nearest non-degenerate triangle with a 13-direction ray-stabbing sign, and
// shacira_mesh_closest, the same distance with the winning triangle and the closest point on it, signed or not. The minimum,
// the argmin with its lowest-index tie rule and the 26 stab flags are order-free and every other value is a function of one
// triangle or of one (point, triangle) pair, so the partition below -- triangle passes, chunks per pass, lanes per point --
// cannot change a bit.
//
//   prologue   one thread per triangle writes its TriRecord (edges, normal, edge planes, reciprocals, and per direction the
//              Moeller-Trumbore w = cross(dir, g), 1 / det and the parallel-ray skip bit) once per call; the pair kernel's
//              inner loop then holds only what depends on the point. Triangles are processed in passes of kMeshPass records
//              so that the record array is bounded (kMeshPass * sizeof(TriRecord) = 5.5 MiB).
//   pair       ONE loop, mesh_pair_kernel<WINNER, SIGNED, FINAL>. Lanes hold points (kMeshPPL per lane, independent
//              instruction streams), blockIdx.y walks triangle chunks. The triangle index is wave-uniform: the record arrives
//              through scalar loads and costs no vector memory traffic or VGPRs; the skip bits are a scalar branch around a
//              whole direction. 13 directions fully unrolled, pos / neg are 26 bits of one register, nothing is indexed
//              dynamically. WINNER keeps the index of the least d^2 (one compare and two selects per pair in place of the
//              fminf); without SIGNED there is no stab code at all.
//   combine    per (point, chunk) into an accumulator per point that the call initialises. Distance: 8 bytes, one atomicMin
//              on the bit pattern of the non-negative d^2 minimum (non-negative floats order like their bits) and one atomicOr
//              of the flags. Winner: 16 bytes, ONE 64-bit atomicMin on the key (bits(d2) << 32) | mesh-wide triangle index --
//              the low word breaks ties towards the lowest index -- and the atomicOr. A finish kernel takes the square root
//              and applies the sign; the winner's also reads the one winning triangle back and derives the closest point
//              from it. A distance call with a single chunk finishes inside the pair kernel (FINAL).
//
// Four instantiations: distance FINAL, distance merged, winner signed, winner unsigned.
//
// -DMESH_SDF_PLAIN=1 (make variant) builds the comparison kernel for the distance call instead: one lane per point, no
// prologue, every per-triangle quantity recomputed per pair from the vertices in global memory -- the shape of the
// reference's kernel. Same bits; tools/mesh_sdf_ab.py times one against the other.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

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
constexpr uint32_t kNoTriangle = 0xffffffffu;

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
__device__ __forceinline__ float dot3(const float (&x)[3], const float (&y)[3]) {
    return dot3(x[0], x[1], x[2], y[0], y[1], y[2]);
}
__device__ __forceinline__ float clamp01(float x) { return fmaxf(0.f, fminf(x, 1.f)); }
__device__ __forceinline__ float sgn(float x) { return copysignf(1.f, x); }
// |e * x - p|^2
__device__ __forceinline__ float edge_d2(const float (&e)[3], float x, const float (&p)[3]) {
    const float t0 = e[0] * x - p[0], t1 = e[1] * x - p[1], t2 = e[2] * x - p[2];
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
    r.r0 = 1.0f / dot3(r.e0, r.e0);
    r.r1 = 1.0f / dot3(r.e1, r.e1);
    r.r2 = 1.0f / dot3(r.e2, r.e2);
    r.rn = 1.0f / dot3(r.n, r.n);
    r.valid = (r.n[0] != 0.f || r.n[1] != 0.f || r.n[2] != 0.f) ? 1u : 0u;
    const float g[3] = {-r.e2[0], -r.e2[1], -r.e2[2]};
    uint32_t skip = 0;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        const float d[3] = {kDirX[i], kDirY[i], kDirZ[i]};
        float w[3];
        MESH_CROSS(w, d, g)
        const float det = dot3(r.e0, w);
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
    float m;          // least d^2 so far
    int32_t idx;      // WINNER: its index within the pass, -1: none; otherwise never touched
    uint32_t flags;   // SIGNED: bit i: pos[i], bit 13 + i: neg[i]
};

// what the contract takes from one (point, triangle) pair before it branches on the edge-plane signs
struct PairTerms {
    float p0[3], p1[3], p2[3];   // p - a, p - b, p - c
    float sum;                   // of the three edge-plane signs: >= 2 over the face
};

__device__ __forceinline__ void pair_terms(const TriRecord &r, const float (&p)[3], PairTerms &k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        k.p0[c] = p[c] - r.a[c];
        k.p1[c] = p[c] - r.b[c];
        k.p2[c] = p[c] - r.c[c];
    }
    k.sum = (sgn(dot3(r.m0, k.p0)) + sgn(dot3(r.m1, k.p1))) + sgn(dot3(r.m2, k.p2));
}

// the edge branch: the clamped projections on the three edges and the squared distances to them
__device__ __forceinline__ void edge_terms(const TriRecord &r, const PairTerms &k, float (&x)[3], float (&E)[3]) {
    x[0] = clamp01(dot3(r.e0, k.p0) * r.r0);
    x[1] = clamp01(dot3(r.e1, k.p1) * r.r1);
    x[2] = clamp01(dot3(r.e2, k.p2) * r.r2);
    E[0] = edge_d2(r.e0, x[0], k.p0);
    E[1] = edge_d2(r.e1, x[1], k.p1);
    E[2] = edge_d2(r.e2, x[2], k.p2);
}

// d2 of one (point, triangle) pair for a triangle with a non-zero n
__device__ __forceinline__ float pair_d2(const TriRecord &r, const PairTerms &k) {
    float d2;
    if (k.sum < 2.f) {
        float x[3], E[3];
        edge_terms(r, k, x, E);
        d2 = fminf(E[0], fminf(E[1], E[2]));
    } else {
        const float h = dot3(r.n, k.p0);
        d2 = (h * h) * r.rn;
    }
    if (d2 < 0.f) d2 = 0.f;
    return d2;
}

// what the 13 directions share for one (point, triangle) pair: p0 = p - a, q = cross(p0, e0), tau = dot(g, q) with g = -e2
struct StabInput {
    float p0[3], q[3], tau;
};

__device__ __forceinline__ void stab_input(const TriRecord &r, const float (&p)[3], StabInput &in) {
#pragma unroll
    for (int c = 0; c < 3; ++c) in.p0[c] = p[c] - r.a[c];
    in.q[0] = in.p0[1] * r.e0[2] - in.p0[2] * r.e0[1];
    in.q[1] = in.p0[2] * r.e0[0] - in.p0[0] * r.e0[2];
    in.q[2] = in.p0[0] * r.e0[1] - in.p0[1] * r.e0[0];
    in.tau = dot3(-r.e2[0], -r.e2[1], -r.e2[2], in.q[0], in.q[1], in.q[2]);
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
template <int I, int P> __device__ __forceinline__ void stab_all(const TriRecord &r, const StabInput (&in)[P],
                                                                 PointState (&s)[P]) {
    if (!((r.skip >> I) & 1u)) {
#pragma unroll
        for (int j = 0; j < P; ++j) stab<I>(r, in[j], s[j].flags);
    }
    if constexpr (I + 1 < 13) stab_all<I + 1, P>(r, in, s);
}

// triangle r (index t within its pass) against the P points of a lane. WINNER: m is replaced iff d2 < m, so a NaN never wins
// and the first of equals stays; else the running fminf. The stab's p0 is pair_terms' (one subtraction after inlining); the
// pair terms are taken under r.valid, where alone they are used
template <bool WINNER, bool SIGNED, int P>
__device__ __forceinline__ void pair_update(const TriRecord &r, int32_t t, PointState (&s)[P]) {
    [[maybe_unused]] StabInput in[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if constexpr (SIGNED) stab_input(r, s[j].p, in[j]);
        if (r.valid) {
            PairTerms k;
            pair_terms(r, s[j].p, k);
            const float d2 = pair_d2(r, k);
            if constexpr (WINNER) {
                const bool better = d2 < s[j].m;
                s[j].m = better ? d2 : s[j].m;
                s[j].idx = better ? t : s[j].idx;
            } else {
                s[j].m = fminf(s[j].m, d2);
            }
        }
    }
    if constexpr (SIGNED) stab_all<0, P>(r, in, s);
}

// idx stays out: initialised where nothing reads it, it still cost the distance loop 7 VALU instructions per triangle
__device__ __forceinline__ void point_init(const float *__restrict__ points, int64_t i, PointState &s) {
    s.p[0] = points[i * 3 + 0];
    s.p[1] = points[i * 3 + 1];
    s.p[2] = points[i * 3 + 2];
    s.m = INFINITY;
    s.flags = 0u;
}

__device__ __forceinline__ float finish(float m, uint32_t flags) {
    const float dist = sqrtf(m);
    return (flags & kAllFlags) == kAllFlags ? -dist : dist;
}

// the accumulator of one point. Distance: (bits(min d2), flags). WINNER: the key as (mesh-wide index, bits(d2)) -- one
// little-endian 64-bit word -- then the flags and a pad
template <bool WINNER> using MeshAcc = std::conditional_t<WINNER, uint4, uint2>;

// acc[i] = (+inf, no triangle, no flags); a distance call without triangles has no workspace and gets +inf straight into sdf
template <bool WINNER>
__global__ void __launch_bounds__(kMeshBlock) mesh_fill_kernel(MeshAcc<WINNER> *__restrict__ acc, float *__restrict__ sdf,
                                                               int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    if constexpr (WINNER) acc[i] = make_uint4(kNoTriangle, kInfBits, 0u, 0u);
    else if (acc) acc[i] = make_uint2(kInfBits, 0u);
    else sdf[i] = INFINITY;
}

__global__ void __launch_bounds__(kMeshBlock) mesh_prologue_kernel(const float *__restrict__ tris,
                                                                   TriRecord *__restrict__ rec, int32_t count) {
    const int32_t t = (int32_t)(blockIdx.x * kMeshBlock + threadIdx.x);
    if (t >= count) return;
    TriRecord r;
    tri_setup(tris + (size_t)t * 9, r);
    rec[t] = r;
}

// rec: the records of this pass (count of them, the first is triangle `first` of the mesh); blockIdx.y = chunk, triangles
// [chunk * chunk_len, +chunk_len) of the pass. FINAL: the call has one pass of one chunk and the result is written to sdf;
// else the chunk's minimum (WINNER: with its triangle) and flags are merged into acc
template <bool WINNER, bool SIGNED, bool FINAL>
__global__ void __launch_bounds__(kMeshBlock) mesh_pair_kernel(const float *__restrict__ points,
                                                               const TriRecord *__restrict__ rec, int32_t count,
                                                               int32_t chunk_len, int32_t first,
                                                               MeshAcc<WINNER> *__restrict__ acc, float *__restrict__ sdf,
                                                               int64_t n) {
    static_assert(WINNER || SIGNED, "the distance call is always signed");
    static_assert(!FINAL || !WINNER, "the winner is always finished from its accumulator");
    const int64_t base = (int64_t)blockIdx.x * kMeshPointsPerBlock + threadIdx.x;
    PointState s[kMeshPPL];
#pragma unroll
    for (int j = 0; j < kMeshPPL; ++j) {
        const int64_t i = base + (int64_t)j * kMeshBlock;
        point_init(points, i < n ? i : n - 1, s[j]);     // idle lanes repeat the last point and store nothing
        if constexpr (WINNER) s[j].idx = -1;
    }
    const int32_t t0 = (int32_t)blockIdx.y * chunk_len;
    const int32_t t1 = min(t0 + chunk_len, count);
    for (int32_t t = t0; t < t1; ++t) {
        const TriRecord &r = rec[t];
        pair_update<WINNER, SIGNED, kMeshPPL>(r, t, s);
    }
#pragma unroll
    for (int j = 0; j < kMeshPPL; ++j) {
        const int64_t i = base + (int64_t)j * kMeshBlock;
        if (i >= n) continue;
        uint32_t *a = reinterpret_cast<uint32_t *>(acc + i);
        if constexpr (FINAL) {
            sdf[i] = finish(s[j].m, s[j].flags);
        } else if constexpr (WINNER) {
            if (s[j].idx >= 0) {
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint(s[j].m) << 32) | (uint32_t)(first + s[j].idx);
                atomicMin(reinterpret_cast<unsigned long long *>(a), key);
            }
            if (SIGNED && s[j].flags) atomicOr(a + 2, s[j].flags);
        } else {
            atomicMin(a, __float_as_uint(s[j].m));       // m >= +0 or +inf: ordered like its bits
            if (s[j].flags) atomicOr(a + 1, s[j].flags);
        }
    }
}

#if !MESH_SDF_PLAIN

__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_finish_kernel(const uint2 *__restrict__ acc, float *__restrict__ sdf,
                                                                     int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 a = acc[i];
    sdf[i] = finish(__uint_as_float(a.x), a.y);
}

#else  // MESH_SDF_PLAIN

__global__ void __launch_bounds__(kMeshBlock) mesh_sdf_plain_kernel(const float *__restrict__ points,
                                                                    const float *__restrict__ tris, int32_t count,
                                                                    float *__restrict__ sdf, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i >= n) return;
    PointState s[1];
    point_init(points, i, s[0]);
    for (int32_t t = 0; t < count; ++t) {
        TriRecord r;
        tri_setup(tris + (size_t)t * 9, r);
        pair_update<false, true, 1>(r, t, s);
    }
    sdf[i] = finish(s[0].m, s[0].flags);
}

#endif

// dist, tidx and the closest point on the winning triangle, rebuilt from its vertices: over the face p - n * dot(n, p0) / |n|^2,
// else the clamped projection on the nearest edge (the first of equals). An unsigned call never set a flag: its dist is +
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
        PairTerms k;
        pair_terms(r, p, k);
        if (k.sum >= 2.f) {
            const float c = dot3(r.n, k.p0) * r.rn;
#pragma unroll
            for (int j = 0; j < 3; ++j) h[j] = p[j] - r.n[j] * c;
        } else {
            float x[3], E[3];
            edge_terms(r, k, x, E);
            const bool first = E[0] <= E[1] && E[0] <= E[2], second = E[1] <= E[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float v = first ? r.a[j] : second ? r.b[j] : r.c[j];
                const float e = first ? r.e0[j] : second ? r.e1[j] : r.e2[j];
                h[j] = v + e * (first ? x[0] : second ? x[1] : x[2]);
            }
        }
    }
    dist[i] = finish(__uint_as_float(a.y), a.z);
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

// the workspace of either call: the records of one pass, then one accumulator per point
size_t mesh_record_bytes(int64_t t) { return (size_t)(t < kMeshPass ? t : kMeshPass) * sizeof(TriRecord); }

template <class Acc> size_t mesh_workspace(int64_t n, int64_t t) { return mesh_record_bytes(t) + (size_t)n * sizeof(Acc); }

template <class Acc> Acc *mesh_accumulators(void *workspace, int64_t t) {
    return reinterpret_cast<Acc *>(static_cast<char *>(workspace) + mesh_record_bytes(t));
}

dim3 mesh_per_point(int64_t n) { return dim3((uint32_t)((n + kMeshBlock - 1) / kMeshBlock)); }

template <class Acc>
using MeshPairKernel = void (*)(const float *, const TriRecord *, int32_t, int32_t, int32_t, Acc *, float *, int64_t);

// every pass of kMeshPass triangles: its records, then its pair kernel over the point blocks and the pass's chunks
template <class Acc>
hipError_t mesh_passes(MeshPairKernel<Acc> pair, int64_t n, int64_t t, const float *points, const float *tris, TriRecord *rec,
                       Acc *acc, float *sdf, hipStream_t s) {
    const uint32_t bx = (uint32_t)((n + kMeshPointsPerBlock - 1) / kMeshPointsPerBlock);
    for (int64_t first = 0; first < t; first += kMeshPass) {
        const int32_t count = (int32_t)(t - first < kMeshPass ? t - first : kMeshPass);
        hipLaunchKernelGGL(mesh_prologue_kernel, mesh_per_point(count), dim3(kMeshBlock), 0, s, tris + (size_t)first * 9, rec,
                           count);
        if (hipError_t e = hipGetLastError()) return e;
        int32_t chunk_len = 0, chunks = 0;
        mesh_chunks(n, count, chunk_len, chunks);
        hipLaunchKernelGGL(pair, dim3(bx, (uint32_t)chunks), dim3(kMeshBlock), 0, s, points, rec, count, chunk_len,
                           (int32_t)first, acc, sdf, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace

size_t mesh_sdf_workspace(int64_t n, int64_t t) { return n <= 0 || t <= 0 ? 0 : mesh_workspace<uint2>(n, t); }

hipError_t mesh_sdf_dispatch(int64_t n, int64_t t, const float *points, const float *tris, float *sdf, void *workspace,
                             hipStream_t s) {
    const dim3 block(kMeshBlock);
    if (t == 0) {
        hipLaunchKernelGGL(mesh_fill_kernel<false>, mesh_per_point(n), block, 0, s, (uint2 *)nullptr, sdf, n);
        return hipGetLastError();
    }
#if MESH_SDF_PLAIN
    hipLaunchKernelGGL(mesh_sdf_plain_kernel, mesh_per_point(n), block, 0, s, points, tris, (int32_t)t, sdf, n);
    return hipGetLastError();
#else
    TriRecord *rec = static_cast<TriRecord *>(workspace);
    uint2 *acc = mesh_accumulators<uint2>(workspace, t);
    int32_t chunk_len = 0, chunks = 0;
    mesh_chunks(n, (int32_t)(t < kMeshPass ? t : kMeshPass), chunk_len, chunks);
    const bool final_in_pair = t <= kMeshPass && chunks == 1;
    if (!final_in_pair) {
        hipLaunchKernelGGL(mesh_fill_kernel<false>, mesh_per_point(n), block, 0, s, acc, sdf, n);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const hipError_t e = mesh_passes(final_in_pair ? mesh_pair_kernel<false, true, true> : mesh_pair_kernel<false, true, false>,
                                     n, t, points, tris, rec, acc, sdf, s);
    if (e != hipSuccess || final_in_pair) return e;
    hipLaunchKernelGGL(mesh_sdf_finish_kernel, mesh_per_point(n), block, 0, s, acc, sdf, n);
    return hipGetLastError();
#endif
}

// with t == 0 the call still fills and finishes its accumulators, so only n decides
size_t mesh_closest_workspace(int64_t n, int64_t t) { return n <= 0 ? 0 : mesh_workspace<uint4>(n, t); }

hipError_t mesh_closest_dispatch(int64_t n, int64_t t, const float *points, const float *tris, bool is_signed, float *dist,
                                 float *hit, int32_t *tidx, void *workspace, hipStream_t s) {
    const dim3 block(kMeshBlock);
    TriRecord *rec = static_cast<TriRecord *>(workspace);
    uint4 *acc = mesh_accumulators<uint4>(workspace, t);
    hipLaunchKernelGGL(mesh_fill_kernel<true>, mesh_per_point(n), block, 0, s, acc, (float *)nullptr, n);
    if (hipError_t e = hipGetLastError()) return e;
    const hipError_t e = mesh_passes(is_signed ? mesh_pair_kernel<true, true, false> : mesh_pair_kernel<true, false, false>, n, t,
                                     points, tris, rec, acc, (float *)nullptr, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mesh_closest_finish_kernel, mesh_per_point(n), block, 0, s, points, tris, acc, dist, hit, tidx, n);
    return hipGetLastError();
}

}  // namespace shacira
