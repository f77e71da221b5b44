// sphere_trace.hip -- find_depth_bound and the fused sphere-trace step over ray packs; the contract is the comment above
// shacira_find_depth_bound in include/shacira_hip.h. One lane per pack (find_depth_bound) or per active slot (step). The
// library is built with -ffp-contract=off: every * and + below rounds once, as the contract states.
#include "internal.h"

namespace shacira {

constexpr int kTraceBlock = 256;

// first nugget i in [c, end) that holds q or lies behind it; -1 if c < 0 or there is none (a NaN q: none)
__device__ __forceinline__ int32_t depth_bound_walk(float q, int32_t c, int32_t end, const float2 *__restrict__ depth) {
    if (c < 0) return -1;
    for (int32_t i = c; i < end; ++i) {
        const float2 d = depth[i];
        if ((q >= d.x && q <= d.y) || q < d.x) return i;
    }
    return -1;
}

__global__ __launch_bounds__(kTraceBlock) void find_depth_bound_kernel(int32_t num_packs, int32_t num_nugs,
                                                                        const float *__restrict__ query,
                                                                        const int32_t *__restrict__ curr,
                                                                        const int32_t *__restrict__ pack_end,
                                                                        const float2 *__restrict__ depth,
                                                                        int32_t *__restrict__ out) {
    const int32_t p = (int32_t)(blockIdx.x * kTraceBlock + threadIdx.x);
    if (p >= num_packs) return;
    out[p] = depth_bound_walk(query[p], curr[p], min(pack_end[p], num_nugs), depth);
}

struct TraceStepArgs {
    int32_t num_packs, num_nugs, num_active, first;
    const int32_t *active_in;
    const float *sdf, *origins, *dirs;
    const float2 *depth;
    const int32_t *pack_end, *pidx;
    float step_size, min_dis, min_dis5, dist_max;
    float *t, *dist, *dist_prev;
    int32_t *curr;
    float *x;
    uint8_t *active, *hit;
    int32_t *active_out;
    float *coords_out;
    int32_t *pidx_out, *count_out, *count_next;
};

__global__ __launch_bounds__(kTraceBlock) void sphere_trace_step_kernel(const TraceStepArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.count_next = 0;   // the following launch's counter: nobody adds to it now
    const int32_t slot = (int32_t)(blockIdx.x * kTraceBlock + threadIdx.x);
    bool survive = false;
    int32_t p = 0, n = 0;
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
    if (slot < a.num_active) p = a.active_in[slot];
    if (slot < a.num_active && p >= 0 && p < a.num_packs) {
        const float o0 = a.origins[3 * (int64_t)p], o1 = a.origins[3 * (int64_t)p + 1], o2 = a.origins[3 * (int64_t)p + 2];
        const float d0 = a.dirs[3 * (int64_t)p], d1 = a.dirs[3 * (int64_t)p + 1], d2 = a.dirs[3 * (int64_t)p + 2];
        const float dist = a.sdf[slot] * a.step_size;
        const float dist_prev = a.first ? dist : a.dist_prev[p];
        float t = a.t[p] + dist;
        x0 = o0 + d0 * t;
        x1 = o1 + d1 * t;
        x2 = o2 + d2 * t;
        const bool hit = fabsf(dist) < a.min_dis || fabsf(dist + dist_prev) * 0.5f < a.min_dis5;
        const bool retire = hit || !(t < a.dist_max);
        a.dist[p] = dist;
        a.dist_prev[p] = retire ? dist_prev : dist;
        a.hit[p] = hit ? 1 : 0;
        if (!retire) {
            const int32_t c = a.curr[p];
            n = depth_bound_walk(t, c, min(a.pack_end[p], a.num_nugs), a.depth);
            if (n >= 0) {
                survive = true;
                if (n != c) {
                    t = a.depth[n].x;
                    x0 = o0 + d0 * t;
                    x1 = o1 + d1 * t;
                    x2 = o2 + d2 * t;
                    a.curr[p] = n;
                }
            }
        }
        a.t[p] = t;
        a.x[3 * (int64_t)p] = x0;
        a.x[3 * (int64_t)p + 1] = x1;
        a.x[3 * (int64_t)p + 2] = x2;
        if (!survive) a.active[p] = 0;
    }
    // wave-aggregated append: one atomic per wave, survivors in lane order
    const uint64_t mask = __ballot(survive);
    if (mask == 0) return;
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)mask) - 1;
    int32_t base = 0;
    if (lane == leader) base = atomicAdd(a.count_out, (int32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (!survive) return;
    const int64_t row = (int64_t)base + (int64_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (row >= a.num_packs) return;   // cannot happen while *count_out started at 0 and no pack is named twice
    a.active_out[row] = p;
    a.coords_out[3 * row] = x0;
    a.coords_out[3 * row + 1] = x1;
    a.coords_out[3 * row + 2] = x2;
    if (a.pidx_out) a.pidx_out[row] = a.pidx[n];
}

hipError_t find_depth_bound_launch(int64_t P, int64_t K, const float *query, const int32_t *curr, const int32_t *pack_end,
                                   const float *depth, int32_t *out, hipStream_t s) {
    const unsigned blocks = (unsigned)((P + kTraceBlock - 1) / kTraceBlock);
    hipLaunchKernelGGL(find_depth_bound_kernel, dim3(blocks), dim3(kTraceBlock), 0, s, (int32_t)P, (int32_t)K, query, curr,
                       pack_end, reinterpret_cast<const float2 *>(depth), out);
    return hipGetLastError();
}

hipError_t sphere_trace_step_launch(int64_t P, int64_t K, int64_t num_active, bool first, const int32_t *active_in,
                                    const float *sdf, const float *origins, const float *dirs, const float *depth,
                                    const int32_t *pack_end, const int32_t *pidx, float step_size, float min_dis,
                                    float dist_max, float *t, float *dist, float *dist_prev, int32_t *curr, float *x,
                                    uint8_t *active, uint8_t *hit, int32_t *active_out, float *coords_out,
                                    int32_t *pidx_out, int32_t *count_out, int32_t *count_next, hipStream_t s) {
    TraceStepArgs a;
    a.num_packs = (int32_t)P; a.num_nugs = (int32_t)K; a.num_active = (int32_t)num_active; a.first = first ? 1 : 0;
    a.active_in = active_in; a.sdf = sdf; a.origins = origins; a.dirs = dirs;
    a.depth = reinterpret_cast<const float2 *>(depth); a.pack_end = pack_end; a.pidx = pidx;
    a.step_size = step_size; a.min_dis = min_dis; a.min_dis5 = 5.0f * min_dis; a.dist_max = dist_max;
    a.t = t; a.dist = dist; a.dist_prev = dist_prev; a.curr = curr; a.x = x; a.active = active; a.hit = hit;
    a.active_out = active_out; a.coords_out = coords_out; a.pidx_out = pidx ? pidx_out : nullptr;
    a.count_out = count_out; a.count_next = count_next;
    const unsigned blocks = (unsigned)((num_active + kTraceBlock - 1) / kTraceBlock);
    hipLaunchKernelGGL(sphere_trace_step_kernel, dim3(blocks), dim3(kTraceBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace shacira
