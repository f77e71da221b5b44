// grid_walk.h -- the one ray walk through the dense [-1, 1]^3 grid of 2^level cells a side (3-D DDA, Amanatides & Woo), shared
// by render.hip (raytrace_dense: every occupied crossing) and spc.hip (spc_first_hit: the first). The two are documented as
// equal bit for bit, so the arithmetic exists here only; tests/golden/grid_walk.npz pins it to recorded device results. The
// header knows nothing about how occupancy is stored: the caller's visitor looks the cell up. Scalars per axis and select
// chains, no array indexed by the runtime axis: no private segment. The step is selects too, not a branch per axis: lanes of a
// wavefront step along different axes, and three divergent blocks cost spc_first_hit a quarter of its time (profiles/spc.md).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace shacira {

// Morton index of a cell, x most significant
__device__ __forceinline__ uint32_t morton_x_major(uint32_t x, uint32_t y, uint32_t z, int level) {
    uint32_t m = 0;
    for (int b = 0; b < level; ++b)
        m |= (((x >> b) & 1u) << (3 * b + 2)) | (((y >> b) & 1u) << (3 * b + 1)) | (((z >> b) & 1u) << (3 * b));
    return m;
}

// one axis of the slab test against [-1, 1]
__device__ __forceinline__ void slab_axis(float o, float d, float &tn, float &tf, bool &miss) {
    if (d == 0.0f) {
        if (o < -1.0f || o > 1.0f) miss = true;
    } else {
        const float inv = 1.0f / d;
        const float t0 = (-1.0f - o) * inv, t1 = (1.0f - o) * inv;
        tn = fmaxf(tn, fminf(t0, t1));
        tf = fminf(tf, fmaxf(t0, t1));
    }
}

// one axis of the walk's set-up: the start cell, the step, the depth of the next crossing and the depth between crossings.
// A start cell that is off by one rounding is skipped by the walk (zero-length stay).
__device__ __forceinline__ void walk_axis(float o, float d, float tin, int G, float cell, int &c, int &step, float &tmax,
                                          float &tdelta) {
    const float p = fmaf(d, tin, o);
    int q = (int)floorf((p + 1.0f) * 0.5f * (float)G);
    q = q < 0 ? 0 : (q > G - 1 ? G - 1 : q);
    c = q;
    if (d > 0.0f) {
        step = 1;
        tdelta = cell / d;
        tmax = ((-1.0f + (float)(q + 1) * cell) - o) / d;
    } else if (d < 0.0f) {
        step = -1;
        tdelta = -cell / d;
        tmax = ((-1.0f + (float)q * cell) - o) / d;
    } else {
        step = 0;
        tdelta = INFINITY;
        tmax = INFINITY;
    }
}

// Calls visit(cx, cy, cz, t_enter, t_exit) once for every cell the ray stays in for a positive length, in depth order (entry
// clipped to 0 for a ray that starts inside the volume); visit returns true to stop the walk. At most 3 G + 3 steps.
template <class Visit>
__device__ __forceinline__ void grid_walk(float ox, float oy, float oz, float dx, float dy, float dz, int level, Visit &&visit) {
    const int G = 1 << level;
    float tn = -INFINITY, tf = INFINITY;
    bool miss = false;
    slab_axis(ox, dx, tn, tf, miss);
    slab_axis(oy, dy, tn, tf, miss);
    slab_axis(oz, dz, tn, tf, miss);
    if (miss || !(tf > fmaxf(tn, 0.0f))) return;
    float t = fmaxf(tn, 0.0f);
    const float cell = 2.0f / (float)G;
    const float tin = t;
    int cx, cy, cz, sx, sy, sz;
    float mx, my, mz, ex, ey, ez;                     // tmax and tdelta per axis
    walk_axis(ox, dx, tin, G, cell, cx, sx, mx, ex);
    walk_axis(oy, dy, tin, G, cell, cy, sy, my, ey);
    walk_axis(oz, dz, tin, G, cell, cz, sz, mz, ez);
    for (int it = 0; it < 3 * G + 3; ++it) {
        const int a = (mx <= my) ? ((mx <= mz) ? 0 : 2) : ((my <= mz) ? 1 : 2);
        const float tm = a == 0 ? mx : (a == 1 ? my : mz);
        const float texit = fminf(tm, tf);
        if (texit > t && visit(cx, cy, cz, t, texit)) return;
        t = fmaxf(t, texit);
        if (tm >= tf) break;
        const int c = (a == 0 ? cx : (a == 1 ? cy : cz)) + (a == 0 ? sx : (a == 1 ? sy : sz));      // c[a] += step[a]
        if (c < 0 || c >= G) break;
        const float m = tm + (a == 0 ? ex : (a == 1 ? ey : ez));                                     // tmax[a] += tdelta[a]
        cx = a == 0 ? c : cx, cy = a == 1 ? c : cy, cz = a == 2 ? c : cz;
        mx = a == 0 ? m : mx, my = a == 1 ? m : my, mz = a == 2 ? m : mz;
    }
}

}  // namespace shacira
