// hashgrid_coord_terms.h -- per-level, per-feature terms of the coordinate derivatives of the hash-grid lookup, shared by the
// coordinate backward (hashgrid_coord_grad.hip) and its own backward (hashgrid_coord_grad2.hip). Each function is ONE
// expression tree with explicit fmaf (the contracts in include/shacira_hip.h): every kernel that needs a term calls these.
#pragma once

#include "hashgrid_device.h"

namespace shacira {

// One feature of one level: D[a] = sum over the corner pairs of axis a, k0 ascending, of W_a(k0) * (v[k1] - v[k0]), as
// D = d0 * W0, then D = fmaf(d, W, D). W_a(k0) = the other axes' weights (f if the corner's bit is set, g otherwise) as a
// left-to-right product in axis order. Corner k: bit DIM-1-a -> axis a (the forward's corner order).
template <int DIM>
__device__ __forceinline__ void coord_feature_diffs(const float (&f)[DIM], const float (&g)[DIM], const float (&v)[1 << DIM],
                                                    float (&D)[DIM]) {
    constexpr int NC = 1 << DIM;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const int bit = 1 << (DIM - 1 - a);
        bool first = true;
#pragma unroll
        for (int k0 = 0; k0 < NC; ++k0) {
            if (k0 & bit) continue;
            float w = 0.0f;
            bool wfirst = true;
#pragma unroll
            for (int b = 0; b < DIM; ++b) {
                if (b == a) continue;
                const float wb = (k0 & (1 << (DIM - 1 - b))) ? f[b] : g[b];
                w = wfirst ? wb : w * wb;
                wfirst = false;
            }
            const float d = v[k0 | bit] - v[k0];
            D[a] = first ? d * w : fmaf(d, w, D[a]);
            first = false;
        }
    }
}

// Number of axis pairs a < b, and the index of one: 2-D (0,1) -> 0; 3-D (0,1) -> 0, (0,2) -> 1, (1,2) -> 2.
template <int DIM> struct AxisPairs { static constexpr int N = DIM * (DIM - 1) / 2; };
__device__ __forceinline__ constexpr int axis_pair(int a, int b) { return a + b - 1; }

// One feature of one level, the mixed second differences: M[pair(a, b)] = sum_k sigma_a(k) sigma_b(k) W_ab(k) v[k]. With
// q(kc) = (v[a1 b1 kc] - v[a1 b0 kc]) - (v[a0 b1 kc] - v[a0 b0 kc]) for the third axis c at corner bit kc:
//   2-D: M = q;   3-D: M = fmaf(q(1), f[c], q(0) * g[c]).
template <int DIM>
__device__ __forceinline__ void coord_feature_mixed(const float (&f)[DIM], const float (&g)[DIM], const float (&v)[1 << DIM],
                                                    float (&M)[AxisPairs<DIM>::N]) {
    if constexpr (DIM == 2) {
        M[0] = (v[3] - v[2]) - (v[1] - v[0]);
    } else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = a + 1; b < 3; ++b) {
                const int c = 3 - a - b;
                const int ba = 1 << (2 - a), bb = 1 << (2 - b), bc = 1 << (2 - c);
                const float q0 = (v[ba | bb] - v[ba]) - (v[bb] - v[0]);
                const float q1 = (v[ba | bb | bc] - v[ba | bc]) - (v[bb | bc] - v[bc]);
                M[axis_pair(a, b)] = fmaf(q1, f[c], q0 * g[c]);
            }
    }
}

}  // namespace shacira
