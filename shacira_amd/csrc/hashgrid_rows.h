// hashgrid_rows.h -- table-row loads shared by the forward (hashgrid_fwd.hip) and the coordinate backward
// (hashgrid_coord_grad.hip): one row as one vector access, and the masked form for lanes that may have no row.
#pragma once

#include "hashgrid_device.h"

namespace shacira {

template <typename T, int F> struct RowVec;  // one table row as a single vector access
template <> struct RowVec<float, 2> { using type = float2; };
template <> struct RowVec<float, 4> { using type = float4; };
template <> struct RowVec<__half, 2> { using type = uint32_t; };
template <> struct RowVec<__half, 4> { using type = uint2; };
template <> struct RowVec<__half, 8> { using type = uint4; };

template <typename T, int F> __device__ __forceinline__ void load_row(const T *p, float (&v)[F]) {
    if constexpr (sizeof(T) == 4 && F == 2) {
        float2 r = *reinterpret_cast<const float2 *>(p);
        v[0] = r.x; v[1] = r.y;
    } else if constexpr (sizeof(T) == 4 && F == 4) {
        float4 r = *reinterpret_cast<const float4 *>(p);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else if constexpr (sizeof(T) == 2 && F == 2) {
        __half2 r = *reinterpret_cast<const __half2 *>(p);
        v[0] = __low2float(r); v[1] = __high2float(r);
    } else {
#pragma unroll
        for (int j = 0; j < F; ++j) v[j] = Scalar<T>::load(p + j);
    }
}

// One table row for a lane that may have none (sample beyond the batch, row beyond the table): the load is UNCONDITIONAL from
// a clamped row and the result is masked afterwards. (Round 4: as `if (ok) load else 0` every gather sat in its own
// lane-dependent branch and the compiler closed each branch with `s_waitcnt vmcnt(0)` -- the four corner gathers of a sample
// went out one round trip after the other instead of together; ISA of hashgrid_fwd_level_pair_kernel.)
template <typename T, int F>
__device__ __forceinline__ void gather_row(const T *__restrict__ table, int64_t grow, bool ok, float (&v)[F]) {
    const int64_t safe = ok ? grow : 0;
    load_row<T, F>(table + safe * F, v);
#pragma unroll
    for (int j = 0; j < F; ++j) v[j] = ok ? v[j] : 0.0f;
}

}  // namespace shacira
