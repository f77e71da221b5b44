// posenc.hip -- the positional-encoding row [prefix | coords | sin | cos] that the decoder MLP reads, written once (contract in
// include/shacira_hip.h, shacira_posenc_forward / _backward / _backward2). With d coordinates, F bands b_k, a prefix of P floats
// and I = d (coordinates included) or 0:
//   col 0 .. P-1              the prefix row, copied
//   col P .. P+I-1            the coordinates, copied
//   col P+I + k*d + j         sin(fl32(coords[j] * b_k))
//   col P+I + d*F + k*d + j   cos(fl32(coords[j] * b_k))
//
//   forward     a workgroup takes tiles of up to 256 rows. Pass one copies prefix and coordinates, one lane per float (per
//               16 bytes of the prefix when pointers and strides allow it); pass two takes one lane per (row, k, j): ONE product,
//               ONE sincosf -- one range reduction for both values -- and two stores. Consecutive lanes are consecutive
//               columns, so a wave's stores are runs of d*F floats.
//   backward    one lane per (row, j): the 2F terms b_k (cos g_sin - sin g_cos) added in k order onto the coordinate's own
//               gradient, from the SAVED sin / cos columns: no trigonometry, no coordinates.
//   backward2   one lane per column of the row: the gradients of the backward with respect to the saved row and to grad_out.
// The row index of a tile's first row is the only 64-bit quantity; inside a tile the flat index is 32-bit. No LDS, no atomics, no
// workspace: two calls give the same bits. The library is built with -ffp-contract=off: every product and sum below is rounded
// once, as written.
//
// sincosf is the device library's (2 ulp class, full-range reduction): __sinf / __cosf lose all accuracy at the arguments a
// 2^9 band reaches. Nothing here has been timed against another shape of the kernel on this file's authority: see
// profiles/posenc.md.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace shacira {

namespace {

constexpr int kPosencBlock = 256;
constexpr int kPosencMaxGrid = 2048;
constexpr int kPosencTileRows = 256;

// m / d for d in 1 .. 4 and m < 2^16 without a division
__device__ __forceinline__ uint32_t div_small(uint32_t m, int d) {
    return d == 1 ? m : d == 2 ? m >> 1 : d == 4 ? m >> 2 : (m * 43691u) >> 17;
}

struct PosencTiles {
    int rows;          // rows per tile: rows * (columns per row) stays below 2^31
    int64_t tiles;
    uint32_t grid;
};

PosencTiles posenc_tiles(int64_t n, int64_t width) {
    PosencTiles t;
    int64_t rows = ((int64_t)1 << 22) / (width > 0 ? width : 1);
    t.rows = (int)(rows < 1 ? 1 : rows > kPosencTileRows ? kPosencTileRows : rows);
    t.tiles = (n + t.rows - 1) / t.rows;
    t.grid = (uint32_t)(t.tiles < kPosencMaxGrid ? t.tiles : kPosencMaxGrid);
    return t;
}

template <bool kVec>
__global__ void __launch_bounds__(kPosencBlock) posenc_forward_kernel(const float *__restrict__ coords, int64_t cstride,
                                                                      const float *__restrict__ prefix, int64_t pstride,
                                                                      const float *__restrict__ bands, float *__restrict__ out,
                                                                      int64_t ostride, int64_t n, int d, int F, int I, int P,
                                                                      int tile_rows, int64_t tiles) {
    const uint32_t pitems = kVec ? (uint32_t)P >> 2 : (uint32_t)P;
    const uint32_t copies = pitems + (uint32_t)I;
    const uint32_t dF = (uint32_t)(d * F);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * tile_rows;
        const uint32_t rows = (uint32_t)(n - r0 < tile_rows ? n - r0 : tile_rows);
        const float *c0 = coords + r0 * cstride;
        const float *p0 = prefix + r0 * pstride;        // P == 0: never read
        float *o0 = out + r0 * ostride;
        if (copies > 0) {
            const uint32_t total = rows * copies;
            for (uint32_t idx = threadIdx.x; idx < total; idx += kPosencBlock) {
                const uint32_t r = idx / copies, c = idx - r * copies;
                float *orow = o0 + (int64_t)r * ostride;
                if (c < pitems) {
                    const float *prow = p0 + (int64_t)r * pstride;
                    if (kVec)
                        reinterpret_cast<uint4 *>(orow)[c] = reinterpret_cast<const uint4 *>(prow)[c];
                    else
                        reinterpret_cast<uint32_t *>(orow)[c] = reinterpret_cast<const uint32_t *>(prow)[c];
                } else {
                    const uint32_t j = c - pitems;
                    reinterpret_cast<uint32_t *>(orow)[(uint32_t)P + j] =
                        reinterpret_cast<const uint32_t *>(c0 + (int64_t)r * cstride)[j];
                }
            }
        }
        const uint32_t total = rows * dF;
        for (uint32_t idx = threadIdx.x; idx < total; idx += kPosencBlock) {
            const uint32_t r = idx / dF, m = idx - r * dF;
            const uint32_t k = div_small(m, d), j = m - k * (uint32_t)d;
            const float arg = c0[(int64_t)r * cstride + j] * bands[k];
            float s, c;
            sincosf(arg, &s, &c);
            float *enc = o0 + (int64_t)r * ostride + (uint32_t)(P + I);
            enc[m] = s;
            enc[dF + m] = c;
        }
    }
}

// grad_coords [n, d] dense. row / grad_out: the forward's layout with their own row strides
__global__ void __launch_bounds__(kPosencBlock) posenc_backward_kernel(const float *__restrict__ row, int64_t rstride,
                                                                       const float *__restrict__ grad_out, int64_t gstride,
                                                                       const float *__restrict__ bands,
                                                                       float *__restrict__ grad_coords, int64_t n, int d, int F,
                                                                       int I, int P, int tile_rows, int64_t tiles) {
    const uint32_t dF = (uint32_t)(d * F);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * tile_rows;
        const uint32_t rows = (uint32_t)(n - r0 < tile_rows ? n - r0 : tile_rows);
        const float *s0 = row + r0 * rstride + (P + I);
        const float *g0 = grad_out + r0 * gstride + P;
        float *out = grad_coords + r0 * d;
        const uint32_t total = rows * (uint32_t)d;
        for (uint32_t idx = threadIdx.x; idx < total; idx += kPosencBlock) {
            const uint32_t r = div_small(idx, d), j = idx - r * (uint32_t)d;
            const float *sn = s0 + (int64_t)r * rstride + j;
            const float *g = g0 + (int64_t)r * gstride + j;
            float acc = I ? g[0] : 0.f;
            g += I;
            for (int k = 0; k < F; ++k) {
                const uint32_t at = (uint32_t)k * (uint32_t)d;
                acc += bands[k] * (sn[dF + at] * g[at] - sn[at] * g[dF + at]);
            }
            out[idx] = acc;
        }
    }
}

// grad_row, grad_grad [n, P + E] dense: the gradients of posenc_backward_kernel's grad_coords . gg with respect to the saved row
// and to grad_out
__global__ void __launch_bounds__(kPosencBlock) posenc_backward2_kernel(const float *__restrict__ gg, const float *__restrict__ row,
                                                                        int64_t rstride, const float *__restrict__ grad_out,
                                                                        int64_t gstride, const float *__restrict__ bands,
                                                                        float *__restrict__ grad_row, float *__restrict__ grad_grad,
                                                                        int64_t n, int d, int F, int I, int P, int tile_rows,
                                                                        int64_t tiles) {
    const uint32_t dF = (uint32_t)(d * F);
    const uint32_t head = (uint32_t)(P + I);
    const uint32_t width = head + 2 * dF;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * tile_rows;
        const uint32_t rows = (uint32_t)(n - r0 < tile_rows ? n - r0 : tile_rows);
        const float *s0 = row + r0 * rstride;
        const float *g0 = grad_out + r0 * gstride;
        const float *gg0 = gg + r0 * d;
        float *orow = grad_row + r0 * (int64_t)width;
        float *ogo = grad_grad + r0 * (int64_t)width;
        const uint32_t total = rows * width;
        for (uint32_t idx = threadIdx.x; idx < total; idx += kPosencBlock) {
            const uint32_t r = idx / width, c = idx - r * width;
            float to_row = 0.f, to_go = 0.f;
            if (c >= head) {
                const bool is_cos = c - head >= dF;
                const uint32_t m = c - head - (is_cos ? dF : 0u);
                const uint32_t k = div_small(m, d), j = m - k * (uint32_t)d;
                const uint32_t other = head + (is_cos ? m : dF + m);       // the column's partner: cos for sin, sin for cos
                const float b = bands[k], w = gg0[r * (uint32_t)d + j];
                const float tr = (b * g0[(int64_t)r * gstride + other]) * w;
                const float tg = (b * s0[(int64_t)r * rstride + other]) * w;
                to_row = is_cos ? tr : -tr;
                to_go = is_cos ? -tg : tg;
            } else if (c >= (uint32_t)P) {
                to_go = gg0[r * (uint32_t)d + (c - (uint32_t)P)];
            }
            orow[idx] = to_row;
            ogo[idx] = to_go;
        }
    }
}

bool aligned16(const void *p, int64_t stride) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (stride & 3) == 0; }

}  // namespace

hipError_t posenc_forward_dispatch(int64_t n, int d, int F, int I, int P, const float *coords, int64_t cstride,
                                   const float *prefix, int64_t pstride, const float *bands, float *out, int64_t ostride,
                                   hipStream_t s) {
    const bool vec = P > 0 && (P & 3) == 0 && aligned16(prefix, pstride) && aligned16(out, ostride);
    const PosencTiles t = posenc_tiles(n, (int64_t)P + I + 2 * d * F);
    if (vec)
        hipLaunchKernelGGL(posenc_forward_kernel<true>, dim3(t.grid), dim3(kPosencBlock), 0, s, coords, cstride, prefix, pstride,
                           bands, out, ostride, n, d, F, I, P, t.rows, t.tiles);
    else
        hipLaunchKernelGGL(posenc_forward_kernel<false>, dim3(t.grid), dim3(kPosencBlock), 0, s, coords, cstride, prefix,
                           pstride, bands, out, ostride, n, d, F, I, P, t.rows, t.tiles);
    return hipGetLastError();
}

hipError_t posenc_backward_dispatch(int64_t n, int d, int F, int I, int P, const float *row, int64_t rstride,
                                    const float *grad_out, int64_t gstride, const float *bands, float *grad_coords,
                                    hipStream_t s) {
    const PosencTiles t = posenc_tiles(n, d);
    hipLaunchKernelGGL(posenc_backward_kernel, dim3(t.grid), dim3(kPosencBlock), 0, s, row, rstride, grad_out, gstride, bands,
                       grad_coords, n, d, F, I, P, t.rows, t.tiles);
    return hipGetLastError();
}

hipError_t posenc_backward2_dispatch(int64_t n, int d, int F, int I, int P, const float *gg, const float *row, int64_t rstride,
                                     const float *grad_out, int64_t gstride, const float *bands, float *grad_row,
                                     float *grad_grad, hipStream_t s) {
    const PosencTiles t = posenc_tiles(n, (int64_t)P + I + 2 * d * F);
    hipLaunchKernelGGL(posenc_backward2_kernel, dim3(t.grid), dim3(kPosencBlock), 0, s, gg, row, rstride, grad_out, gstride,
                       bands, grad_row, grad_grad, n, d, F, I, P, t.rows, t.tiles);
    return hipGetLastError();
}

}  // namespace shacira
