// ssim.hip -- structural similarity of two channels-last fp32 images (contract in include/shacira_hip.h, shacira_ssim_forward
// and shacira_ssim_backward): the 11-tap Gaussian window of sigma 1.5, the sample covariance (121 / 120), the mean of the
// per-pixel score over the windows that lie wholly inside the image, the plain mean of that over the channels.
//
//   stencil    one workgroup per (tile of kSsimTh x kSsimTw pixels, channel). The tile and its 5-pixel halo of x and y go into
//              LDS (border pixels by reflection, d c b a | a b c d; shifted by the median of three row means, see below), the
//              horizontal pass writes the five fields G x, G y, G xx, G yy, G xy of the 26 rows into LDS, the vertical pass
//              keeps 14 rows of one column in registers and produces 4 pixels per lane. A wave reads one 64-float LDS row per instruction: 64 lanes, 64 banks. The
//              forward instantiation turns the fields into the score S, adds the valid pixels of the tile in fp64 (lane
//              shuffles, then the four waves in order) into ONE partial per (channel, tile), and writes the full map when
//              asked. The backward instantiation writes dS/dux, dS/duxx, dS/duxy (zero outside the valid region) as planes.
//   finish     one workgroup adds the partials of a channel in a fixed order, divides by the valid pixels, averages the channels.
//   gather     backward: the same tile structure over the three derivative planes with zeros outside the image (the
//              transpose of the valid filter), combined with x and y and scaled by grad / (C * valid pixels).
// No floating-point atomics anywhere: two calls on the same operands give the same bits.
//
// LDS: 2 * 26 * 74 + 5 * 26 * 64 floats = 48 672 bytes for the stencil (three workgroups, 12 waves, per CU of 160 KiB),
// 3 * 26 * 74 + 3 * 26 * 64 floats = 43 056 bytes for the gather.
//
// Nothing here has been timed against another shape of the kernel. The forward's algorithmic traffic is 2 * H * W * C * 4
// bytes -- 15 MB for an 800 x 800 RGB image -- so at that size the call is bound by its two launches, not by the stencil.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "internal.h"

namespace shacira {

namespace {

constexpr int kTh = SHACIRA_SSIM_TILE_H;       // 16
constexpr int kTw = SHACIRA_SSIM_TILE_W;       // 64
constexpr int kRad = 5;                        // int(3.5 * 1.5 + 0.5)
constexpr int kWin = 2 * kRad + 1;
constexpr int kInH = kTh + 2 * kRad;           // 26
constexpr int kInW = kTw + 2 * kRad;           // 74
constexpr int kSsimBlock = 256;
constexpr int kRowsPerLane = kTh / (kSsimBlock / 64);    // 4 output rows per lane in the vertical pass
constexpr int kColRows = kRowsPerLane + 2 * kRad;        // 14 rows of one column in registers
constexpr int kFinishBlock = 1024;
static_assert(kTw == 64, "a wave owns one LDS row of the vertical pass");
static_assert(kTh % (kSsimBlock / 64) == 0, "every wave takes the same number of rows");

struct SsimConst {
    float w[kRad + 1];        // from the edge inwards: w[0] = weight of offset +-5, w[5] = the centre
    float c1, c2, cov;        // (0.01 R)^2, (0.03 R)^2, 121 / 120
};

SsimConst ssim_constants(float data_range) {
    SsimConst k;
    double e[kRad + 1], sum = 0.0;
    for (int i = 0; i <= kRad; ++i) {
        const double d = (double)(kRad - i);
        e[i] = std::exp(-0.5 / (1.5 * 1.5) * d * d);
        sum += i < kRad ? 2.0 * e[i] : e[i];
    }
    for (int i = 0; i <= kRad; ++i) k.w[i] = (float)(e[i] / sum);
    const double r = (double)data_range;
    k.c1 = (float)((0.01 * r) * (0.01 * r));
    k.c2 = (float)((0.03 * r) * (0.03 * r));
    k.cov = (float)(121.0 / 120.0);
    return k;
}

// index i of an axis of n >= 11 pixels read through scipy's 'reflect' border; beyond the 5-pixel halo of the image (the part of a
// last tile that hangs over the edge, never written) any pixel of the image
__device__ __forceinline__ int64_t reflect_index(int64_t i, int64_t n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : i;
}

// the window over v[0 .. 10]: the small outer pairs first, the centre last, so that the one rounding that matters is the last
// add. The fused multiply-adds are meant: one rounding per tap.
__device__ __forceinline__ float window11(const float *v, const SsimConst &k) {
    float acc = k.w[0] * (v[0] + v[10]);
#pragma unroll
    for (int i = 1; i < kRad; ++i) acc = fmaf(k.w[i], v[i] + v[10 - i], acc);
    return fmaf(k.w[kRad], v[kRad], acc);
}

// the median of three; fminf / fmaxf return the operand that is a number, so one NaN among the three drops out
__device__ __forceinline__ float median3(float a, float b, float c) {
    return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}

// v of another lane of the row of 16, by a DPP control: the add that takes it costs one VALU instruction and no LDS traffic
template <int kCtrl>
__device__ __forceinline__ float dpp_lane(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), kCtrl, 0xF, 0xF, true));
}

// the mean of v over the 64 lanes of the wave, wave-uniform. Every step adds a lane's partner to it and the partner adds the
// lane, so the lanes of a row of 16 end with the same bits; the four rows are then added in one order.
__device__ __forceinline__ float wave_mean(float v) {
    v += dpp_lane<0xB1>(v);         // quad_perm [1, 0, 3, 2]
    v += dpp_lane<0x4E>(v);         // quad_perm [2, 3, 0, 1]
    v += dpp_lane<0x141>(v);        // row_half_mirror: the other quad of the eight
    v += dpp_lane<0x140>(v);        // row_mirror: the other eight of the row
    float row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) row[i] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16 * i));
    return ((row[0] + row[1]) + (row[2] + row[3])) * (1.f / 64.f);
}

// kGrad false: partials[ch * tiles + tile] = the fp64 sum of S over the tile's valid pixels; map (may be NULL) [H, W, C].
// kGrad true:  planes [3][C][H][W] = dS/dux, dS/duxx, dS/duxy, zero outside the valid region.
template <bool kGrad>
__global__ void __launch_bounds__(kSsimBlock) ssim_stencil_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                  int64_t H, int64_t W, int cin, int C, int64_t tiles_x,
                                                                  SsimConst k, double *__restrict__ partials,
                                                                  float *__restrict__ map, float *__restrict__ planes) {
    __shared__ float sx[kInH][kInW];
    __shared__ float sy[kInH][kInW];
    __shared__ float sh[5][kInH][kTw];
    __shared__ double swave[kSsimBlock / 64];
    const int tid = (int)threadIdx.x;
    const int ch = (int)blockIdx.y;
    const int64_t tile = (int64_t)blockIdx.x;
    const int64_t r0 = (tile / tiles_x) * kTh, c0 = (tile % tiles_x) * kTw;
    if (!kGrad && !map && (r0 + kTh <= kRad || r0 >= H - kRad || c0 + kTw <= kRad || c0 >= W - kRad)) {
        if (tid == 0) partials[(int64_t)ch * gridDim.x + tile] = 0.0;       // no valid pixel and no map to write
        return;
    }
    // The fields are taken of x - mx and y - my: variance and covariance do not change under a shift, but the cancellation in
    // uxx - ux * ux does -- on a nearly flat image it leaves the differences of neighbours, not the rounding of 0.49. The means
    // get the shift back below. Any shift is valid, but the whole tile pays for a bad one. One pixel as the shift is bad twice:
    // a pixel of 50 puts 1e-2 into the S of all the tile, one of 1e20 makes it NaN; and on an image around zero (pixels in
    // [-1, 1]) a pixel is far from the mean, so ux = mx + G(x - mx) rounds at the size of mx, ten times what G(x) does. So mx is
    // the median of three row means: the rows are the tile's centre row (clamped to the image) and the ones two and four rows
    // above it, the columns the tile's with its left halo, inside the image -- at least six, the 64 lanes spread over them. A
    // mean is near the tile's, where the shift serves the variances best and never costs the means more than itself; one pixel,
    // whatever it holds, spoils one mean, and the median takes another (fminf / fmaxf pass over a NaN). A median that is still
    // not finite shifts by nothing, so a NaN stays inside its own window. The rows lie in the tile or its halo: equal tiles of
    // x and y shift alike. Every wave forms the same sums in the same order, and forward and backward do it here: one shift
    // per tile.
    const int64_t rc = r0 + kTh / 2 < H ? r0 + kTh / 2 : H - 1;                      // >= 8: the window fits the image
    const int64_t lo = c0 > kRad ? c0 - kRad : 0, hi = c0 + kTw - 1 < W ? c0 + kTw - 1 : W - 1;
    const int64_t pc = lo + (((tid & 63) * (int)(hi - lo + 1)) >> 6);              // the 64 lanes spread over lo .. hi
    float px[3], py[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int64_t at = ((rc - 2 * g) * W + pc) * cin + ch;
        px[g] = x[at];
        py[g] = y[at];
    }
    // A lane's loads of the tile, all of them in flight behind the probes', then one wait: as a loop that loads, waits and
    // stores, the staging is eight memory round trips in a row, and the probes would be a ninth.
    constexpr int kStage = (kInH * kInW + kSsimBlock - 1) / kSsimBlock;        // 8, the last one partial
    float tx[kStage], ty[kStage];
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = tid + j * kSsimBlock < kInH * kInW ? tid + j * kSsimBlock : kInH * kInW - 1;
        const int r = i / kInW, c = i % kInW;
        const int64_t gr = reflect_index(r0 - kRad + r, H), gc = reflect_index(c0 - kRad + c, W);
        const int64_t at = (gr * W + gc) * cin + ch;
        tx[j] = x[at];
        ty[j] = y[at];
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        px[g] = wave_mean(px[g]);
        py[g] = wave_mean(py[g]);
    }
    float mx = median3(px[0], px[1], px[2]), my = median3(py[0], py[1], py[2]);
    mx = fabsf(mx) < INFINITY ? mx : 0.f;
    my = fabsf(my) < INFINITY ? my : 0.f;
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = tid + j * kSsimBlock;
        if (i < kInH * kInW) {
            sx[i / kInW][i % kInW] = tx[j] - mx;
            sy[i / kInW][i % kInW] = ty[j] - my;
        }
    }
    __syncthreads();
    for (int i = tid; i < kInH * kTw; i += kSsimBlock) {
        const int r = i / kTw, c = i % kTw;
        float a[kWin], b[kWin], p[kWin];
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            a[j] = sx[r][c + j];
            b[j] = sy[r][c + j];
        }
        sh[0][r][c] = window11(a, k);
        sh[1][r][c] = window11(b, k);
#pragma unroll
        for (int j = 0; j < kWin; ++j) p[j] = a[j] * a[j];
        sh[2][r][c] = window11(p, k);
#pragma unroll
        for (int j = 0; j < kWin; ++j) p[j] = b[j] * b[j];
        sh[3][r][c] = window11(p, k);
#pragma unroll
        for (int j = 0; j < kWin; ++j) p[j] = a[j] * b[j];
        sh[4][r][c] = window11(p, k);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    float u[5][kRowsPerLane];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        float col[kColRows];
#pragma unroll
        for (int j = 0; j < kColRows; ++j) col[j] = sh[f][wave * kRowsPerLane + j][lane];
#pragma unroll
        for (int o = 0; o < kRowsPerLane; ++o) u[f][o] = window11(col + o, k);
    }
    const int64_t gc = c0 + lane;
    double acc = 0.0;
#pragma unroll
    for (int o = 0; o < kRowsPerLane; ++o) {
        const int64_t gr = r0 + wave * kRowsPerLane + o;
        const bool inside = gr < H && gc < W;
        const bool valid = gr >= kRad && gr < H - kRad && gc >= kRad && gc < W - kRad;
        const float uxx = u[2][o], uyy = u[3][o], uxy = u[4][o];
        const float vx = k.cov * (uxx - u[0][o] * u[0][o]);
        const float vy = k.cov * (uyy - u[1][o] * u[1][o]);
        const float vxy = k.cov * (uxy - u[0][o] * u[1][o]);
        const float ux = mx + u[0][o], uy = my + u[1][o];
        const float a1 = 2.f * ux * uy + k.c1, a2 = 2.f * vxy + k.c2;
        const float b1 = (ux * ux + uy * uy) + k.c1, b2 = (vx + vy) + k.c2;
        const float s = (a1 * a2) / (b1 * b2);
        if (!kGrad) {
            if (valid) acc += (double)s;
            if (map && inside) map[(gr * W + gc) * C + ch] = s;
        } else if (inside) {
            // S as a function of (ux, uxx, uxy), in the shape that is exactly zero where it must be: at x == y the quotients
            // P, Q, S are exactly 1, both brackets of d_ux vanish and d_uxy == -2 d_uxx to the bit
            const float P = a1 / b1, Q = a2 / b2;
            const float d_ux = 2.f * (uy * Q - ux * s) / b1 + (2.f * k.cov) * (ux * s - uy * P) / b2;
            const float d_uxx = -(k.cov * s) / b2;
            const float d_uxy = ((2.f * k.cov) * P) / b2;
            const int64_t plane = H * W, at = (int64_t)ch * plane + gr * W + gc;
            planes[at] = valid ? d_ux : 0.f;
            planes[(int64_t)C * plane + at] = valid ? d_uxx : 0.f;
            planes[2 * (int64_t)C * plane + at] = valid ? d_uxy : 0.f;
        }
    }
    if (!kGrad) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d);
        if (lane == 0) swave[wave] = acc;
        __syncthreads();
        if (tid == 0) partials[(int64_t)ch * gridDim.x + tile] = ((swave[0] + swave[1]) + swave[2]) + swave[3];
    }
}

// value[0] = mean over the channels of (sum of the channel's partials / valid pixels). Thread t adds partials t, t + 1024, ...
// in that order, the 1024 sums meet in a binary tree: a fixed order
__global__ void __launch_bounds__(kFinishBlock) ssim_finish_kernel(const double *__restrict__ partials, int64_t tiles, int C,
                                                                   double valid_pixels, double *__restrict__ value) {
    __shared__ double part[kFinishBlock];
    double total = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        double sum = 0.0;
        for (int64_t i = threadIdx.x; i < tiles; i += kFinishBlock) sum += partials[(int64_t)ch * tiles + i];
        part[threadIdx.x] = sum;
        __syncthreads();
        for (int d = kFinishBlock / 2; d > 0; d >>= 1) {
            if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
            __syncthreads();
        }
        total += part[0] / valid_pixels;
        __syncthreads();
    }
    if (threadIdx.x == 0) value[0] = total / (double)C;
}

// grad_x [H, W, cin] = scale * (Gt[d_ux] + 2 x Gt[d_uxx] + y Gt[d_uxy]) for the channels below C, zero for the others;
// scale = grad[0] / (C * valid pixels). Gt: the window over the planes with zeros outside the image
__global__ void __launch_bounds__(kSsimBlock) ssim_gather_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                 const float *__restrict__ planes,
                                                                 const float *__restrict__ grad, int64_t H, int64_t W, int cin,
                                                                 int C, int64_t tiles_x, SsimConst k, double inv_count,
                                                                 float *__restrict__ grad_x) {
    __shared__ float sd[3][kInH][kInW];
    __shared__ float sm[3][kInH][kTw];
    const int tid = (int)threadIdx.x;
    const int ch = (int)blockIdx.y;
    const int64_t tile = (int64_t)blockIdx.x;
    const int64_t r0 = (tile / tiles_x) * kTh, c0 = (tile % tiles_x) * kTw;
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t gc = c0 + lane;
    if (ch >= C) {
#pragma unroll
        for (int o = 0; o < kRowsPerLane; ++o) {
            const int64_t gr = r0 + wave * kRowsPerLane + o;
            if (gr < H && gc < W) grad_x[(gr * W + gc) * cin + ch] = 0.f;
        }
        return;
    }
    const int64_t plane = H * W;
    for (int i = tid; i < kInH * kInW; i += kSsimBlock) {
        const int r = i / kInW, c = i % kInW;
        const int64_t gr = r0 - kRad + r, gcc = c0 - kRad + c;
        const bool in = gr >= 0 && gr < H && gcc >= 0 && gcc < W;
        const int64_t at = (int64_t)ch * plane + gr * W + gcc;
#pragma unroll
        for (int f = 0; f < 3; ++f) sd[f][r][c] = in ? planes[(int64_t)f * C * plane + at] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < kInH * kTw; i += kSsimBlock) {
        const int r = i / kTw, c = i % kTw;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            float a[kWin];
#pragma unroll
            for (int j = 0; j < kWin; ++j) a[j] = sd[f][r][c + j];
            sm[f][r][c] = window11(a, k);
        }
    }
    __syncthreads();
    float g[3][kRowsPerLane];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        float col[kColRows];
#pragma unroll
        for (int j = 0; j < kColRows; ++j) col[j] = sm[f][wave * kRowsPerLane + j][lane];
#pragma unroll
        for (int o = 0; o < kRowsPerLane; ++o) g[f][o] = window11(col + o, k);
    }
    const float scale = (float)((double)grad[0] * inv_count);
#pragma unroll
    for (int o = 0; o < kRowsPerLane; ++o) {
        const int64_t gr = r0 + wave * kRowsPerLane + o;
        if (gr < H && gc < W) {
            const int64_t at = (gr * W + gc) * cin + ch;
            grad_x[at] = scale * ((g[0][o] + (2.f * x[at]) * g[1][o]) + y[at] * g[2][o]);
        }
    }
}

int64_t ssim_tiles_x(int64_t W) { return (W + kTw - 1) / kTw; }

}  // namespace

int64_t ssim_tiles(int64_t H, int64_t W) { return ((H + kTh - 1) / kTh) * ssim_tiles_x(W); }

// forward: one fp64 partial per (channel, tile); backward: the three derivative planes [3][C][H][W] fp32
size_t ssim_workspace(int64_t H, int64_t W, int C, bool backward) {
    return backward ? (size_t)3 * (size_t)C * (size_t)H * (size_t)W * sizeof(float)
                    : (size_t)C * (size_t)ssim_tiles(H, W) * sizeof(double);
}

hipError_t ssim_forward_dispatch(int64_t H, int64_t W, int cin, int C, const float *x, const float *y, float data_range,
                                 double *value, float *map, void *workspace, hipStream_t s) {
    const SsimConst k = ssim_constants(data_range);
    const int64_t tiles = ssim_tiles(H, W);
    double *partials = static_cast<double *>(workspace);
    hipLaunchKernelGGL(ssim_stencil_kernel<false>, dim3((uint32_t)tiles, (uint32_t)C), dim3(kSsimBlock), 0, s, x, y, H, W, cin,
                       C, ssim_tiles_x(W), k, partials, map, (float *)nullptr);
    if (hipError_t e = hipGetLastError()) return e;
    const double valid = (double)(H - 2 * kRad) * (double)(W - 2 * kRad);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(kFinishBlock), 0, s, partials, tiles, C, valid, value);
    return hipGetLastError();
}

hipError_t ssim_backward_dispatch(int64_t H, int64_t W, int cin, int C, const float *x, const float *y, float data_range,
                                  const float *grad, float *grad_x, void *workspace, hipStream_t s) {
    const SsimConst k = ssim_constants(data_range);
    const int64_t tiles = ssim_tiles(H, W);
    float *planes = static_cast<float *>(workspace);
    hipLaunchKernelGGL(ssim_stencil_kernel<true>, dim3((uint32_t)tiles, (uint32_t)C), dim3(kSsimBlock), 0, s, x, y, H, W, cin,
                       C, ssim_tiles_x(W), k, (double *)nullptr, (float *)nullptr, planes);
    if (hipError_t e = hipGetLastError()) return e;
    const double inv_count = 1.0 / ((double)C * (double)(H - 2 * kRad) * (double)(W - 2 * kRad));
    hipLaunchKernelGGL(ssim_gather_kernel, dim3((uint32_t)tiles, (uint32_t)cin), dim3(kSsimBlock), 0, s, x, y, planes, grad, H,
                       W, cin, C, ssim_tiles_x(W), k, inv_count, grad_x);
    return hipGetLastError();
}

}  // namespace shacira
