// adam.hip -- fused Adam step over a flat fp32 parameter buffer (gfx950). "Next" row f1 of SURVEY.md section 8:
// the step that immediately follows the hash-grid backward in the reference's trainers is torch.optim.Adam over the
// whole table (wisp/trainers/base_trainer.py:206-266 builds the groups, image_trainer.py:355-359 steps), i.e. the
// multi-pass foreach implementation: ~10 elementwise kernels over 48.8 MB each. Here it is ONE streaming pass
// (reads p, g, m, v; writes p, m, v; optionally zeroes g for the next accumulation): 7-8 x 4 bytes per element,
// HBM-bound.
//
// Arithmetic follows torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay folded into the gradient):
//   g' = g + wd*p ; m = b1*m + (1-b1)*g' ; v = b2*v + (1-b2)*g'*g'
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
//
// The multi-tensor kernels also come loss-scaled, for mixed-precision training without a host round trip (the
// reference trains under autocast + GradScaler, wisp/trainers/base_trainer.py:167-168): the gradient is divided by a
// scale read from device memory and the whole step is skipped when a device flag says the scaler found a non-finite
// gradient. RMSprop (nerf_base.yaml's optimizer_type, torch.optim.RMSprop with centered=False) runs on the same frame:
//   g' = g + wd*p ; sq = alpha*sq + (1-alpha)*g'*g' ; avg = sqrt(sq) + eps
//   momentum == 0: p -= lr * g'/avg        otherwise: buf = momentum*buf + g'/avg ; p -= lr*buf
#include <cmath>

#include "internal.h"

namespace shacira {

constexpr int kOptimMaxTensors = 32;

__global__ __launch_bounds__(256) void adam_step_kernel(float *__restrict__ p, float *__restrict__ g,
                                                        float *__restrict__ m, float *__restrict__ v, int64_t n,
                                                        float lr_over_bc1, float b1, float b2, float inv_sqrt_bc2,
                                                        float eps, float wd, int zero_grad, float lr,
                                                        const int32_t *__restrict__ step_dev) {
    if (step_dev) {  // graph-capturable form: the step count lives on the device, corrections computed here
        const double t = (double)step_dev[0];
        lr_over_bc1 = (float)((double)lr / (1.0 - pow((double)b1, t)));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, t)));
    }
    // float4 accesses need all four pointers on 16 bytes; a view into a flat buffer (dist.FlatGradients) is only 4-byte
    // aligned, and then every element goes through the scalar loop (as in adam_multi_kernel)
    const bool aligned = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    const int64_t n4 = aligned ? (n & ~(int64_t)3) : 0;   // elements stepped as float4 groups
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n4; i += stride) {
        float4 pp = *reinterpret_cast<float4 *>(p + i);
        float4 gg = *reinterpret_cast<float4 *>(g + i);
        float4 mm = *reinterpret_cast<float4 *>(m + i);
        float4 vv = *reinterpret_cast<float4 *>(v + i);
        float *pa = &pp.x, *ga = &gg.x, *ma = &mm.x, *va = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gr = ga[k] + wd * pa[k];
            ma[k] = b1 * ma[k] + (1.0f - b1) * gr;
            va[k] = b2 * va[k] + (1.0f - b2) * gr * gr;
            const float denom = sqrtf(va[k]) * inv_sqrt_bc2 + eps;
            pa[k] = pa[k] - lr_over_bc1 * (ma[k] / denom);
        }
        *reinterpret_cast<float4 *>(p + i) = pp;
        *reinterpret_cast<float4 *>(m + i) = mm;
        *reinterpret_cast<float4 *>(v + i) = vv;
        if (zero_grad) *reinterpret_cast<float4 *>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t j = n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const float gr = g[j] + wd * p[j];
        const float mj = b1 * m[j] + (1.0f - b1) * gr;
        const float vj = b2 * v[j] + (1.0f - b2) * gr * gr;
        const float denom = sqrtf(vj) * inv_sqrt_bc2 + eps;
        p[j] = p[j] - lr_over_bc1 * (mj / denom);
        m[j] = mj;
        v[j] = vj;
        if (zero_grad) g[j] = 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Multi-tensor form: up to kOptimMaxTensors parameters (each with its own lr / weight decay) in ONE launch; the
// pointer table travels in the kernarg segment. Block b works on chunk (b - first_block[t]) of tensor t. The table,
// the block-to-tensor search, the chunk loop and the host-side fill are shared by every multi-tensor kernel of this
// file (Adam, loss-scaled Adam, RMSprop); a kernel differs in its Rule, the update of one element in registers.
struct OptimMulti {
    float *p[kOptimMaxTensors], *g[kOptimMaxTensors], *s0[kOptimMaxTensors], *s1[kOptimMaxTensors];  // s0, s1: state
    int64_t n[kOptimMaxTensors];
    float lr[kOptimMaxTensors], wd[kOptimMaxTensors];
    uint32_t first_block[kOptimMaxTensors + 1];
    int count;
};

constexpr int kOptimChunk = 256 * 4 * 8;  // elements per block

__device__ __forceinline__ int optim_tensor_of_block(const OptimMulti &a) {
    int t = 0;
    while (t + 1 < a.count && a.first_block[t + 1] <= blockIdx.x) ++t;
    return t;
}

struct AdamRule {
    static constexpr bool kSecondState = true;
    float lr_over_bc1, b1, b2, inv_sqrt_bc2, eps;
    __device__ AdamRule(float lr, float b1_, float b2_, float eps_, double t) : b1(b1_), b2(b2_), eps(eps_) {
        lr_over_bc1 = (float)((double)lr / (1.0 - pow((double)b1, t)));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, t)));
    }
    __device__ __forceinline__ void operator()(float &p, float gr, float du, float &m, float &v) const {
        const float t = (1.0f - b2) * gr;
        float new_m = (1.0f - b1) * gr, new_v = t * gr;
        if (du != 0.0f) {  // the terms of g' + du, each rounded once (see optim_chunk_step)
            new_m = __fmaf_rn(1.0f - b1, gr, (1.0f - b1) * du);
            new_v = __fmaf_rn(t, gr, 2.0f * t * du);
        }
        m = b1 * m + new_m;
        v = b2 * v + new_v;
        p = p - lr_over_bc1 * (m / (sqrtf(v) * inv_sqrt_bc2 + eps));
    }
};

// torch.optim.RMSprop (centered=False, maximize=False); without momentum there is no second state tensor
template <bool kMomentum>
struct RmspropRule {
    static constexpr bool kSecondState = kMomentum;
    float lr, alpha, eps, momentum;
    __device__ __forceinline__ void operator()(float &p, float gr, float du, float &sq, float &buf) const {
        const float t = (1.0f - alpha) * gr;
        float new_sq = t * gr;
        if (du != 0.0f) new_sq = __fmaf_rn(t, gr, 2.0f * t * du);
        sq = alpha * sq + new_sq;
        const float avg = sqrtf(sq) + eps;
        float q = gr / avg;
        if (du != 0.0f) q = q + __fdividef(__fmaf_rn(-q, avg, gr) + du, avg);   // (g' + du) / avg, rounded once
        if (kMomentum) {
            buf = momentum * buf + q;
            p = p - lr * buf;
        } else {
            p = p - lr * q;
        }
    }
};

// This block's chunk of tensor t. float4 accesses need every pointer on 16 bytes; a view into a flat buffer
// (dist.FlatGradients) is only 4-byte aligned, and then every element goes through the scalar loop.
// kScaled (the loss-scaled entries): the gradient is divided by `scale` first. The quotient gu is an fp32 value of its
// own (__fdiv_rn: never folded into the weight-decay product); it is what `grad` holds afterwards when `write_back` is
// set (p.grad is then the unscaled gradient, as after torch's fused optimizers). The division's remainder is carried
// beside it: du = (g - gu*scale) / scale, the part of g / scale that fp32 drops (the fma gives the remainder exactly).
// A rule adds du's first-order terms to what it accumulates, because g'^2 sees the rounding of gu twice: without du
// the second moment misses the single-step bars of tests/adam_ref.py at scale 1000 (1.1 to 1.3 bars), with it the
// state is as close to the float64 step on g / scale as the unscaled step is to its own. A power-of-two scale leaves
// no remainder, du == 0 selects the unscaled expressions, and no bit of the step changes.
__device__ __forceinline__ float optim_unscale(float g, float scale, float inv_scale, float &du) {
    const float gu = __fdiv_rn(g, scale);
    const float r = __fmaf_rn(-gu, scale, g);
    du = (r != 0.0f && r == r) ? r * inv_scale : 0.0f;   // r is NaN under a non-finite gradient: nothing to carry
    return gu;
}

template <bool kScaled, class Rule>
__device__ __forceinline__ void optim_chunk_step(const OptimMulti &a, int t, const Rule &rule, float scale,
                                                 bool write_back, int zero_grad) {
    const float wd = a.wd[t];
    const float inv_scale = kScaled ? 1.0f / scale : 1.0f;
    float *p = a.p[t], *g = a.g[t], *s0 = a.s0[t], *s1 = Rule::kSecondState ? a.s1[t] : nullptr;
    const int64_t n = a.n[t];
    const int64_t lo = (int64_t)(blockIdx.x - a.first_block[t]) * kOptimChunk;
    const int64_t hi = (lo + kOptimChunk < n) ? lo + kOptimChunk : n;
    const bool aligned = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0);
    int64_t j = lo;
    if (aligned) {  // full float4 groups of this chunk (lo is a multiple of the chunk size)
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (j = lo + (int64_t)threadIdx.x * 4; j < hi4; j += 256 * 4) {
            float4 pp = *reinterpret_cast<float4 *>(p + j);
            float4 gg = *reinterpret_cast<float4 *>(g + j);
            float4 aa = *reinterpret_cast<float4 *>(s0 + j);
            float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
            if (Rule::kSecondState) bb = *reinterpret_cast<float4 *>(s1 + j);
            float *pa = &pp.x, *ga = &gg.x, *s0a = &aa.x, *s1a = &bb.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float du = 0.0f;
                if (kScaled) ga[k] = optim_unscale(ga[k], scale, inv_scale, du);
                const float gr = ga[k] + wd * pa[k];
                rule(pa[k], gr, du, s0a[k], s1a[k]);
            }
            *reinterpret_cast<float4 *>(p + j) = pp;
            *reinterpret_cast<float4 *>(s0 + j) = aa;
            if (Rule::kSecondState) *reinterpret_cast<float4 *>(s1 + j) = bb;
            if (zero_grad) *reinterpret_cast<float4 *>(g + j) = make_float4(0.f, 0.f, 0.f, 0.f);
            else if (kScaled && write_back) *reinterpret_cast<float4 *>(g + j) = gg;
        }
        j = hi4;
    }
    for (j += threadIdx.x; j < hi; j += 256) {
        float pj = p[j], gj = g[j], aj = s0[j], bj = 0.0f;
        if (Rule::kSecondState) bj = s1[j];
        float du = 0.0f;
        if (kScaled) gj = optim_unscale(gj, scale, inv_scale, du);
        const float gr = gj + wd * pj;
        rule(pj, gr, du, aj, bj);
        p[j] = pj;
        s0[j] = aj;
        if (Rule::kSecondState) s1[j] = bj;
        if (zero_grad) g[j] = 0.0f;
        else if (kScaled && write_back) g[j] = gj;
    }
}

// A skipped step (the scaler found a non-finite gradient) leaves p and the state alone; with zero_grad the gradient is
// still cleared, so that a persistent gradient buffer does not carry the inf into the next accumulation.
__device__ __forceinline__ void optim_chunk_clear_grad(const OptimMulti &a, int t) {
    float *g = a.g[t];
    const int64_t n = a.n[t];
    const int64_t lo = (int64_t)(blockIdx.x - a.first_block[t]) * kOptimChunk;
    const int64_t hi = (lo + kOptimChunk < n) ? lo + kOptimChunk : n;
    int64_t j = lo;
    if (((uintptr_t)g & 15) == 0) {
        const int64_t hi4 = lo + ((hi - lo) & ~(int64_t)3);
        for (j = lo + (int64_t)threadIdx.x * 4; j < hi4; j += 256 * 4)
            *reinterpret_cast<float4 *>(g + j) = make_float4(0.f, 0.f, 0.f, 0.f);
        j = hi4;
    }
    for (j += threadIdx.x; j < hi; j += 256) g[j] = 0.0f;
}

__global__ __launch_bounds__(256) void adam_multi_kernel(OptimMulti a, float b1, float b2, float eps, int step,
                                                         const int32_t *__restrict__ step_dev, int zero_grad) {
    const int t = optim_tensor_of_block(a);
    const AdamRule rule(a.lr[t], b1, b2, eps, step_dev ? (double)step_dev[0] : (double)step);
    optim_chunk_step<false>(a, t, rule, 1.0f, false, zero_grad);
}

// The loss-scaled entries. Every workgroup reads *found_inf first: non-zero skips the step. grad_scale NULL: the
// gradients are already unscaled (nothing is written back); found_inf NULL: never skip.
__global__ __launch_bounds__(256) void adam_multi_scaled_kernel(OptimMulti a, float b1, float b2, float eps, int step,
                                                                const int32_t *__restrict__ step_dev,
                                                                const float *__restrict__ grad_scale,
                                                                const float *__restrict__ found_inf, int zero_grad) {
    const int t = optim_tensor_of_block(a);
    if (found_inf && found_inf[0] != 0.0f) {
        if (zero_grad) optim_chunk_clear_grad(a, t);
        return;
    }
    const AdamRule rule(a.lr[t], b1, b2, eps, step_dev ? (double)step_dev[0] : (double)step);
    optim_chunk_step<true>(a, t, rule, grad_scale ? grad_scale[0] : 1.0f, grad_scale != nullptr, zero_grad);
}

template <bool kMomentum, bool kScaled>
__global__ __launch_bounds__(256) void rmsprop_multi_kernel(OptimMulti a, float alpha, float eps, float momentum,
                                                            const float *__restrict__ grad_scale,
                                                            const float *__restrict__ found_inf, int zero_grad) {
    const int t = optim_tensor_of_block(a);
    if (kScaled && found_inf && found_inf[0] != 0.0f) {
        if (zero_grad) optim_chunk_clear_grad(a, t);
        return;
    }
    const RmspropRule<kMomentum> rule{a.lr[t], alpha, eps, momentum};
    optim_chunk_step<kScaled>(a, t, rule, (kScaled && grad_scale) ? grad_scale[0] : 1.0f, grad_scale != nullptr,
                              zero_grad);
}

// Fills the table; returns the number of blocks (0: nothing to launch). s1 may be NULL (no second state tensor).
static uint32_t optim_multi_table(OptimMulti &a, int count, float *const *p, float *const *g, float *const *s0,
                                  float *const *s1, const int64_t *n, const float *lr, const float *wd) {
    uint32_t blocks = 0;
    a.count = count;
    for (int t = 0; t < count; ++t) {
        a.p[t] = p[t]; a.g[t] = g[t]; a.s0[t] = s0[t]; a.s1[t] = s1 ? s1[t] : nullptr;
        a.n[t] = n[t]; a.lr[t] = lr[t]; a.wd[t] = wd[t];
        a.first_block[t] = blocks;
        blocks += (uint32_t)((n[t] + kOptimChunk - 1) / kOptimChunk);
    }
    a.first_block[count] = blocks;
    return blocks;
}

// grad_scale and found_inf both NULL: the plain kernel (what shacira_adam_step_multi launches)
hipError_t adam_multi_launch(int count, float *const *p, float *const *g, float *const *m, float *const *v,
                             const int64_t *n, const float *lr, const float *wd, float b1, float b2, float eps,
                             int step, const int32_t *step_dev, const float *grad_scale, const float *found_inf,
                             int zero_grad, hipStream_t s) {
    OptimMulti a;
    const uint32_t blocks = optim_multi_table(a, count, p, g, m, v, n, lr, wd);
    if (blocks == 0) return hipSuccess;
    if (grad_scale || found_inf)
        hipLaunchKernelGGL(adam_multi_scaled_kernel, dim3(blocks), dim3(256), 0, s, a, b1, b2, eps, step, step_dev,
                           grad_scale, found_inf, zero_grad);
    else
        hipLaunchKernelGGL(adam_multi_kernel, dim3(blocks), dim3(256), 0, s, a, b1, b2, eps, step, step_dev, zero_grad);
    return hipGetLastError();
}

hipError_t rmsprop_multi_launch(int count, float *const *p, float *const *g, float *const *sq, float *const *buf,
                                const int64_t *n, const float *lr, const float *wd, float alpha, float eps,
                                float momentum, const float *grad_scale, const float *found_inf, int zero_grad,
                                hipStream_t s) {
    OptimMulti a;
    const uint32_t blocks = optim_multi_table(a, count, p, g, sq, momentum != 0.0f ? buf : nullptr, n, lr, wd);
    if (blocks == 0) return hipSuccess;
    const bool scaled = grad_scale || found_inf;
    auto kernel = momentum != 0.0f ? (scaled ? rmsprop_multi_kernel<true, true> : rmsprop_multi_kernel<true, false>)
                                   : (scaled ? rmsprop_multi_kernel<false, true> : rmsprop_multi_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, a, alpha, eps, momentum, grad_scale, found_inf, zero_grad);
    return hipGetLastError();
}

hipError_t adam_step_launch(float *p, float *g, float *m, float *v, int64_t n, float lr, float b1, float b2, float eps,
                            float wd, int step, const int32_t *step_dev, int zero_grad, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const double bc1 = step_dev ? 1.0 : 1.0 - std::pow((double)b1, (double)step);
    const double bc2 = step_dev ? 1.0 : 1.0 - std::pow((double)b2, (double)step);
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adam_step_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, p, g, m, v, n, (float)(lr / bc1), b1,
                       b2, (float)(1.0 / std::sqrt(bc2)), eps, wd, zero_grad, lr, step_dev);
    return hipGetLastError();
}

}  // namespace shacira
