// latent_quant.h -- the SGA quantiser and the NaN-keeping clamp shared by latent.hip and latent_mlp.hip, so that the two
// decoders cannot drift apart (they did: latent_mlp.hip kept an open-mask copy and a fminf(fmaxf()) clamp).
#pragma once
#include <hip/hip_runtime.h>

namespace shacira {

// Stochastic Gumbel annealing (basic_latent_decoder.py:183-191): relaxed one-hot choice between floor(w) and floor(w)+1
// with logits -tanh(distance)/T, sampled as torch's RelaxedOneHotCategorical(T) does from two uniforms per latent:
// u = clamp(rand, eps, 1-eps); g = -log(-log u); score = (logit + g)/T; sample = exp(score - logsumexp(score)).
// dq = d(sample)/dw: rsample() path when `diff` (floor carries no gradient), else straight-through floor (s0 + s1).
__device__ __forceinline__ void sga_quantise(float w, float u0, float u1, float T, bool diff, float &q, float &dq) {
    const float lim = 1.0f - 1e-6f, eps = 1.1920929e-07f;
    const float wf = floorf(w), wc = wf + 1.0f;
    const float a = w - wf, b = wc - w;
    const float tf_ = tanhf(fminf(fmaxf(a, -lim), lim)), tc = tanhf(fminf(fmaxf(b, -lim), lim));
    const float lf = -tf_ / T, lc = -tc / T;
    u0 = fminf(fmaxf(u0, eps), 1.0f - eps);
    u1 = fminf(fmaxf(u1, eps), 1.0f - eps);
    const float z0 = (lf + -logf(-logf(u0))) / T, z1 = (lc + -logf(-logf(u1))) / T;
    const float m = fmaxf(z0, z1);
    const float lse = m + logf(expf(z0 - m) + expf(z1 - m));
    const float s0 = expf(z0 - lse), s1 = expf(z1 - lse);
    q = wf * s0 + wc * s1;
    if (diff) {
        // torch.clamp hands the gradient on at the bounds themselves (w = -0.999999: b == lim)
        const float in_f = (a >= -lim && a <= lim) ? 1.0f : 0.0f, in_c = (b >= -lim && b <= lim) ? 1.0f : 0.0f;
        dq = s0 * s1 * ((1.0f - tc * tc) * in_c + (1.0f - tf_ * tf_) * in_f) / (T * T);
    } else {
        dq = s0 + s1;
    }
}

// torch.clamp(v, -c, c): a NaN stays a NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp_keep_nan(float v, float c) { return v < -c ? -c : (v > c ? c : v); }

}  // namespace shacira
