"""One Adam step in numpy float64 (torch.optim.Adam, amsgrad=False, maximize=False, L2 weight decay folded into the gradient)
and the single-step bars the GPU tests hold the fused kernels to. TEST INFRASTRUCTURE ONLY.

The C-ABI takes the hyper-parameters as floats, so they are rounded to fp32 first; the two bias-correction factors
lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) are formed in double and then rounded to fp32, as the kernels do. Everything else is
exact to double precision: the kernels' fp32 arithmetic is what the bars measure.
"""
import numpy as np


def _f32(x):
    return float(np.float32(x))


def adam_step(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """State (p, g, m, v) before step number t (1-based) -> (p, m, v, scale) float64. `scale` is the size of the update before
    the two terms of exp_avg cancel, lr / bc1 * (|b1 m| + |(1 - b1) g'|) / denom >= |p_before - p_after|: the unit the error
    of p is measured in. (In units of the update itself the figure is meaningless: where b1 m and (1 - b1) g' cancel the
    update is as small as the rounding of its terms, and CPU torch fp32 Adam is then 3% to 13% "off" on 4M random elements.)"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = _f32(lr), _f32(b1), _f32(b2), _f32(eps), _f32(wd)
    lr_over_bc1 = _f32(lr / (1.0 - b1 ** float(t)))
    inv_sqrt_bc2 = _f32(1.0 / np.sqrt(1.0 - b2 ** float(t)))
    gr = g + wd * p
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    denom = np.sqrt(v1) * inv_sqrt_bc2 + eps
    scale = lr_over_bc1 * ((np.abs(b1 * m) + np.abs((1.0 - b1) * gr)) / denom)
    return p - lr_over_bc1 * (m1 / denom), m1, v1, scale


def moment_bars(p, g, m, v, b1=0.9, b2=0.999, wd=0.0):
    """The absolute bars on exp_avg and exp_avg_sq after one step from fp32 state: 2^-22 of the magnitudes that are added."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2, wd = _f32(b1), _f32(b2), _f32(wd)
    gr = g + wd * p
    return (2.0 ** -22 * (np.abs(b1 * m) + np.abs((1.0 - b1) * gr)),
            2.0 ** -22 * (np.abs(b2 * v) + np.abs((1.0 - b2) * gr * gr)))


def update_error(p_got, p0, p_ref, scale):
    """The error of a stepped parameter in units of `scale`, after taking off the rounding of p itself (2^-23 |p0|); 0 where
    the scale is 0 (no update at all)."""
    err = np.abs(np.asarray(p_got, np.float64) - p_ref) - 2.0 ** -23 * np.abs(np.asarray(p0, np.float64))
    return np.where(scale > 0, np.maximum(err, 0.0) / np.where(scale > 0, scale, 1.0), 0.0)


def torch_single_step(p0, g, m0, v0, t, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """CPU torch.optim.Adam (fp32, foreach=False) stepped once from the same state: the yardstick for the update allowance."""
    import torch
    lr, b1, b2, eps, wd = _f32(lr), _f32(b1), _f32(b2), _f32(eps), _f32(wd)    # the values the ABI would carry
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, np.float32)))
    p.grad = torch.from_numpy(np.array(g, np.float32))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m0, np.float32)),
                    "exp_avg_sq": torch.from_numpy(np.array(v0, np.float32))}
    opt.step()
    return p.detach().numpy()


def update_allowance(p0, g, m0, v0, t, **hyper):
    """(allowance, measured): four times the worst error of CPU torch fp32 Adam on these inputs in units of the update scale -- the
    factor covers another contraction and operation order -- and never below 2^-21."""
    p_ref, _, _, scale = adam_step(p0, g, m0, v0, t, **hyper)
    measured = float(update_error(torch_single_step(p0, g, m0, v0, t, **hyper), p0, p_ref, scale).max()) if np.size(p0) else 0.0
    return max(4.0 * measured, 2.0 ** -21), measured
