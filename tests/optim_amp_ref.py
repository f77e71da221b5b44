"""One RMSprop step in numpy float64 (torch.optim.RMSprop, centered=False, maximize=False, L2 weight decay folded into the
gradient) and the single-step bars the GPU tests hold the fused kernel to; the loss-scaled Adam reference. TEST INFRASTRUCTURE
ONLY. The rules are adam_ref's: hyper-parameters rounded to fp32 first (the C-ABI carries floats), everything else exact to
double precision, so that the kernels' fp32 arithmetic is what the bars measure.
"""
import numpy as np

import adam_ref
from adam_ref import _f32


def rmsprop_step(p, g, sq, buf, lr, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0):
    """State (p, g, square_avg, momentum_buffer) -> (p, sq, buf, scale) float64; `buf` may be None when momentum == 0 and comes
    back as None then. `scale` = lr (|momentum buf0| + |g'| / avg) >= |p_before - p_after| is the size of the update before the
    two terms of the momentum buffer cancel: the unit the error of p is measured in (adam_ref.adam_step explains why)."""
    p, g, sq = (np.asarray(a, np.float64) for a in (p, g, sq))
    lr, alpha, eps, wd, momentum = _f32(lr), _f32(alpha), _f32(eps), _f32(wd), _f32(momentum)
    gr = g + wd * p
    sq1 = alpha * sq + (1.0 - alpha) * gr * gr
    avg = np.sqrt(sq1) + eps
    if momentum > 0:
        buf0 = np.asarray(buf, np.float64)
        buf1 = momentum * buf0 + gr / avg
        return p - lr * buf1, sq1, buf1, lr * (np.abs(momentum * buf0) + np.abs(gr) / avg)
    return p - lr * (gr / avg), sq1, None, lr * (np.abs(gr) / avg)


def state_bars(p, g, sq, buf, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0):
    """The absolute bars on square_avg and momentum_buffer after one step from fp32 state: 2^-22 of the magnitudes that are
    added. (sq bar, buf bar); the buf bar is None when momentum == 0."""
    p, g, sq = (np.asarray(a, np.float64) for a in (p, g, sq))
    alpha, eps, wd, momentum = _f32(alpha), _f32(eps), _f32(wd), _f32(momentum)
    gr = g + wd * p
    sq1 = alpha * sq + (1.0 - alpha) * gr * gr
    sq_bar = 2.0 ** -22 * (np.abs(alpha * sq) + np.abs((1.0 - alpha) * gr * gr))
    if momentum > 0:
        return sq_bar, 2.0 ** -22 * (np.abs(momentum * np.asarray(buf, np.float64)) + np.abs(gr / (np.sqrt(sq1) + eps)))
    return sq_bar, None


def torch_single_step(p0, g, sq0, buf0, lr, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0):
    """CPU torch.optim.RMSprop (fp32, foreach=False) stepped once from the same state: the yardstick for the update allowance."""
    import torch
    lr, alpha, eps, wd, momentum = _f32(lr), _f32(alpha), _f32(eps), _f32(wd), _f32(momentum)
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, np.float32)))
    p.grad = torch.from_numpy(np.array(g, np.float32))
    opt = torch.optim.RMSprop([p], lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=momentum, foreach=False)
    opt.state[p] = {"step": torch.tensor(0.0), "square_avg": torch.from_numpy(np.array(sq0, np.float32))}
    if momentum > 0:
        opt.state[p]["momentum_buffer"] = torch.from_numpy(np.array(buf0, np.float32))
    opt.step()
    return p.detach().numpy()


def update_allowance(p0, g, sq0, buf0, **hyper):
    """(allowance, measured): four times the worst error of CPU torch fp32 RMSprop on these inputs in units of the update
    scale, never below 2^-21 (adam_ref.update_allowance's rule; the yardstick is torch, not the kernel)."""
    p_ref, _, _, scale = rmsprop_step(p0, g, sq0, buf0, **hyper)
    measured = float(adam_ref.update_error(torch_single_step(p0, g, sq0, buf0, **hyper), p0, p_ref, scale).max()) \
        if np.size(p0) else 0.0
    return max(4.0 * measured, 2.0 ** -21), measured


def scaled_adam_step(p, g_scaled, m, v, t, grad_scale, **hyper):
    """The loss-scaled Adam reference: adam_ref.adam_step applied to g_scaled / grad_scale (the quotient in float64)."""
    return adam_ref.adam_step(p, np.asarray(g_scaled, np.float64) / float(np.float32(grad_scale)), m, v, t, **hyper)
