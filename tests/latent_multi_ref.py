"""fp64 restatement of the selector decoder (MultiLatentDecoder without hidden layers). TEST INFRASTRUCTURE ONLY.

Written from the contract comment above ``multi_decode_kernel`` (shacira_amd/csrc/latent.hip) and the module
``wisp/models/latent_decoders/multi_latent_decoder.py``:

    a_soft = softmax_k(alpha[:, r] / T);  a = onehot(first argmax) if straight_through else a_soft   (gradient: identity)
    q      = rint(latent) (half to even), or the SGA sample (oracle.latent.sga_quantise);  x = q / div
    'dft': per_k = (x @ dft) * scale_k + shift_k;           y = sum_k per_k a_k
    'sq' : mixed = sum_k (x @ scale_k) a_k;  per_k = mixed + shift_k;  y = sum_k per_k a_k      (mixes twice, as the reference)
    out  = clamp(y, -c, c) when c > 0; the clamp passes the gradient on the closed interval [-c, c]

Everything is float64; nothing is cast. Besides each value the functions return the sum of the absolute values of the terms
that form it (``*_abs``): the scale a rounding bound needs. ``q_tol`` / ``dq_tol`` (absolute tolerances of the quantised latent
and of its derivative, for the SGA path whose fp32 evaluation is ill-conditioned at small temperatures) are carried to
every output they reach, to first order and with absolute weights, as ``*_qtol``.
"""
import numpy as np

from oracle import latent as ol


def selector(alpha, temperature, straight_through):
    """alpha [K, R] -> (a_soft, a) both [K, R] float64; ties go to the first maximum, as torch.argmax."""
    al = alpha.astype(np.float64) / float(temperature)
    e = np.exp(al - al.max(0, keepdims=True))
    asoft = e / e.sum(0, keepdims=True)
    if not straight_through:
        return asoft, asoft
    a = np.zeros_like(asoft)
    a[np.argmax(al, axis=0), np.arange(al.shape[1])] = 1.0
    return asoft, a


def quantise(latent, uniforms, temperature, diff_sampling):
    """-> (q, dq/dw) float64 [R, LD]."""
    if uniforms is None:
        return np.rint(latent.astype(np.float64)), np.ones(latent.shape, np.float64)
    # sga_quantise works in float64 and rounds q to float32 on return: redo the last line to keep all 53 bits
    w = latent.astype(np.float64)
    _, dq = ol.sga_quantise(latent, uniforms, temperature, diff_sampling)
    s0, s1 = sga_weights(latent, uniforms, temperature)
    wf = np.floor(w)
    return wf * s0 + (wf + 1.0) * s1, dq


def sga_scores(latent, uniforms, temperature):
    """The two scores of the relaxed choice and Z >= |z0| + |z1| with every addend taken absolutely (float64)."""
    w = latent.astype(np.float64)
    T = float(temperature)
    lim = float(np.float32(1.0 - 1e-6))
    wf = np.floor(w)
    lf = -np.tanh(np.clip(w - wf, -lim, lim)) / T
    lc = -np.tanh(np.clip(wf + 1.0 - w, -lim, lim)) / T
    eps = float(np.finfo(np.float32).eps)
    g = -np.log(-np.log(np.clip(uniforms.astype(np.float64), eps, 1.0 - eps)))
    z0, z1 = (lf + g[..., 0]) / T, (lc + g[..., 1]) / T
    Z = (np.abs(lf) + np.abs(g[..., 0]) + np.abs(lc) + np.abs(g[..., 1]) + 2.0) / T
    return z0, z1, Z


def sga_weights(latent, uniforms, temperature):
    """(s0, s1) = softmax of the two scores, each from its own formula so that a weight of 1e-28 keeps its digits."""
    z0, z1, _ = sga_scores(latent, uniforms, temperature)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(z1 - z0)), 1.0 / (1.0 + np.exp(z0 - z1))


C_SGA = 12


def sga_tolerances(latent, uniforms, temperature, diff_sampling):
    """Absolute tolerances (q_tol, dq_tol) [R, LD] of a float32 evaluation of the SGA sample and of its derivative.

    The sample is q = wf s0 + wc s1 with s_i = exp(z_i - lse(z)); an ABSOLUTE error d in an exponent is a RELATIVE error d of
    s_i, and the exponents are as large as Z = (|logit_f| + |g0| + |logit_c| + |g1| + 2) / T (340 at T = 0.05), so the fp32
    sample is only good to ~ eps32 Z. Roundings that reach one exponent, in units of eps32 Z (C_SGA = 12):
      z_i = (logit + g) / T: tanh 2, its division by T 1, log(-log u) 2 (the inner log's 2 ulp become an absolute 2 eps32 of
      the outer one) + 1, the sum 1, the division 1 -> at most 6, as the two scores of Z share them;
      lse = m + log(sum): the two exp 2, the log 1, the sum 1 -> 4 (absolute, <= eps32 Z);  z_i - lse: 1;  exp: 1.
    q then moves by C_SGA eps32 Z (|wf| s0 + |wc| s1) -- the weights no longer add up to one -- and is rounded twice more.
    dq = s0 s1 (...) / T^2 (diff_sampling) carries both weights' relative errors and 8 more roundings (two tanh^2, the
    bracket, the products, the division); dq = s0 + s1 otherwise carries one weight's and 2."""
    _, _, Z = sga_scores(latent, uniforms, temperature)
    s0, s1 = sga_weights(latent, uniforms, temperature)
    q, dq = quantise(latent, uniforms, temperature, diff_sampling)
    wf = np.floor(latent.astype(np.float64))
    eps = float(np.finfo(np.float32).eps)
    q_tol = eps * (C_SGA * Z * (np.abs(wf) * s0 + np.abs(wf + 1.0) * s1) + 2.0 * np.abs(q))
    dq_tol = eps * ((2 * C_SGA * Z + 8.0) if diff_sampling else (C_SGA * Z + 2.0)) * np.abs(dq)
    return q_tol, dq_tol


def forward(latent, alpha, uniforms, temperature, straight_through, diff_sampling, div, scale, dft, shift, clamp_weights,
            q_tol=None):
    """-> dict(out, y (before the clamp), y_abs, y_qtol); scale [K, S, F], shift [K, F] or None, dft [LD, F] or None."""
    scale = scale.astype(np.float64)
    K, _, F = scale.shape
    dft = None if dft is None else dft.astype(np.float64)
    sh = np.zeros((K, F)) if shift is None else shift.reshape(K, F).astype(np.float64)
    d = div.astype(np.float64).reshape(1, -1)
    _, a = selector(alpha, temperature, straight_through)
    q, _ = quantise(latent, uniforms, temperature, diff_sampling)
    x = q / d
    xt = np.zeros_like(x) if q_tol is None else q_tol / np.abs(d)
    asum = a.sum(0)[:, None]
    if dft is not None:
        zm = x @ dft
        sc = scale[:, 0, :]                                                                   # [K, F]
        y = ((zm[None] * sc[:, None, :] + sh[:, None, :]) * a[:, :, None]).sum(0)
        lin = lambda v: (((v @ np.abs(dft))[None] * np.abs(sc)[:, None, :]) * a[:, :, None]).sum(0)
        y_abs = lin(np.abs(x)) + (np.abs(sh)[:, None, :] * a[:, :, None]).sum(0)
    else:
        u = np.stack([x @ scale[k] for k in range(K)])
        mixed = (u * a[:, :, None]).sum(0)
        y = ((mixed[None] + sh[:, None, :]) * a[:, :, None]).sum(0)
        lin = lambda v: asum * (np.stack([v @ np.abs(scale[k]) for k in range(K)]) * a[:, :, None]).sum(0)
        y_abs = lin(np.abs(x)) + (np.abs(sh)[:, None, :] * a[:, :, None]).sum(0)
    out = np.clip(y, -clamp_weights, clamp_weights) if clamp_weights > 0 else y
    return dict(out=out, y=y, y_abs=y_abs, y_qtol=lin(xt))


def backward(latent, alpha, uniforms, temperature, straight_through, diff_sampling, div, scale, dft, shift, clamp_weights,
             grad_out, q_tol=None, dq_tol=None):
    """-> dict of grad_latent [R, LD], grad_alpha [K, R], grad_scale [K, S, F], grad_shift [K, F], each with ``_abs``
    (sum of the absolute terms) and ``_qtol`` (what q_tol / dq_tol can move it by)."""
    scale = scale.astype(np.float64)
    K, S, F = scale.shape
    T = float(temperature)
    dft = None if dft is None else dft.astype(np.float64)
    sh = np.zeros((K, F)) if shift is None else shift.reshape(K, F).astype(np.float64)
    d = div.astype(np.float64).reshape(1, -1)
    asoft, a = selector(alpha, temperature, straight_through)
    q, dq = quantise(latent, uniforms, temperature, diff_sampling)
    x = q / d
    xt = np.zeros_like(x) if q_tol is None else q_tol / np.abs(d)
    dqt = np.zeros_like(x) if dq_tol is None else dq_tol
    y = forward(latent, alpha, uniforms, temperature, straight_through, diff_sampling, div, scale, dft, shift, 0.0)["y"]
    g = grad_out.astype(np.float64).copy()
    if clamp_weights > 0:
        g[~((y >= -clamp_weights) & (y <= clamp_weights))] = 0.0          # closed interval passes
    ga = np.abs(g)
    asum = a.sum(0)[:, None]                                               # [R, 1]
    ak = a[:, :, None]                                                     # [K, R, 1]
    r = {}
    r["grad_shift"] = (g[None] * ak).sum(1)
    r["grad_shift_abs"] = (ga[None] * ak).sum(1)
    r["grad_shift_qtol"] = np.zeros((K, F))
    if dft is not None:
        sc = scale[:, 0, :]
        zm, zma, zmt = x @ dft, np.abs(x) @ np.abs(dft), xt @ np.abs(dft)
        r["grad_scale"] = (g[None] * ak * zm[None]).sum(1)[:, None, :]
        r["grad_scale_abs"] = (ga[None] * ak * zma[None]).sum(1)[:, None, :]
        r["grad_scale_qtol"] = (ga[None] * ak * zmt[None]).sum(1)[:, None, :]
        da = (g[None] * (zm[None] * sc[:, None, :] + sh[:, None, :])).sum(2)                      # [K, R]
        da_abs = (ga[None] * (zma[None] * np.abs(sc)[:, None, :] + np.abs(sh)[:, None, :])).sum(2)
        da_t = (ga[None] * zmt[None] * np.abs(sc)[:, None, :]).sum(2)
        dzm = (g[None] * ak * sc[:, None, :]).sum(0)                                             # [R, F]
        dx, dx_abs = dzm @ dft.T, (ga[None] * ak * np.abs(sc)[:, None, :]).sum(0) @ np.abs(dft).T
    else:
        u = np.stack([x @ scale[k] for k in range(K)])
        ua = np.stack([np.abs(x) @ np.abs(scale[k]) for k in range(K)])
        ut = np.stack([xt @ np.abs(scale[k]) for k in range(K)])
        mixed, mixa, mixt = (u * ak).sum(0), (ua * ak).sum(0), (ut * ak).sum(0)
        du = g[None] * asum[None] * ak                                                          # [K, R, F]
        dua = np.abs(du)
        r["grad_scale"] = np.einsum("rc,krj->kcj", x, du)
        r["grad_scale_abs"] = np.einsum("rc,krj->kcj", np.abs(x), dua)
        r["grad_scale_qtol"] = np.einsum("rc,krj->kcj", xt, dua)
        da = (g[None] * (mixed[None] + sh[:, None, :] + asum[None] * u)).sum(2)
        da_abs = (ga[None] * (mixa[None] + np.abs(sh)[:, None, :] + asum[None] * ua)).sum(2)
        da_t = (ga[None] * (mixt[None] + asum[None] * ut)).sum(2)
        dx = np.einsum("krj,kcj->rc", du, scale)
        dx_abs = np.einsum("krj,kcj->rc", dua, np.abs(scale))
    # through the softmax; the straight-through one-hot hands its gradient to the soft weights unchanged
    r["grad_alpha"] = asoft * (da - (asoft * da).sum(0, keepdims=True)) / T
    r["grad_alpha_abs"] = asoft * (da_abs + (asoft * da_abs).sum(0, keepdims=True)) / T
    r["grad_alpha_qtol"] = asoft * (da_t + (asoft * da_t).sum(0, keepdims=True)) / T
    r["grad_latent"] = dx / d * dq
    r["grad_latent_abs"] = dx_abs / np.abs(d) * np.abs(dq)
    r["grad_latent_qtol"] = dx_abs / np.abs(d) * dqt
    return r
