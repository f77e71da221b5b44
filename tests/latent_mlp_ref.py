"""float64 restatement of the hidden-layer latent decoder (shacira_amd/csrc/latent_mlp.hip). TEST INFRASTRUCTURE ONLY.

    decoded = clamp(final_act(L_n(act(... act(L_1(q(latent) / div)) ...)))),   L_k(x) = x @ W_k + b_k

numpy, explicit matmuls, explicit backward formulas; parameters in the C-ABI's packed layout: per layer W_k [in, out]
row-major, then b_k [out]. ``widths`` = (latent_dim, hidden..., feature_dim). q = rint (half to even, straight-through) or the
SGA sample (latent_multi_ref.quantise). Activations: none, sigmoid, tanh, relu, sine = sin(30 z).

ReLU and the clamp mask follow the rule at the top of tests/mlp_ref.py (what torch does): forward ``0 where z <= 0, else z``
(a NaN stays), backward a SELECT on ``h <= 0`` (an off unit gives an exact 0 under any upstream gradient); the clamp passes
the gradient on the closed interval and masks a NaN output. x = q / div overflows to +-inf where float32 does, so that the
non-finite rows of the float64 evaluation are those of a float32 one.

Tolerances (EPS = 2^-23 = two units of round-to-nearest per counted rounding), carried layer by layer to first order:

    tol_x0 = EPS |q / div| + q_tol / |div|                                        (the division; the SGA sample's own bound)
    tol_z  = (fan_in + 2) EPS (sum|x||W| + |b|) + sum|W| tol_x   [+ EPS |z| for sine: the product 30 z]
    tol_y  = L tol_z + c_act EPS |y|        L = max|act'| over [z - tol_z, z + tol_z] (relu: 0 where all of it is < 0)
    tol_d  = what tol_y / tol_z do to the derivative the kernel forms from its own y (or z), + its roundings

and backwards, with G the gradient at a layer's output, ``a`` its absolute chain and ``t`` its tolerance:

    gz = G d          a_z = a |d|            t_z = t |d| + a tol_d + EPS a_z
    gx = gz W^T       a_x = a_z |W|^T        t_x = t_z |W|^T + (fan_out + 1) EPS a_x
    gW = sum_r x gz   abs = sum_r |x| a_z    carried = sum_r (tol_x a_z + |x| t_z)        (gb: x = 1, tol_x = 0)
    grad_latent = gx / div * dq    abs = a_x / |div| |dq|    tol = t_x / |div| |dq| + a_x / |div| dq_tol + 2 EPS abs

``abs`` uses the chain scales, not |gz|: gz is a signed sum whose fp32 error is proportional to its terms (tests/mlp_ref.py).
"""
import numpy as np

import latent_multi_ref as mr

EPS = float(np.finfo(np.float32).eps)
FLT_MAX = float(np.finfo(np.float32).max)
ACTS = ("none", "sigmoid", "tanh", "relu", "sine")
RELU_MARGIN = 32.0          # safe_rows: |z| > 32 tol_z at every hidden or final relu
CLAMP_MARGIN = 1.0          # off_the_clamp_edge: ||y| - c| > tol_y: a kernel within tol_y of y is on the same side of c
MAX_REJECTED = 0.05         # neither filter may take more than this share of a batch

# roundings of the kernel's activation expression, relative to |y| (libm calls: documented <= 2 ulp each)
C_ACT = {"none": 0,         # y = z
         "relu": 0,         # a select
         "sigmoid": 4,      # 1 / (1 + expf(-z)): expf 2 (its relative error reaches y scaled by e / (1 + e) <= 1), add 1, divide 1
         "tanh": 2,         # tanhf 2
         "sine": 2}         # sinf 2 (the product 30 z is in tol_z)


def num_params(widths):
    return sum(a * b + b for a, b in zip(widths[:-1], widths[1:]))


def unpack(params, widths):
    """packed vector -> [(W [in, out], b [out])] float64."""
    params = np.asarray(params, np.float64)
    assert params.shape == (num_params(widths),), (params.shape, widths)
    layers, off = [], 0
    for a, b in zip(widths[:-1], widths[1:]):
        layers.append((params[off:off + a * b].reshape(a, b), params[off + a * b:off + a * b + b]))
        off += a * b + b
    return layers


def pack(layers):
    return np.concatenate([np.concatenate([np.asarray(W).reshape(-1), np.asarray(b).reshape(-1)]) for W, b in layers])


def activate(act, z):
    """-> (y, d = act'(z)) float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        if act == "sigmoid":
            y = 1.0 / (1.0 + np.exp(-z))
            return y, y * (1.0 - y)
        if act == "tanh":
            y = np.tanh(z)
            return y, 1.0 - y * y
        if act == "relu":
            y = np.where(z <= 0, 0.0, z)                   # a NaN compares false and stays
            return y, np.where(y <= 0, 0.0, 1.0)
        if act == "sine":
            return np.sin(30.0 * z), 30.0 * np.cos(30.0 * z)
    return z, np.ones_like(z)


def _lipschitz(act, z, tol_z):
    """max |act'| over [z - tol_z, z + tol_z]."""
    if act == "sine":
        return np.full_like(z, 30.0)
    if act == "none":
        return np.ones_like(z)
    if act == "relu":                                        # 0 where the whole interval is off: that unit is an exact 0
        return np.where(z + tol_z < 0, 0.0, 1.0)
    lo, hi = z - tol_z, z + tol_z
    near = np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(np.abs(lo), np.abs(hi)))     # the point of the interval nearest 0
    return activate(act, near)[1]                            # sigmoid' and tanh' fall with |z|: <= 1/4 and <= 1


def _derivative_tol(act, y, d, tol_z, tol_y):
    """Tolerance of the derivative the kernel forms: d = y (1 - y), 1 - y y, 30 cosf(30 z)."""
    if act == "sigmoid":                                     # |dd/dy| = |1 - 2y|; the subtraction and the product: 2
        return np.abs(1.0 - 2.0 * y) * tol_y + 2.0 * EPS * np.abs(d)
    if act == "tanh":                                        # |dd/dy| = 2|y|; the product y y (<= 1) and the subtraction
        return 2.0 * np.abs(y) * tol_y + EPS * (y * y + np.abs(d))
    if act == "sine":                                        # |dd/dz| <= 900; cosf 2, the product with 30 1
        return 900.0 * tol_z + 3.0 * EPS * np.abs(d)
    return np.zeros_like(y)                                  # none: 1; relu: a gate the row filter keeps on its side


def _quantised(latent, uniforms, T, diff, div):
    d = np.asarray(div, np.float64).reshape(1, -1)
    with np.errstate(over="ignore", invalid="ignore"):
        q, dq = mr.quantise(latent, uniforms, T, diff)
        if uniforms is None:
            q_tol, dq_tol = np.zeros(q.shape), np.zeros(q.shape)
        else:
            q_tol, dq_tol = mr.sga_tolerances(latent, uniforms, T, diff)
        x = q / d
        x = np.where(np.abs(x) > FLT_MAX, np.sign(x) * np.inf, x)                   # float32 overflows there
        tol_x = EPS * np.abs(x) + q_tol / np.abs(d)
    return x, tol_x, dq, dq_tol, d


def forward(latent, uniforms, T, diff, div, params, widths, act, final_act, clampw):
    """-> dict(out, y (before the clamp), tol_y, xs (every layer's input), zs (pre-activations), tol_xs, tol_zs, ds, tol_ds)."""
    layers = unpack(params, widths)
    x, tol_x, dq, dq_tol, d = _quantised(latent, uniforms, T, diff, div)
    xs, zs, tol_xs, tol_zs, ds, tol_ds, acts = [], [], [], [], [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (W, b) in enumerate(layers):
            a = act if k + 1 < len(layers) else final_act
            z = x @ W + b
            tol_z = (W.shape[0] + 2) * EPS * (np.abs(x) @ np.abs(W) + np.abs(b)) + tol_x @ np.abs(W)
            if a == "sine":
                tol_z = tol_z + EPS * np.abs(z)
            y, dv = activate(a, z)
            tol_y = _lipschitz(a, z, tol_z) * tol_z + C_ACT[a] * EPS * np.abs(y)
            xs.append(x), zs.append(z), tol_xs.append(tol_x), tol_zs.append(tol_z), ds.append(dv), acts.append(a)
            tol_ds.append(_derivative_tol(a, y, dv, tol_z, tol_y))
            x, tol_x = y, tol_y
    out = np.where(x < -clampw, -clampw, np.where(x > clampw, clampw, x)) if clampw > 0 else x   # a NaN stays
    return dict(out=out, y=x, tol_y=tol_x, xs=xs, zs=zs, tol_xs=tol_xs, tol_zs=tol_zs, ds=ds, tol_ds=tol_ds, acts=acts, dq=dq,
                dq_tol=dq_tol, div=d)


def backward(latent, uniforms, T, diff, div, params, widths, act, final_act, clampw, grad_out):
    """-> dict(grad_latent, grad_latent_abs, grad_latent_tol, grad_params, grad_params_abs, grad_params_tol, fw, and
    grad_x_abs = a_x / |div|: the scale of the gradient at q, before dq)."""
    layers = unpack(params, widths)
    fw = forward(latent, uniforms, T, diff, div, params, widths, act, final_act, clampw)
    g = np.asarray(grad_out, np.float64).copy()
    if clampw > 0:
        g = np.where((fw["y"] >= -clampw) & (fw["y"] <= clampw), g, 0.0)            # closed interval; a NaN output is masked
    ga, gt = np.abs(g), np.zeros_like(g)
    gp, gp_abs, gp_tol = [None] * len(layers), [None] * len(layers), [None] * len(layers)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(len(layers) - 1, -1, -1):
            W, _ = layers[k]
            x, tol_x, dv, tol_d = fw["xs"][k], fw["tol_xs"][k], fw["ds"][k], fw["tol_ds"][k]
            if fw["acts"][k] == "relu":
                off = dv == 0                                                       # select on h <= 0
                gz, az, tz = np.where(off, 0.0, g), np.where(off, 0.0, ga), np.where(off, 0.0, gt)
            else:
                gz, az = g * dv, ga * np.abs(dv)
                tz = gt * np.abs(dv) + ga * tol_d + EPS * az
            gp[k] = (x.T @ gz, gz.sum(0))
            gp_abs[k] = (np.abs(x).T @ az, az.sum(0))
            gp_tol[k] = (tol_x.T @ az + np.abs(x).T @ tz, tz.sum(0))
            g = gz @ W.T
            ga = az @ np.abs(W).T
            gt = tz @ np.abs(W).T + (W.shape[1] + 1) * EPS * ga
        d, dq = fw["div"], fw["dq"]
        gl = g / d * dq
        gl_abs = ga / np.abs(d) * np.abs(dq)
        gl_tol = gt / np.abs(d) * np.abs(dq) + ga / np.abs(d) * fw["dq_tol"] + 2.0 * EPS * gl_abs
    return dict(grad_latent=gl, grad_latent_abs=gl_abs, grad_latent_tol=gl_tol, grad_x_abs=ga / np.abs(d), grad_params=pack(gp),
                grad_params_abs=pack(gp_abs), grad_params_tol=pack(gp_tol), fw=fw)


def sga_f32(latent, uniforms, T, diff):
    """The SGA sample and its derivative evaluated in numpy float32, operation by operation, in the PRODUCT form the kernels
    use (dq = s0 s1 (...) / T^2, no difference of near-equal numbers) -> (q, dq) float32."""
    f = np.float32
    w, T = latent.astype(f), f(T)
    lim, eps = f(1.0 - 1e-6), f(np.finfo(f).eps)
    wf = np.floor(w)
    wc = wf + f(1)
    a, b = w - wf, wc - w
    tf_, tc = np.tanh(np.clip(a, -lim, lim)), np.tanh(np.clip(b, -lim, lim))
    u = np.clip(uniforms.astype(f), eps, f(1) - eps)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        g = -np.log(-np.log(u))
        z0, z1 = (-tf_ / T + g[..., 0]) / T, (-tc / T + g[..., 1]) / T
        m = np.maximum(z0, z1)
        lse = m + np.log(np.exp(z0 - m) + np.exp(z1 - m))
        s0, s1 = np.exp(z0 - lse), np.exp(z1 - lse)
        q = wf * s0 + wc * s1
        if diff:
            in_f, in_c = ((a >= -lim) & (a <= lim)).astype(f), ((b >= -lim) & (b <= lim)).astype(f)
            dq = s0 * s1 * ((f(1) - tc * tc) * in_c + (f(1) - tf_ * tf_) * in_f) / (T * T)
        else:
            dq = s0 + s1
    assert q.dtype == f and dq.dtype == f
    return q, dq


def forward_f32(latent, div, params, widths, act, final_act, uniforms=None, T=1.0, diff=False):
    """The forward (before the clamp) evaluated in numpy float32, product by product (the SGA sample by sga_f32): how much of
    tol_y a plain fp32 evaluation uses. Printed by the GPU tests beside the kernel's own figure."""
    f = np.float32
    q = np.rint(latent.astype(f)) if uniforms is None else sga_f32(latent, uniforms, T, diff)[0]
    x = (q / np.asarray(div, f).reshape(1, -1)).astype(f)
    layers = unpack(params, widths)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (W, b) in enumerate(layers):
            W, b = W.astype(f), b.astype(f)
            z = np.broadcast_to(b, (x.shape[0], b.size)).copy()
            for i in range(W.shape[0]):
                z = (z + (x[:, i:i + 1] * W[i:i + 1]).astype(f)).astype(f)
            a = act if k + 1 < len(layers) else final_act
            if a == "sigmoid":
                x = (f(1) / (f(1) + np.exp(-z))).astype(f)
            elif a == "tanh":
                x = np.tanh(z)
            elif a == "relu":
                x = np.where(z <= 0, f(0), z)
            elif a == "sine":
                x = np.sin((f(30) * z).astype(f))
            else:
                x = z
    return x.astype(np.float64)


def safe_rows(fw):
    """Rows none of whose relu pre-activations lies within RELU_MARGIN tol_z of 0 (an exact 0 from all-zero operands, whose
    tol_z is 0, is safe: fp32 computes that 0 too; an infinite or NaN pre-activation is not near the gate either: those rows
    stay in the batch with their grad_out and are held to float32 torch's policy). Looks at the reference only."""
    ok = np.ones(fw["y"].shape[0], bool)
    for a, z, tz in zip(fw["acts"], fw["zs"], fw["tol_zs"]):
        if a == "relu":
            with np.errstate(invalid="ignore"):
                near = (np.abs(z) <= RELU_MARGIN * tz) & (tz > 0) & np.isfinite(z)
            ok &= ~near.any(1)
    return ok


def off_the_clamp_edge(fw, clampw):
    """Rows none of whose outputs lies within CLAMP_MARGIN tol_y of +-clampw; an output that equals the bound is exempt only
    with a zero tolerance. (A test whose outputs equal the bound by construction proves that exactness itself and does not
    draw its rows through this filter.) Looks at the reference only."""
    if clampw <= 0:
        return np.ones(fw["y"].shape[0], bool)
    with np.errstate(invalid="ignore"):
        dist = np.abs(np.abs(fw["y"]) - clampw)
        near = (dist <= CLAMP_MARGIN * fw["tol_y"]) & (fw["tol_y"] > 0) & np.isfinite(fw["y"])   # +-inf is beyond, not near
    return ~near.any(1)


TIES = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1e-9, -1e-9], np.float32)   # rint: 0, -0, 2, -2, 2, -2, 0, -0


def make_inputs(seed, rows, widths, sga=False, w_std=0.5):
    """Random inputs every test of the hidden-layer decoder draws through: latents in [-6, 6] (the first eight rows' column 0
    holds TIES when there are 16 rows or more), div in [0.5, 3], non-zero biases, uniforms when ``sga``."""
    rng = np.random.default_rng(seed)
    ld = widths[0]
    p = dict(latent=rng.uniform(-6, 6, (rows, ld)).astype(np.float32), div=rng.uniform(0.5, 3, ld).astype(np.float32),
             uniforms=rng.random((rows, ld, 2), dtype=np.float32) if sga else None,
             grad_out=rng.standard_normal((rows, widths[-1])).astype(np.float32), widths=tuple(widths), clampw=0.0)
    if rows >= 16:                                           # round-half ties and the two sides of zero
        p["latent"][:8, 0] = TIES
    layers = [((rng.standard_normal((a, b)) * w_std / np.sqrt(a)).astype(np.float32),
               (rng.standard_normal(b) * 0.1 + 0.05).astype(np.float32)) for a, b in zip(widths[:-1], widths[1:])]
    p["params"] = pack(layers).astype(np.float32)
    return p


def clamp_at_quantile(p, T, diff, act, final_act, quantile=0.67):
    """clamp_weights near that quantile of the float64 |y| over the batch's finite rows -- in the middle of the widest gap
    between attained values within 0.05 of it: about a third of the outputs exceed it."""
    ok = (np.abs(p["latent"]) < 1e30).all(1)
    uni = None if p["uniforms"] is None else p["uniforms"][ok]
    y = forward(p["latent"][ok], uni, T, diff, p["div"], p["params"], p["widths"], act, final_act, 0.0)["y"]
    v = np.sort(np.abs(y).reshape(-1))
    lo, hi = int((quantile - 0.05) * v.size), max(int((quantile + 0.05) * v.size), int((quantile - 0.05) * v.size) + 2)
    w = v[lo:min(hi, v.size)]
    if w.size < 2:
        return float(np.float32(v[min(lo, v.size - 1)] * 1.5))
    i = int(np.argmax(np.diff(w)))                           # the widest gap there: a one-column latent attains few values
    return float(np.float32(0.5 * (w[i] + w[i + 1])))


POLICY_LATENTS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "overflow": 3e38, "-overflow": -3e38}


def policy_batch(seed, rows, widths, bad_rows, names=None):
    """A random batch with div[0] = 0.5 in which ``bad_rows`` carry, in column 0, the POLICY_LATENTS ``names`` in turn
    (3e38 / 0.5 overflows float32). -> (inputs, {row: name})."""
    p = make_inputs(seed, rows, widths)
    p["div"][0] = 0.5
    names = list(names or POLICY_LATENTS)
    where = {}
    for n, r in enumerate(bad_rows):
        p["latent"][r, 0] = POLICY_LATENTS[names[n % len(names)]]
        where[int(r)] = names[n % len(names)]
    return p, where


def torch_eval(latent, uniforms, T, diff, div, params, widths, act, final_act, clampw, grad_out, dtype):
    """The module's own path with torch ops on the CPU in ``dtype`` (LatentDecoder('sq') with these layers; autograd):
    -> (out, grad_latent, grad_params packed). float64: a second float64 statement; float32: the NaN / inf POLICY."""
    import torch
    from shacira_amd.wisp.models.latent_decoders import LatentDecoder
    hidden = tuple(widths[1:-1])
    dec = LatentDecoder(widths[0], widths[-1], "none", "sq", True, num_layers_dec=len(hidden), hidden_dim_dec=hidden or 0,
                        activation=act, final_activation=final_act, clamp_weights=float(clampw), use_sga=uniforms is not None,
                        diff_sampling=bool(diff)).to(dtype)
    dec.temperature = float(T)
    mods = dec._decoder_layers()
    with torch.no_grad():
        dec.div.copy_(torch.from_numpy(np.asarray(div)).to(dtype))
        for m, (W, b) in zip(mods, unpack(params, widths)):
            m.scale.copy_(torch.from_numpy(W).to(dtype))
            m.shift.copy_(torch.from_numpy(b).to(dtype).reshape(m.shift.shape))
    lat = torch.from_numpy(np.ascontiguousarray(latent)).to(dtype).requires_grad_(True)
    if uniforms is not None:
        uni, rand = torch.from_numpy(np.ascontiguousarray(uniforms)).to(dtype), torch.rand
        torch.rand = lambda *a, **k: uni.clone()             # the sampler draws ONE torch.rand([rows, ld, 2])
        try:
            y = dec(lat)
        finally:
            torch.rand = rand
    else:
        y = dec(lat)
    y.backward(torch.from_numpy(np.ascontiguousarray(grad_out)).to(dtype))
    gp = np.concatenate([np.concatenate([m.scale.grad.numpy().reshape(-1), m.shift.grad.numpy().reshape(-1)]) for m in mods])
    return y.detach().numpy(), lat.grad.numpy(), gp


def nonfinite_class(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf: what the policy tests compare."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))
