"""The decoder MLP (mlp.hip, mlp_mfma.hip) in numpy float64 with explicit matmuls and explicit backward formulas, the scales
the GPU tests state their bars in, and the row filter every tolerance test draws its rows through. TEST INFRASTRUCTURE ONLY.

Parameters are the C-ABI's flat block: W1 [H, IN] row-major, b1 [H], W2 [H, H], b2 [H], ..., Wout [OUT, H], bout [OUT];
`dims` = (IN, H, NH, OUT).

The ReLU rule (what torch.relu and its backward do, in float64 and in float32, checked in test_mlp_ref_cpu.py):
    forward    h  = z where z > 0, 0 where z <= 0, NaN where z is NaN
    backward   dz = 0 where h <= 0, the upstream gradient (whatever it is, NaN and inf included) everywhere else
so a NaN activation stays a NaN and lets its gradient THROUGH, and a unit that is off gives an exact 0 even under a NaN or
infinite upstream gradient (a select, not a product with a 0/1 mask).

Scales (all >= the magnitude of what they scale, and what fp32 rounding errors are proportional to):
    y_scale   [n, OUT]  the forward pass run with |W|, |b|, |x| (no gate needed: nothing is negative)
    gx_scale  [n, IN]   the backward chain run with |W|, |grad_y| and the reference's own gates
    gp_scale  [P]       per weight sum_s sdz_s ain_s, per bias sum_s sdz_s, where sdz is the backward chain on absolute values
                        (gx_scale's construction, stopped at that layer) and ain the forward chain on absolute values
                        (y_scale's construction, stopped at that layer's input), both with the reference's gates

gp_scale uses the chain scales, not the products sum_s |dz_s| |in_s| of the reference's own values: dz_s is a sum of up to 128
signed products, so where it cancels to a thousandth of its terms its fp32 rounding error is a thousand times its own size. At
one row grad_params is the single product dz . in, and CPU torch fp32 then misses the reference by up to 1.5e-4 of |dz| |in|
(43 -> 128 -> 128 -> 3, n = 31): no fp32 evaluation meets a bar in those units at small n. The chain scales are what the rounding
error of a product of two rounded factors is proportional to, and what y_scale and gx_scale are built from. They are about ten
times the products; the allowance in them is the 2^-21 floor (torch's own worst miss: 2.2e-8 at 70_001 rows, 2.0e-7 at the
small sizes). The error in units of the products is still computed and printed by the GPU tests (products_error).

safe_rows: a row is safe if every hidden pre-activation z of the float64 evaluation has |z| > 2^-12 (sum_i |w_i| |in_i| + |b|).
An fp32 dot product of fan-in K <= 128 in any order is within (K + 1) 2^-24 <= 2^-17 of that sum, so a safe row's
pre-activation is 32 bounds away from the other ReLU branch and an fp32 kernel gates it as the reference does. The filter
looks at the inputs and the reference only: no test drops a row after seeing a kernel's output.

Share of randn rows the filter rejects: REJECTION below.
"""
import numpy as np

# every instantiation: (dims, mlp_variant). -1 = the MFMA kernels (16x16x4 for width 16, 32x32x2 for width 64, the split
# kernel for width 128), 0 = the VALU kernels of mlp.hip. (32, 16, 3, 3) has no MFMA kernel: it runs VALU under either value.
MFMA_SHAPES = [(32, 64, 1, 16), (43, 64, 2, 3), (32, 64, 2, 3), (16, 64, 2, 3), (32, 64, 1, 3), (96, 128, 1, 16),
               (43, 128, 2, 3), (32, 16, 2, 3), (24, 16, 2, 3), (16, 16, 2, 3), (48, 16, 2, 3), (32, 16, 1, 3), (32, 16, 2, 4)]
VALU_SHAPES = [(32, 16, 2, 3), (24, 16, 2, 3), (16, 16, 2, 3), (48, 16, 2, 3), (32, 16, 1, 3), (32, 16, 3, 3), (32, 16, 2, 4)]
SHAPES = [(d, -1) for d in MFMA_SHAPES] + [(d, 0) for d in VALU_SHAPES]

SAFE_MARGIN = 2.0 ** -12
ALLOWANCE_FLOOR = 2.0 ** -21


def num_params(dims):
    IN, H, NH, OUT = dims
    return sum((IN if l == 0 else H) * H + H for l in range(NH)) + OUT * H + OUT


def unpack(params, dims):
    """flat block -> [(W [fan_out, fan_in], b [fan_out])] for the NH hidden layers and the output layer (views)."""
    IN, H, NH, OUT = dims
    params = np.asarray(params)
    assert params.shape == (num_params(dims),)
    layers, off = [], 0
    for l in range(NH + 1):
        fi, fo = (IN if l == 0 else H), (OUT if l == NH else H)
        layers.append((params[off:off + fi * fo].reshape(fo, fi), params[off + fi * fo:off + fi * fo + fo]))
        off += fi * fo + fo
    return layers


def pack(layers):
    return np.concatenate([np.concatenate([np.asarray(W).reshape(-1), np.asarray(b).reshape(-1)]) for W, b in layers])


def relu(z):
    return np.where(np.isnan(z), z, np.where(z > 0, z, 0.0))


def relu_backward(h, g):
    return np.where(h <= 0, 0.0, g)


def _hidden(x, layers):
    """inputs of every layer [x, h_0, ..., h_{NH-1}] and the hidden pre-activations [z_0, ...]"""
    ins, zs = [x], []
    for W, b in layers[:-1]:
        zs.append(ins[-1] @ W.T + b)
        ins.append(relu(zs[-1]))
    return ins, zs


def forward_scaled(x, params, dims):
    """forward only -> dict(y, y_scale) in float64"""
    layers = unpack(np.asarray(params, np.float64), dims)
    ins, _ = _hidden(np.asarray(x, np.float64), layers)
    a = np.abs(ins[0])
    for W, b in layers:
        a = a @ np.abs(W).T + np.abs(b)
    return dict(y=ins[-1] @ layers[-1][0].T + layers[-1][1], y_scale=a)


def forward_backward(x, params, grad_y, dims, dtype=np.float64, sizes=None):
    """-> dict(y, gx, gp, y_scale, gx_scale, gp_scale). `dtype` float32 restates the same formulas in fp32 (the exactness check
    of the integer case); the scales are always float64. With `sizes` (ascending row counts <= n), gp and gp_scale are dicts
    {size: value over the first `size` rows}; y, gx and their scales are per row, so a prefix of them is the prefix's answer."""
    with np.errstate(invalid="ignore", over="ignore"):
        x, gy = np.asarray(x, dtype), np.asarray(grad_y, dtype)
        n = x.shape[0]
        layers = unpack(np.asarray(params, dtype), dims)
        NH = len(layers) - 1
        ins, _ = _hidden(x, layers)
        y = ins[-1] @ layers[-1][0].T + layers[-1][1]
        # the forward chain on absolute values, with the reference's gates: what the fp32 error of every layer's input scales with
        ains = [np.abs(x).astype(np.float64)]
        for l, (W, b) in enumerate(layers):
            a = ains[-1] @ np.abs(W).T.astype(np.float64) + np.abs(b)
            ains.append(np.where(ins[l + 1] <= 0, 0.0, a) if l < NH else a)
        a = np.abs(x).astype(np.float64)
        for W, b in layers:
            a = a @ np.abs(W).T.astype(np.float64) + np.abs(b)
        y_scale = a
        # backward: dz of the output layer is grad_y; dz_l = relu'(h_l) . (W_{l+1}^T dz_{l+1})
        dz, sdz = gy, np.abs(gy).astype(np.float64)
        dzs, sdzs = [None] * (NH + 1), [None] * (NH + 1)
        for l in range(NH, -1, -1):
            dzs[l], sdzs[l] = dz, sdz
            W, _ = layers[l]
            dz, sdz = dz @ W, sdz @ np.abs(W).astype(np.float64)
            if l > 0:
                dz, sdz = relu_backward(ins[l], dz), relu_backward(ins[l], sdz)

        def gp_of(lo, hi):
            g, sc, pr = [], [], []
            for l in range(NH + 1):
                d, i = dzs[l][lo:hi], ins[l][lo:hi]
                g.append((d.T @ i, d.sum(axis=0)))
                sc.append((sdzs[l][lo:hi].T @ ains[l][lo:hi], sdzs[l][lo:hi].sum(axis=0)))
                d, i = np.abs(d).astype(np.float64), np.abs(i).astype(np.float64)
                pr.append((d.T @ i, d.sum(axis=0)))
            return pack(g), pack(sc), pack(pr)

        out = dict(y=y, gx=dz, y_scale=y_scale, gx_scale=sdz)
        if sizes is None:
            out["gp"], out["gp_scale"], out["gp_products"] = gp_of(0, n)
            return out
        out["gp"], out["gp_scale"], out["gp_products"] = {}, {}, {}
        lo, g, sc, pr = 0, 0.0, 0.0, 0.0
        for size in sizes:
            assert lo <= size <= n
            dg, dsc, dpr = gp_of(lo, size)
            g, sc, pr, lo = g + dg, sc + dsc, pr + dpr, size
            out["gp"][size], out["gp_scale"][size], out["gp_products"][size] = g, sc, pr
        return out


def prefix(ref, size):
    """the reference of the first `size` rows, from a forward_backward(..., sizes=[.., size, ..]) result"""
    return dict(y=ref["y"][:size], gx=ref["gx"][:size], y_scale=ref["y_scale"][:size], gx_scale=ref["gx_scale"][:size],
                gp=ref["gp"][size], gp_scale=ref["gp_scale"][size], gp_products=ref["gp_products"][size])


def products_error(got, ref):
    """worst |gp - ref| in units of sum_s |dz_s| |in_s| (the products of the reference's own values): reported, not a bar --
    see the module docstring"""
    err, s = np.abs(np.asarray(got["gp"], np.float64) - ref["gp"]), ref["gp_products"]
    ok = np.isfinite(err) & (s > 0)
    return float((err[ok] / s[ok]).max()) if ok.any() else 0.0


def violations(got, ref, allowance, keys=("y", "gx", "gp")):
    """The bar. Where the reference is finite: |got - ref| <= allowance * scale, elementwise. Where it is not: NaN exactly where
    the reference has NaN, +inf / -inf exactly where it has them. -> list of (key, elements outside, worst error in scale
    units); empty = passes. `allowance` = (y, gx, gp)."""
    bad = []
    for key, allow in zip(("y", "gx", "gp"), allowance):
        if key not in keys or got.get(key) is None or key not in ref:
            continue
        g, r, s = np.asarray(got[key], np.float64), ref[key], ref[key + "_scale"]
        assert g.shape == r.shape, (key, g.shape, r.shape)
        fin = np.isfinite(r)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(g - r)
            out = np.where(fin, ~(err <= allow * s), (np.isnan(r) != np.isnan(g)) | (~np.isnan(r) & (g != r)))
            units = np.where(fin & (s > 0), err / np.where(s > 0, s, 1.0), 0.0)
        if out.any():
            bad.append((key, int(out.sum()), float(np.nanmax(units)) if units.size else 0.0))
    return bad


def safe_rows(x, params, dims):
    """bool [n]: rows none of whose hidden pre-activations is within SAFE_MARGIN of the other ReLU branch (module docstring)."""
    layers = unpack(np.asarray(params, np.float64), dims)
    ins, zs = _hidden(np.asarray(x, np.float64), layers)
    ok = np.ones(ins[0].shape[0], bool)
    for (W, b), inp, z in zip(layers[:-1], ins, zs):
        ok &= (np.abs(z) > SAFE_MARGIN * (np.abs(inp) @ np.abs(W).T + np.abs(b))).all(axis=1)
    return ok


def draw_safe_rows(draw, n, params, dims, max_rounds=64):
    """n safe rows of the family `draw(count) -> x [count, IN] float32`: draws, filters, and draws more until it has n.
    -> (x [n, IN] float32, rows drawn in all)."""
    kept, have, drawn = [], 0, 0
    for _ in range(max_rounds):
        if have >= n:
            break
        count = max(64, int(1.25 * (n - have)) + 16)
        x = np.ascontiguousarray(draw(count), np.float32)
        x = x[safe_rows(x, params, dims)]
        kept.append(x)
        have += x.shape[0]
        drawn += count
    assert have >= n, "the family yields too few safe rows: change the family, not the margin"
    return np.ascontiguousarray(np.concatenate(kept)[:n]), drawn


# --------------------------------------------------------------------------------------------------------------- families
def default_params(dims, seed, gain=1.0):
    """nn.Linear's default initialisation (kaiming_uniform(a = sqrt 5): weights and biases U(-1/sqrt(fan_in), 1/sqrt(fan_in)))
    times `gain`, as the flat fp32 block. test_mlp.py's parameters are gain 3 (width 16) and 1.5 (wider)."""
    IN, H, NH, OUT = dims
    rng = np.random.default_rng(seed)
    layers = []
    for l in range(NH + 1):
        fi, fo = (IN if l == 0 else H), (OUT if l == NH else H)
        k = 1.0 / np.sqrt(fi)
        layers.append((rng.uniform(-k, k, (fo, fi)) * gain, rng.uniform(-k, k, fo) * gain))
    return pack(layers).astype(np.float32)


def scaled_gain(dims):
    return 3.0 if dims[1] < 64 else 1.5


def randn_rows(seed, in_dim, scale=1.0, same_sign=False):
    rng = np.random.default_rng(seed)
    if same_sign:
        return lambda count: (np.abs(rng.standard_normal((count, in_dim))) * scale).astype(np.float32)
    return lambda count: (rng.standard_normal((count, in_dim)) * scale).astype(np.float32)


def exact_case(dims, n):
    """Integers all the way: small weights and biases that differ from their neighbours (so a swapped or shifted index shows),
    one-hot x rows with an integer amplitude (feature s mod IN: every feature, every k block of the MFMA kernels and their zero
    padding), one-hot grad_y rows. Every scale stays below 2^24 (asserted in test_mlp_ref_cpu.py), so every product and every
    partial sum in ANY order is an integer fp32 holds exactly. -> (x, params, grad_y) float32."""
    IN, H, NH, OUT = dims
    R = 7 if H <= 64 else 3                                        # weights in [-R, R]: 2R + 1 consecutive ones are distinct
    layers = []
    for l in range(NH + 1):
        fi, fo = (IN if l == 0 else H), (OUT if l == NH else H)
        j, i = np.meshgrid(np.arange(fo), np.arange(fi), indexing="ij")
        W = (5 * j + 3 * i + 2 * l + (j * i) % 3) % (2 * R + 1) - R
        layers.append((W, (3 * np.arange(fo) + l) % 9 - 4))
    s = np.arange(n)
    x = np.zeros((n, IN), np.float32)
    x[s, s % IN] = (1 + s % 4) * np.where(s % 3 == 0, -1, 1)
    gy = np.zeros((n, OUT), np.float32)
    gy[s, (s // 2) % OUT] = (1 + s % 3) * np.where(s % 5 < 2, -1, 1)
    return x, pack(layers).astype(np.float32), gy


# -------------------------------------------------------------------------------------------------------------- allowance
def errors_in_scale(got, ref):
    """worst |got - ref| / scale of y, gx, gp (0 where the scale is 0 and the values agree; inf where they do not)."""
    out = []
    for k in ("y", "gx", "gp"):
        if k not in ref or got.get(k) is None:
            out.append(0.0)
            continue
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        s = ref[k + "_scale"]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where(err > 0, np.inf, 0.0))
        out.append(float(r.max()) if r.size else 0.0)
    return tuple(out)


def torch_fp32(x, params, grad_y, dims):
    """CPU torch fp32 nn.Linear layers + autograd on the same inputs: the yardstick of the allowance."""
    import torch
    layers = [(torch.tensor(np.array(W), requires_grad=True), torch.tensor(np.array(b), requires_grad=True))
              for W, b in unpack(np.asarray(params, np.float32), dims)]
    xt = torch.tensor(np.asarray(x, np.float32), requires_grad=True)
    h = xt
    for W, b in layers[:-1]:
        h = torch.relu(torch.nn.functional.linear(h, W, b))
    y = torch.nn.functional.linear(h, *layers[-1])
    y.backward(torch.tensor(np.asarray(grad_y, np.float32)))
    return dict(y=y.detach().numpy(), gx=xt.grad.numpy(), gp=pack([(W.grad.numpy(), b.grad.numpy()) for W, b in layers]))


ALLOWANCE_ROWS = 70_001


def allowance_inputs(dims, n=ALLOWANCE_ROWS):
    """the inputs the allowance is measured on: default-initialised parameters, n filtered randn rows, randn grad_y"""
    seed = 1000 * dims[0] + 100 * dims[2] + dims[1] + dims[3]
    params = default_params(dims, seed)
    x, _ = draw_safe_rows(randn_rows(seed + 1, dims[0]), n, params, dims)
    gy = np.random.default_rng(seed + 2).standard_normal((n, dims[3])).astype(np.float32)
    return x, params, gy


def measure_torch():
    """worst error of CPU torch fp32 in units of (y_scale, gx_scale, gp_scale), over all shapes"""
    import torch
    worst, threads = np.zeros(3), torch.get_num_threads()
    torch.set_num_threads(1)                     # one thread: the fp32 GEMMs' summation order does not depend on the host's core count
    try:
        for dims in sorted(set(MFMA_SHAPES + VALU_SHAPES)):
            x, params, gy = allowance_inputs(dims)
            ref = forward_backward(x, params, gy, dims)
            worst = np.maximum(worst, errors_in_scale(torch_fp32(x, params, gy, dims), ref))
    finally:
        torch.set_num_threads(threads)
    return tuple(float(w) for w in worst)


def allowance(measured=None):
    """(y, gx, gp) allowances: four times what CPU torch fp32 misses the reference by (the factor covers another contraction
    and operation order: the convention of adam_ref), never below 2^-21."""
    measured = measure_torch() if measured is None else measured
    return tuple(max(4.0 * m, ALLOWANCE_FLOOR) for m in measured)


# Measured by test_mlp_ref_cpu.py::test_allowance_constants, which asserts them: the worst error of CPU torch fp32 nn.Linear
# layers (one thread) in units of (y_scale, gx_scale, gp_scale) over all 14 shapes at 70_001 filtered randn rows, and the bars: four times
# that, floor 2^-21 (the floor holds for y and for grad_params, whose misses average out over 70_001 rows).
# The kernels on the MI355X reach y 1.6e-7, grad_x 2.7e-7, grad_params 2.2e-7 (MFMA) and 4.2e-7 (VALU, at feature scale 1e-4:
# 1.15 times inside the bar; see test_gpu_mlp_edges.py's docstring before reading a miss there as a new fault).
TORCH_MEASURED = (5.2060328630964275e-08, 1.990555963721828e-07, 2.1821706326327083e-08)
ALLOWANCE = (4.76837158203125e-07, 7.962223854887312e-07, 4.76837158203125e-07)

# Share of randn rows the filter rejects, 20_000 rows, {dims: {(parameter gain, feature scale): share}}; asserted to 0.01 by
# test_mlp_ref_cpu.py::test_filter_rejection_share. A row is rejected when ANY hidden unit is within the margin, so the share
# grows with the number of hidden units: 2 % at width 16, 10 % at width 64 with two layers, 16 % to 23 % at width 128. At
# feature scale 1e-4 the biases decide every gate and no row is rejected. The shares at widths 64 and 128 are above the 10 %
# the filter was meant to stay under; the family and the margin are both kept (a pre-activation's ratio to its absolute sum
# has density ~2.5 at zero for any zero-mean family, so the share follows the unit count). The filter reads the inputs and the
# float64 evaluation only: what it keeps is not chosen by any kernel.
REJECTION = {
    (32, 16, 2, 3): {(1.0, 1.0): 0.0182, (3.0, 1.0): 0.0194, (1.0, 1e3): 0.0170},
    (32, 16, 3, 3): {(1.0, 1.0): 0.0201},
    (43, 64, 2, 3): {(1.0, 1.0): 0.0997, (1.5, 1.0): 0.1019},
    (96, 128, 1, 16): {(1.0, 1.0): 0.1554},
    (43, 128, 2, 3): {(1.0, 1e-4): 0.0, (1.0, 1.0): 0.2327, (1.5, 1.0): 0.2282, (1.0, 1e3): 0.2180},
}
