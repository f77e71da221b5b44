"""tests/mlp_ref.py checked on the CPU: the float64 reference against torch autograd, its ReLU rule against torch's, the bar of
test_gpu_mlp_edges.py against deliberately wrong copies of the operation (it must reject each), the fp32 restatement of the
workgroup's four-wave flush in arrival order and in fixed order, the integer case's exactness, the measured allowance constants,
the row filter's rejection share, and the set of compiled shapes against the tested list."""
import numpy as np
import pytest
import torch

import mlp_ref as R

ALL_DIMS = sorted(set(R.MFMA_SHAPES + R.VALU_SHAPES))
MUTATION_DIMS = [(32, 16, 2, 3), (43, 64, 2, 3), (43, 128, 2, 3)]            # a narrow, a wide and a width-128 shape


def _inputs(dims, n, seed=0, gain=None):
    params = R.default_params(dims, seed + 11, R.scaled_gain(dims) if gain is None else gain)
    x, _ = R.draw_safe_rows(R.randn_rows(seed + 12, dims[0]), n, params, dims)
    gy = np.random.default_rng(seed + 13).standard_normal((n, dims[3])).astype(np.float32)
    return x, params, gy


@pytest.mark.parametrize("dims", ALL_DIMS)
def test_reference_agrees_with_torch_autograd_in_float64(dims):
    x, params, gy = _inputs(dims, 301)
    ref = R.forward_backward(x, params, gy, dims, sizes=[100, 301])
    lins = []
    for W, b in R.unpack(params, dims):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.array(W, np.float64)))
            lin.bias.copy_(torch.from_numpy(np.array(b, np.float64)))
        lins.append(lin)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    h = xt
    for lin in lins[:-1]:
        h = torch.relu(lin(h))
    y = lins[-1](h)
    y.backward(torch.from_numpy(gy.astype(np.float64)))
    gp = R.pack([(lin.weight.grad.numpy(), lin.bias.grad.numpy()) for lin in lins])
    for name, a, b in (("y", ref["y"], y.detach().numpy()), ("gx", ref["gx"], xt.grad.numpy()), ("gp", ref["gp"][301], gp)):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
    whole = R.forward_backward(x[:100], params, gy[:100], dims)                 # the prefix sums are the prefix's answer
    assert np.abs(whole["gp"] - ref["gp"][100]).max() <= 1e-12 * np.abs(whole["gp"]).max()
    for k in ("y", "gx", "y_scale", "gx_scale"):                                # (to BLAS blocking: 1e-13, not bit for bit)
        assert np.abs(whole[k] - ref[k][:100]).max() <= 1e-13 * np.abs(whole[k]).max(), k
    for k in ("y", "gx"):                                                       # the scales bound what they scale
        assert np.all(np.abs(ref[k]) <= ref[k + "_scale"] * (1 + 1e-12))
    assert np.all(np.abs(ref["gp"][301]) <= ref["gp_scale"][301] * (1 + 1e-12))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_relu_rule_is_torch_relu(dtype):
    z = torch.tensor([1.5, -1.5, 0.0, -0.0, float("nan"), float("inf"), -float("inf")] * 40, dtype=dtype, requires_grad=True)
    g = torch.tensor([2.0, float("nan"), float("inf"), 3.0, -float("inf")] * 56, dtype=dtype)      # every pair (z, g) occurs
    h = torch.relu(z)
    h.backward(g)
    ours_h = R.relu(z.detach().numpy())
    assert np.array_equal(ours_h, h.detach().numpy(), equal_nan=True)
    assert np.array_equal(R.relu_backward(ours_h, g.numpy()), z.grad.numpy(), equal_nan=True)
    nan_unit = np.isnan(ours_h) & np.isfinite(g.numpy())                         # a NaN unit passes its gradient on
    assert nan_unit.any() and np.array_equal(z.grad.numpy()[nan_unit], g.numpy()[nan_unit])
    off_unit = (ours_h == 0) & ~np.isfinite(g.numpy())                           # a unit that is off gives an exact 0
    assert off_unit.any() and not z.grad.numpy()[off_unit].any()


# ------------------------------------------------------------------------------------------------------------------ mutations
def _mutant(kind, x, params, gy, dims):
    """A float64 evaluation that is wrong in one way a kernel could be."""
    IN, H, NH, OUT = dims
    if kind == "sample_missing":                              # one sample missing from grad_params
        got = R.forward_backward(x, params, gy, dims)
        got["gp"] = R.forward_backward(x[:-1], params, gy[:-1], dims)["gp"]
        return got
    if kind == "w1_stride":                                   # W1 read with a row stride one larger than IN
        p = np.array(params, np.float64)
        p[:H * IN] = p[(np.arange(H)[:, None] * (IN + 1) + np.arange(IN)[None, :]).reshape(-1)]
        got = R.forward_backward(x, p, gy, dims)
        return got
    if kind == "tail_features":                               # the last IN % 4 input features read as zero
        x2 = np.array(x)
        x2[:, IN - IN % 4:] = 0
        return R.forward_backward(x2, params, gy, dims)
    assert kind == "fmax_relu"                                # fmaxf(z, 0) and the gate h > 0: a NaN becomes a finite row
    relu, back = R.relu, R.relu_backward
    R.relu = lambda z: np.where(z > 0, z, 0.0)
    R.relu_backward = lambda h, g: np.where(h > 0, g, 0.0)
    try:
        return R.forward_backward(x, params, gy, dims)
    finally:
        R.relu, R.relu_backward = relu, back


# tail_features needs IN % 4 != 0: the two shapes with 43 inputs (no width-16 shape has such an input width)
@pytest.mark.parametrize("kind,dims", [(k, d) for k in ("sample_missing", "w1_stride", "tail_features", "fmax_relu")
                                       for d in MUTATION_DIMS if k != "tail_features" or d[0] % 4])
def test_the_bar_rejects_a_wrong_copy(kind, dims):
    n = 4097
    x, params, gy = _inputs(dims, n, seed=dims[1])
    if kind == "fmax_relu":
        x[n // 2, 3] = np.nan
    ref = R.forward_backward(x, params, gy, dims)
    assert R.violations(ref, ref, R.ALLOWANCE) == []
    assert R.violations(R.torch_fp32(x, params, gy, dims), ref, R.ALLOWANCE) == [] or kind == "fmax_relu"
    bad = R.violations(_mutant(kind, x, params, gy, dims), ref, R.ALLOWANCE)
    assert bad, kind
    hit = {k for k, _, _ in bad}
    assert hit >= {"sample_missing": {"gp"}, "w1_stride": {"y", "gx", "gp"}, "tail_features": {"y", "gx", "gp"},
                   "fmax_relu": {"y", "gp"}}[kind], bad


# ------------------------------------------------------------------------------------------ the four-wave flush, restated in fp32
def _flush_atomic(wave_values, arrival):
    """LDS atomicAdd: the image takes the waves' fp32 accumulators in the order they arrive."""
    acc = np.float32(0.0)
    for w in arrival:
        acc = np.float32(acc + wave_values[w])
    return acc


def _flush_fixed(wave_values, arrival):
    """The waves take turns in wave order behind barriers: the arrival order does not enter."""
    acc = np.float32(0.0)
    for w in range(len(wave_values)):
        acc = np.float32(acc + wave_values[w])
    return acc


def test_four_wave_sum_depends_on_arrival_order_unless_fixed():
    vals = np.array([1.0, 2.0 ** -24, 2.0 ** -24, -1.0], np.float32)          # 1 + 2^-24 rounds back to 1; 2^-24 + 2^-24 does not
    a, b = _flush_atomic(vals, [0, 1, 2, 3]), _flush_atomic(vals, [1, 2, 0, 3])
    assert a.view(np.int32) != b.view(np.int32) and (a, b) == (np.float32(0.0), np.float32(2.0 ** -23))
    assert _flush_fixed(vals, [0, 1, 2, 3]).view(np.int32) == _flush_fixed(vals, [1, 2, 0, 3]).view(np.int32)
    rng = np.random.default_rng(0)                                             # and on ordinary numbers, often
    v = rng.standard_normal((1000, 4)).astype(np.float32)
    differ = sum(_flush_atomic(r, [0, 1, 2, 3]).view(np.int32) != _flush_atomic(r, [3, 1, 0, 2]).view(np.int32) for r in v)
    assert differ > 100
    assert all(_flush_fixed(r, [0, 1, 2, 3]).view(np.int32) == _flush_fixed(r, [3, 1, 0, 2]).view(np.int32) for r in v)


# ------------------------------------------------------------------------------------------------------------ the integer case
@pytest.mark.parametrize("dims", ALL_DIMS)
@pytest.mark.parametrize("n", [65, 129, 513])
def test_integer_case_is_exact_in_fp32(dims, n):
    x, params, gy = R.exact_case(dims, n)
    r64 = R.forward_backward(x, params, gy, dims)
    r32 = R.forward_backward(x, params, gy, dims, dtype=np.float32)
    for k in ("y", "gx", "gp"):
        assert r32[k].dtype == np.float32 and np.array_equal(r32[k].astype(np.float64), r64[k]), k
        assert r64[k + "_scale"].max() < 2 ** 24, k              # every partial sum, in any order, is an integer below 2^24
        assert np.array_equal(r64[k], np.round(r64[k]))
        assert (r64[k] != 0).mean() > 0.3, k
    for W, _ in R.unpack(params, dims):                          # neighbours differ: a shifted index changes the value
        assert np.all(W[:, 1:] != W[:, :-1]) and (W.shape[0] == 1 or np.any(W[1:] != W[:-1]))
    h = R._hidden(x.astype(np.float64), R.unpack(params.astype(np.float64), dims))[1]
    assert all((z > 0).any() and (z < 0).any() for z in h)       # the ReLUs gate both ways


# ------------------------------------------------------------------------------------------------------------------- allowance
def test_allowance_constants():
    """The stored bars are four times the stored torch figures (floor 2^-21), and a fresh measurement gives the stored figures.
    torch runs on one thread there, so its summation order does not follow the host's core count; 2 % is left for another
    vector width. Four times the fresh figures must not exceed the stored bars by more than that either."""
    assert R.ALLOWANCE == R.allowance(R.TORCH_MEASURED)
    measured = R.measure_torch()
    print("torch fp32 worst error in units of (y, gx, gp) scale:", measured, "stored:", R.TORCH_MEASURED)
    for m, s, fresh, bar in zip(measured, R.TORCH_MEASURED, R.allowance(measured), R.ALLOWANCE):
        assert abs(m - s) <= 0.02 * s, (measured, R.TORCH_MEASURED)
        assert fresh <= 1.02 * bar and bar >= R.ALLOWANCE_FLOOR


@pytest.mark.parametrize("dims", sorted(R.REJECTION))
def test_filter_rejection_share(dims):
    for (gain, scale), stored in R.REJECTION[dims].items():
        params = R.default_params(dims, 5, gain)
        share = 1.0 - R.safe_rows(R.randn_rows(7, dims[0], scale)(20_000), params, dims).mean()
        print(dims, gain, scale, f"{share:.4f}")
        assert abs(share - stored) <= 0.01, (dims, gain, scale, share, stored)


def test_draw_safe_rows_returns_only_safe_rows():
    dims = (43, 128, 2, 3)
    params = R.default_params(dims, 3)
    x, drawn = R.draw_safe_rows(R.randn_rows(4, 43), 5000, params, dims)
    assert x.shape == (5000, 43) and x.dtype == np.float32 and drawn > 5000
    assert R.safe_rows(x, params, dims).all()


# ------------------------------------------------------------------------------------------------ the compiled set of shapes
def test_supported_shapes_are_exactly_the_tested_list():
    """shacira_mlp_supported over in 1..128, hidden {16, 32, 64, 128}, num_hidden 1..3, out 1..16 (validation only: no GPU):
    a new instantiation has to be added to mlp_ref.SHAPES, which test_gpu_mlp_edges.py runs in full."""
    from shacira_amd import _lib
    L = _lib.lib()

    def scan():
        return sorted((i, h, nh, o) for i in range(1, 129) for h in (16, 32, 64, 128) for nh in (1, 2, 3) for o in range(1, 17)
                      if L.shacira_mlp_supported(i, h, nh, o))

    assert _lib.get_option("mlp_variant") == -1
    assert scan() == sorted(set(R.MFMA_SHAPES + R.VALU_SHAPES))
    _lib.set_option("mlp_variant", 0)
    try:
        assert scan() == sorted(R.VALU_SHAPES)
    finally:
        _lib.set_option("mlp_variant", -1)
    assert len(R.MFMA_SHAPES) == 13 and len(R.VALU_SHAPES) == 7 and len(R.SHAPES) == 20
    assert set(R.VALU_SHAPES) - set(R.MFMA_SHAPES) == {(32, 16, 3, 3)}
    for dims in R.MFMA_SHAPES + R.VALU_SHAPES:
        assert L.shacira_mlp_backward_workspace_bytes(*dims) >= 256 * R.num_params(dims) * 8
