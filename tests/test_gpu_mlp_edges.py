"""mlp.hip and mlp_mfma.hip at their tile, grid and NaN edges against the decoder MLP in float64 (tests/mlp_ref.py): every
instantiation (mlp_ref.SHAPES: 13 MFMA, 7 VALU), forward, grad_x and grad_params.

Sizes. MB = the MFMA block (16: width 16, 32: widths 64 and 128) or 128 for the VALU kernels (their tile). Tile and workgroup
edges 1, MB-1, MB, MB+1, 4MB-1, 4MB, 4MB+1 for all; the second trip of each grid-stride loop where it belongs: 32_767 /
32_768 / 32_769 (wide kernels, narrow backward, the split kernel's trip on zeros), 65_535 / 65_537 (VALU backward, 1 -> 2 tiles
per block), 131_073 (narrow forward), 262_145 (VALU forward).

Bar: |got - ref| <= allowance * scale elementwise, scales and allowances from mlp_ref: y_scale is the forward pass on absolute
values, gx_scale the backward chain on absolute values with the reference's gates, gp_scale per weight sum_s sdz_s ain_s (per
bias sum_s sdz_s) with sdz and ain those two chains stopped at the layer -- NOT the products sum_s |dz_s| |in_s| of the
reference's own values, which no fp32 evaluation meets at small n (mlp_ref's docstring; CPU torch fp32 misses by up to 1.5e-4
of them at n = 31). allowance = 4 x CPU torch fp32's worst miss in the same units at 70_001 rows, floor 2^-21. Rows come through
mlp_ref.safe_rows BEFORE any kernel runs; nothing is dropped afterwards. Exact cases carry no tolerance.

                                      y          grad_x     grad_params
    torch fp32 (70_001 rows)          5.2e-8     2.0e-7     2.2e-8   (2.0e-7 at the sizes of this file, where less averages out)
    allowance                         4.8e-7     8.0e-7     4.8e-7   (y and grad_params: the floor)
    MFMA kernels, random rows         1.6e-7     2.7e-7     2.2e-7   measured on the MI355X: worst over shapes, sizes,
    VALU kernels, random rows         1.3e-7     2.4e-7     4.2e-7   feature scales and initialisations
    MFMA kernels, same-sign rows      7.3e-8     2.2e-7     7.4e-8
    VALU kernels, same-sign rows      3.5e-8     2.4e-7     6.1e-8

The VALU kernels' 4.2e-7 is at feature scale 1e-4 (1.4e-7 at scale 1): they start the accumulator at the bias, so every one of
the fan-in roundings of a hidden unit happens at the size of the bias. It is 1.15 times inside the bar: a regression there is
most likely that, not a new fault. The MFMA kernels add the bias last; with it as the start value they missed the bar at one
row by 5.1e-7 to 7.4e-7. In units of the reference's own products the kernels' worst grad_params error is 9.9e-5 (MFMA) and
3.4e-5 (VALU), CPU torch's 7e-5 to 1.5e-4: printed by test_random_rows_against_float64 (pytest -s), not a bar.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import mlp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = np.float32(-1234.5678)
IDS = ["-".join(map(str, d)) + ("-mfma" if v == -1 else "-valu") for d, v in R.SHAPES]
shapes = pytest.mark.parametrize("dims,variant", R.SHAPES, ids=IDS)


def _kind(dims, variant):
    if variant == 0:
        return "valu"
    return {16: "narrow", 64: "wide", 128: "split"}[dims[1]]


def _mb(dims, variant):
    return {"valu": 128, "narrow": 16, "wide": 32, "split": 32}[_kind(dims, variant)]


def _sizes(dims, variant):
    """(sizes run forward and backward, sizes run forward only)"""
    mb, kind = _mb(dims, variant), _kind(dims, variant)
    tile = [1, mb - 1, mb, mb + 1, 4 * mb - 1, 4 * mb, 4 * mb + 1]
    grid = [65_535, 65_537] if kind == "valu" else [32_767, 32_768, 32_769]
    return sorted(set(tile + grid)), {"valu": [262_145], "narrow": [131_073]}.get(kind, [])


@contextlib.contextmanager
def _variant(v):
    from shacira_amd import _lib
    _lib.set_option("mlp_variant", v)
    try:
        yield
    finally:
        _lib.set_option("mlp_variant", -1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(dims, x, params, gy=None, need_grad_x=True):
    """x, params, gy: device tensors -> dict of numpy results (hip_ops entries)"""
    from shacira_amd import hip_ops
    out = dict(y=hip_ops.mlp_forward(x, params, *dims).cpu().numpy())
    if gy is not None:
        gx, gp = hip_ops.mlp_backward(x, params, gy, *dims, need_grad_x=need_grad_x)
        out["gx"], out["gp"] = (gx.cpu().numpy() if gx is not None else None), gp.cpu().numpy()
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _seed(dims, *more):
    return int(sum(p * v for p, v in zip((1, 131, 17_161, 2_248_091), dims)) + sum(more))


# ------------------------------------------------------------------------------------------------ 1. random rows, all sizes
@pytest.mark.parametrize("scale", [1e-4, 1.0, 1e3])
@pytest.mark.parametrize("init", ["default", "scaled"])
@shapes
def test_random_rows_against_float64(dims, variant, init, scale):
    """Filtered randn rows at feature scales 1e-4 (hash-grid features at initialisation), 1 and 1e3; nn.Linear's default
    initialisation and test_mlp.py's scaled parameters; every size of the module docstring, as prefixes of one drawn set."""
    both, fwd_only = _sizes(dims, variant)
    nmax = max(both + fwd_only)
    seed = _seed(dims, variant, int(np.log10(scale)) + 7)
    params = R.default_params(dims, seed, R.scaled_gain(dims) if init == "scaled" else 1.0)
    x, drawn = R.draw_safe_rows(R.randn_rows(seed + 1, dims[0], scale), nmax, params, dims)
    gy = np.random.default_rng(seed + 2).standard_normal((nmax, dims[3])).astype(np.float32)
    ref = R.forward_backward(x[:both[-1]], params, gy[:both[-1]], dims, sizes=both)
    xd, pd, gd = _dev(x), _dev(params), _dev(gy)
    failures, worst, products = [], np.zeros(3), 0.0
    with _variant(variant):
        for n in both:
            got, want = _run(dims, xd[:n], pd, gd[:n]), R.prefix(ref, n)
            worst = np.maximum(worst, R.errors_in_scale(got, want))
            products = max(products, R.products_error(got, want))
            failures += [(n,) + b for b in R.violations(got, want, R.ALLOWANCE)]
        for n in fwd_only:
            got, want = _run(dims, xd[:n], pd), R.forward_scaled(x[:n], params, dims)
            worst = np.maximum(worst, R.errors_in_scale(got, want))
            failures += [(n,) + b for b in R.violations(got, want, R.ALLOWANCE)]
    print(f"{dims} variant {variant} {init} scale {scale:g}: worst y {worst[0]:.3g} gx {worst[1]:.3g} gp {worst[2]:.3g} of the "
          f"scales (allowance {R.ALLOWANCE[0]:.3g} {R.ALLOWANCE[1]:.3g} {R.ALLOWANCE[2]:.3g}); gp in units of the reference's own "
          f"products {products:.3g}; drew {drawn} rows for {nmax}")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------- 2. same-sign rows
@shapes
def test_same_sign_rows(dims, variant):
    """x >= 0 and grad_y > 0: nothing cancels in the fp32 accumulators that persist across a wave's (a thread's) tiles."""
    sizes = [32_769, 70_001]
    seed = _seed(dims, variant, 99)
    params = R.default_params(dims, seed)
    x, _ = R.draw_safe_rows(R.randn_rows(seed + 1, dims[0], same_sign=True), sizes[-1], params, dims)
    gy = (np.abs(np.random.default_rng(seed + 2).standard_normal((sizes[-1], dims[3]))) + 2.0 ** -10).astype(np.float32)
    assert (x >= 0).all() and (gy > 0).all()
    ref = R.forward_backward(x, params, gy, dims, sizes=sizes)
    xd, pd, gd = _dev(x), _dev(params), _dev(gy)
    failures, worst = [], np.zeros(3)
    with _variant(variant):
        for n in sizes:
            got, want = _run(dims, xd[:n], pd, gd[:n]), R.prefix(ref, n)
            worst = np.maximum(worst, R.errors_in_scale(got, want))
            failures += [(n,) + b for b in R.violations(got, want, R.ALLOWANCE)]
    print(f"{dims} variant {variant} same sign: worst y {worst[0]:.3g} gx {worst[1]:.3g} gp {worst[2]:.3g} of the scales")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------ 3. exact case
@shapes
def test_integer_case_is_exact(dims, variant):
    """Small integer weights, one-hot integer rows: every product and partial sum is exact in fp32 in any order
    (test_mlp_ref_cpu.py::test_integer_case_is_exact_in_fp32), so y, grad_x and grad_params equal the reference, no tolerance.
    Feature s mod IN is hot in row s: every k block of the first layer, its zero padding (IN = 43, 24 and 48 on MB 16, 96) and
    the k order of the register chaining; OUT = 3, 4 and 16."""
    n = 4 * _mb(dims, variant) + 1
    x, params, gy = R.exact_case(dims, n)
    ref = R.forward_backward(x, params, gy, dims)
    with _variant(variant):
        got = _run(dims, _dev(x), _dev(params), _dev(gy))
    for k in ("y", "gx", "gp"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].astype(np.float64), ref[k]), \
            (k, int((got[k] != ref[k]).sum()), float(np.abs(got[k] - ref[k]).max()))


# ------------------------------------------------------------------------------------------------------ 4. row independence
@shapes
def test_rows_do_not_depend_on_their_position(dims, variant):
    for n in (4 * _mb(dims, variant) + 1, 32_769):
        rng = np.random.default_rng(_seed(dims, variant, n))
        params = R.default_params(dims, n, R.scaled_gain(dims))
        x = rng.standard_normal((n, dims[0])).astype(np.float32)
        gy = rng.standard_normal((n, dims[3])).astype(np.float32)
        p = rng.permutation(n)
        with _variant(variant):
            a = _run(dims, _dev(x), _dev(params), _dev(gy))
            b = _run(dims, _dev(x[p]), _dev(params), _dev(gy[p]))
        for k in ("y", "gx"):
            assert np.array_equal(_bits(a[k][p]), _bits(b[k])), (n, k)


# -------------------------------------------------------------------------------------------------------- 5. non-finite rows
@pytest.mark.parametrize("bad", ["nan_x", "inf_x", "nan_gy", "inf_gy"])
@shapes
def test_non_finite_rows(dims, variant, bad):
    """A NaN / +inf feature or grad_y entry in the first and the last row of a tile and in the ragged tail: NaN and +-inf exactly
    where the float64 reference has them (y, grad_x, grad_params), every other row bit-identical to the run without them."""
    mb = _mb(dims, variant)
    n = 4 * mb + 3
    rows = [0, mb - 1, mb, 2 * mb - 1, 4 * mb, 4 * mb + 2]
    seed = _seed(dims, variant, 5)
    params = R.default_params(dims, seed, R.scaled_gain(dims))
    x, _ = R.draw_safe_rows(R.randn_rows(seed + 1, dims[0]), n, params, dims)
    gy = np.random.default_rng(seed + 2).standard_normal((n, dims[3])).astype(np.float32)
    x2, gy2 = x.copy(), gy.copy()
    value = np.float32(np.nan if bad.startswith("nan") else np.inf)
    for r in rows:
        if bad.endswith("_x"):
            x2[r, (7 * r + 3) % dims[0]] = value
        else:
            gy2[r, r % dims[3]] = value
    ref = R.forward_backward(x2, params, gy2, dims)
    hit = ~np.isfinite(ref["y"]).all(axis=1) | ~np.isfinite(ref["gx"]).all(axis=1)
    assert sorted(np.flatnonzero(hit)) == rows and np.isnan(ref["gp"]).any()
    with _variant(variant):
        clean = _run(dims, _dev(x), _dev(params), _dev(gy))
        got = _run(dims, _dev(x2), _dev(params), _dev(gy2))
    assert R.violations(got, ref, R.ALLOWANCE) == []
    for k in ("y", "gx"):
        assert np.isfinite(clean[k]).all()
        assert np.array_equal(_bits(got[k][~hit]), _bits(clean[k][~hit])), k
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])) and np.array_equal(np.isinf(got[k]), np.isinf(ref[k])), k
    assert np.array_equal(np.isnan(got["gp"]), np.isnan(ref["gp"]))


# ------------------------------------------------------------------------------------------------- the C-ABI through ctypes
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _guarded(count, guard):
    """`count` floats inside a sentinel-filled device buffer with `guard` floats on either side (guard % 4 == 0: aligned)"""
    buf = torch.full((count + 2 * guard,), float(SENTINEL), dtype=torch.float32, device=DEV)
    return buf, buf[guard:guard + count]


def _untouched(buf, count, guard):
    host = _bits(buf.cpu().numpy())
    want = SENTINEL.view(np.int32)
    return bool(np.all(host[:guard] == want) and np.all(host[guard + count:] == want))


def _abi_backward(dims, n, xd, pd, gd, gx_ptr, gp_ptr, ws=None, ws_bytes=None):
    from shacira_amd import _lib
    L = _lib.lib()
    need = L.shacira_mlp_backward_workspace_bytes(*dims)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(0):
        rc = L.shacira_mlp_backward(n, *dims, xd.data_ptr() if xd is not None else None, pd.data_ptr() if pd is not None else None,
                                    gd.data_ptr() if gd is not None else None, gx_ptr, gp_ptr, ws.data_ptr(),
                                    need if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------------------- 6. overrun
@shapes
def test_nothing_is_written_past_the_last_row(dims, variant):
    """y and grad_x one row longer than the batch, grad_params with 4 floats behind it, the workspace exactly as long as
    shacira_mlp_backward_workspace_bytes says inside a larger buffer: all sentinels outside are intact."""
    from shacira_amd import _lib
    L = _lib.lib()
    IN, H, NH, OUT = dims
    P = R.num_params(dims)
    for n in (_mb(dims, variant) + 1, 32_769):
        rng = np.random.default_rng(_seed(dims, variant, n))
        xd = _dev(rng.standard_normal((n, IN)).astype(np.float32))
        gd = _dev(rng.standard_normal((n, OUT)).astype(np.float32))
        pd = _dev(R.default_params(dims, n, R.scaled_gain(dims)))
        with _variant(variant):
            want = _run(dims, xd, pd, gd)
            ybuf, y = _guarded(n * OUT, 4 * OUT)
            gxbuf, gx = _guarded(n * IN, 4 * IN)
            gpbuf, gp = _guarded(P, 4)
            need = L.shacira_mlp_backward_workspace_bytes(*dims)
            assert need % 16 == 0
            wsbuf = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=DEV)
            with torch.cuda.device(0):
                rc = L.shacira_mlp_forward(n, *dims, xd.data_ptr(), pd.data_ptr(), y.data_ptr(), _stream())
            assert rc == 0
            assert _abi_backward(dims, n, xd, pd, gd, gx.data_ptr(), gp.data_ptr(), ws=wsbuf[256:256 + need]) == 0
        assert _untouched(ybuf, n * OUT, 4 * OUT) and _untouched(gxbuf, n * IN, 4 * IN) and _untouched(gpbuf, P, 4), n
        ws_host = wsbuf.cpu().numpy()
        assert np.all(ws_host[:256] == 0x5A) and np.all(ws_host[256 + need:] == 0x5A), n
        assert np.array_equal(_bits(y.cpu().numpy().reshape(n, OUT)), _bits(want["y"]))
        assert np.array_equal(_bits(gx.cpu().numpy().reshape(n, IN)), _bits(want["gx"]))
        assert np.array_equal(_bits(gp.cpu().numpy()), _bits(want["gp"]))


# ------------------------------------------------------------------------------------------------------ 7. grad_x == NULL
@shapes
def test_backward_without_grad_x(dims, variant):
    from shacira_amd.wisp.models.decoders import BasicDecoder
    IN, H, NH, OUT = dims
    for n in (4 * _mb(dims, variant) + 1, 32_769):
        rng = np.random.default_rng(_seed(dims, variant, n, 7))
        xd = _dev(rng.standard_normal((n, IN)).astype(np.float32))
        gd = _dev(rng.standard_normal((n, OUT)).astype(np.float32))
        pd = _dev(R.default_params(dims, n, R.scaled_gain(dims)))
        with _variant(variant):
            a = _run(dims, xd, pd, gd)
            b = _run(dims, xd, pd, gd, need_grad_x=False)
        assert b["gx"] is None and np.array_equal(_bits(a["gp"]), _bits(b["gp"])), n
        assert np.array_equal(_bits(a["y"]), _bits(b["y"]))
    # through the module: an input that does not require grad takes the NULL path
    torch.manual_seed(_seed(dims))
    dec = BasicDecoder(IN, OUT, torch.relu, True, torch.nn.Linear, NH, H, []).to(DEV)
    grads = []
    with _variant(variant):
        for req in (True, False):
            dec.zero_grad()
            xin = xd.clone().requires_grad_(req)
            dec(xin).backward(gd)
            grads.append([p.grad.cpu().numpy().copy() for p in dec.parameters()])
            assert (xin.grad is not None) == req
    for ga, gb in zip(*grads):
        assert np.array_equal(_bits(ga), _bits(gb))
    packed = np.concatenate([g.reshape(-1) for g in grads[0]])
    with _variant(variant):
        direct = _run(dims, xd, dec.packed_params().detach(), gd)
    assert np.array_equal(_bits(packed), _bits(direct["gp"]))


# ------------------------------------------------------------------------------------------------------- 8. num_rows == 0
@shapes
def test_zero_rows(dims, variant):
    from shacira_amd import _lib, hip_ops
    L = _lib.lib()
    IN, H, NH, OUT = dims
    P = R.num_params(dims)
    pd = _dev(R.default_params(dims, 1))
    x0 = torch.empty((0, IN), dtype=torch.float32, device=DEV)
    g0 = torch.empty((0, OUT), dtype=torch.float32, device=DEV)
    with _variant(variant):
        y = hip_ops.mlp_forward(x0, pd, *dims)
        gx, gp = hip_ops.mlp_backward(x0, pd, g0, *dims)
        assert tuple(y.shape) == (0, OUT) and tuple(gx.shape) == (0, IN)
        assert gp.shape == pd.shape and not gp.cpu().numpy().any()
        gpbuf, gpv = _guarded(P, 4)
        with torch.cuda.device(0):
            assert L.shacira_mlp_forward(0, *dims, None, pd.data_ptr(), None, _stream()) == 0
        assert _abi_backward(dims, 0, None, pd, None, None, gpv.data_ptr()) == 0
    assert _untouched(gpbuf, P, 4)
    assert np.array_equal(_bits(gpv.cpu().numpy()), np.zeros(P, np.int32))      # exact zeros, +0.0


# ---------------------------------------------------------------------------------------------------- 9. reproducibility
@shapes
def test_backward_is_reproducible(dims, variant):
    """Five calls on the same 70_001 rows: grad_params (and grad_x) bit-identical. Compares bits; it does not chase a fault."""
    n = 70_001
    rng = np.random.default_rng(_seed(dims, variant, 9))
    xd = _dev(rng.standard_normal((n, dims[0])).astype(np.float32))
    gd = _dev(rng.standard_normal((n, dims[3])).astype(np.float32))
    pd = _dev(R.default_params(dims, 9, R.scaled_gain(dims)))
    from shacira_amd import hip_ops
    with _variant(variant):
        runs = [hip_ops.mlp_backward(xd, pd, gd, *dims) for _ in range(5)]
    first = [_bits(t.cpu().numpy()) for t in runs[0]]
    differing = [sum(int((_bits(t.cpu().numpy()) != f).sum()) for t, f in zip(run, first)) for run in runs[1:]]
    assert differing == [0, 0, 0, 0], differing


# --------------------------------------------------------------------------------------------------------- 10. alignment
def _views(off, arrays):
    """The arrays as views into ONE flat device buffer, array k starting (off + k) % 4 elements past a 16-byte boundary, or at
    a boundary for off = None."""
    cursor, starts = 0, []
    for k, a in enumerate(arrays):
        s = cursor + 4
        s += ((0 if off is None else (off + k - 1) % 3 + 1) - s) % 4
        starts.append(s)
        cursor = s + a.size
    host = np.full(cursor + 4, SENTINEL, np.float32)
    for s, a in zip(starts, arrays):
        host[s:s + a.size] = a.reshape(-1)
    flat = torch.from_numpy(host).to(DEV)
    views = [flat[s:s + a.size].view(a.shape) for s, a in zip(starts, arrays)]
    for k, v in enumerate(views):
        assert v.data_ptr() % 16 == (0 if off is None else 4 * ((off + k - 1) % 3 + 1)) and v.is_contiguous()
    return flat, views


@pytest.mark.parametrize("off", [1, 2, 3])
@shapes
def test_four_byte_aligned_operands(dims, variant, off):
    """x, grad_y and params as 4-byte-aligned views into one flat buffer (1, 2 or 3 elements past a 16-byte boundary, each
    operand another). hip_ops copies an x whose rows the kernels read as float4 (IN % 4 == 0); through hip_ops and through
    BasicDecoder the results are bit-identical to the aligned call. The C-ABI refuses such an x, grad_x or y with
    SHACIRA_EINVAL and writes nothing; an x with IN % 4 != 0 (scalar loads) is accepted and gives the same bits."""
    from shacira_amd import _lib
    from shacira_amd.wisp.models.decoders import BasicDecoder
    L = _lib.lib()
    IN, H, NH, OUT = dims
    P = R.num_params(dims)
    n = 4 * _mb(dims, variant) + 1
    rng = np.random.default_rng(_seed(dims, variant, off))
    arrays = [rng.standard_normal((n, IN)).astype(np.float32), rng.standard_normal((n, OUT)).astype(np.float32),
              R.default_params(dims, off, R.scaled_gain(dims))]
    _, (xa, ga, pa) = _views(None, arrays)
    flat, (xm, gm, pm) = _views(off, arrays)
    before = flat.cpu().numpy()
    with _variant(variant):
        want = _run(dims, xa, pa, ga)
        got = _run(dims, xm, pm, gm)
        for k in ("y", "gx", "gp"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        # the module: a misaligned view as the input
        torch.manual_seed(1)
        dec = BasicDecoder(IN, OUT, torch.relu, True, torch.nn.Linear, NH, H, []).to(DEV)
        outs = []
        for xin, gin in ((xa, ga), (xm, gm)):
            dec.zero_grad()
            xin = xin.detach().requires_grad_(True)
            y = dec(xin)
            y.backward(gin)
            outs.append([y.detach().cpu().numpy(), xin.grad.cpu().numpy()] + [p.grad.cpu().numpy().copy() for p in dec.parameters()])
        for a, b in zip(*outs):
            assert np.array_equal(_bits(a), _bits(b))
        # the C-ABI
        ybuf, y = _guarded(n * OUT, 8)
        gxbuf, gx = _guarded(n * IN, 8)
        gpbuf, gp = _guarded(P, 8)
        with torch.cuda.device(0):
            rc = L.shacira_mlp_forward(n, *dims, xm.data_ptr(), pm.data_ptr(), y.data_ptr(), _stream())
            torch.cuda.synchronize()
        rcb = _abi_backward(dims, n, xm, pm, gm, gx.data_ptr(), gp.data_ptr())
        if IN % 4 == 0:
            assert rc == _lib.EINVAL and rcb == _lib.EINVAL
            assert _untouched(ybuf, 0, 8) and _untouched(gxbuf, 0, 8) and _untouched(gpbuf, 0, 8)        # nothing ran
            assert _abi_backward(dims, n, xa, pm, gm, gx.data_ptr() + 4 * off, gp.data_ptr()) == _lib.EINVAL
            assert _untouched(gxbuf, 0, 8) and _untouched(gpbuf, 0, 8)
        else:
            assert rc == 0 and rcb == 0
            assert np.array_equal(_bits(y.cpu().numpy().reshape(n, OUT)), _bits(want["y"]))
            assert np.array_equal(_bits(gx.cpu().numpy().reshape(n, IN)), _bits(want["gx"]))
            assert np.array_equal(_bits(gp.cpu().numpy()), _bits(want["gp"]))
            assert _untouched(ybuf, n * OUT, 8) and _untouched(gxbuf, n * IN, 8) and _untouched(gpbuf, P, 8)
        with torch.cuda.device(0):
            rc = L.shacira_mlp_forward(n, *dims, xa.data_ptr(), pm.data_ptr(), y.data_ptr() + 4 * off, _stream())
            torch.cuda.synchronize()
        if OUT % 4 == 0:
            assert rc == _lib.EINVAL
        else:
            assert rc == 0                                    # scalar stores: any 4-byte alignment
            host = ybuf.cpu().numpy()
            assert np.array_equal(_bits(host[8 + off:8 + off + n * OUT].reshape(n, OUT)), _bits(want["y"]))
            assert host[8 + off + n * OUT] == SENTINEL
    assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before))                                      # inputs are only read


# ---------------------------------------------------------------------------------------------------------- 11. refusals
def test_refusals():
    from shacira_amd import _lib
    L = _lib.lib()
    dims, n = (32, 16, 2, 3), 8
    P = R.num_params(dims)
    xd, gd, pd = (torch.zeros(k, device=DEV) for k in (n * 32, n * 3, P))
    ybuf, y = _guarded(n * 3, 4)
    gxbuf, gx = _guarded(n * 32, 4)
    gpbuf, gp = _guarded(P, 4)
    need = L.shacira_mlp_backward_workspace_bytes(*dims)
    assert need > 0 and L.shacira_mlp_backward_workspace_bytes(33, 16, 2, 3) == 0
    ptrs = (xd.data_ptr(), pd.data_ptr())
    with torch.cuda.device(0):
        assert L.shacira_mlp_forward(n, 33, 16, 2, 3, *ptrs, y.data_ptr(), _stream()) == _lib.EDTYPE     # unsupported shape
        assert L.shacira_mlp_forward(-1, *dims, *ptrs, y.data_ptr(), _stream()) == _lib.EINVAL           # negative num_rows
        assert L.shacira_mlp_forward(n, *dims, xd.data_ptr(), None, y.data_ptr(), _stream()) == _lib.EINVAL   # null params
        assert L.shacira_mlp_forward(n, *dims, None, pd.data_ptr(), y.data_ptr(), _stream()) == _lib.EINVAL
        assert L.shacira_mlp_forward(n, *dims, *ptrs, None, _stream()) == _lib.EINVAL
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    back = lambda n_, d, x_, p_, g_, gp_, nbytes: _abi_backward(d, n_, x_, p_, g_, gx.data_ptr(), gp_, ws=ws, ws_bytes=nbytes)
    # (_abi_backward's default workspace size is the queried one; here the sizes are given)
    assert back(n, (33, 16, 2, 3), xd, pd, gd, gp.data_ptr(), need) == _lib.EDTYPE
    assert back(n, dims, xd, pd, gd, gp.data_ptr(), need - 1) == _lib.EWORKSPACE                         # one byte short
    assert back(-1, dims, xd, pd, gd, gp.data_ptr(), need) == _lib.EINVAL
    assert back(n, dims, xd, None, gd, gp.data_ptr(), need) == _lib.EINVAL                               # null params
    assert back(n, dims, xd, pd, gd, None, need) == _lib.EINVAL                                          # null grad_params
    assert back(n, dims, None, pd, gd, gp.data_ptr(), need) == _lib.EINVAL
    assert back(n, dims, xd, pd, None, gp.data_ptr(), need) == _lib.EINVAL
    assert _untouched(ybuf, 0, 4) and _untouched(gxbuf, 0, 4) and _untouched(gpbuf, 0, 4)                # nothing ran
    assert back(n, dims, xd, pd, gd, gp.data_ptr(), need) == 0                                           # ... and the valid call
    assert _untouched(gpbuf, P, 4) and _untouched(gxbuf, n * 32, 4)
