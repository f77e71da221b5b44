"""SSIM on the MI355X: the fused HIP kernels of ssim.hip (hip_ops.ssim_forward / ssim_backward, metrics.ssim / ssim_map /
ssim_loss) against the fp64 restatement of the definition (tests/ssim_ref.py) and, for the gradient, against fp64 autograd of
metrics.ssim_torch (itself held to the restatement and to finite differences in tests/test_ssim_cpu.py).

Bounds. The kernel is fp32 and may order its sums differently from scipy, so it is held to the fp32 error of the definition
itself, measured on the very input of each case:
  value     |got - ref64| <= max(8 * d32, 16 * 2^-24),  d32 = |ref32 - ref64|  (the restatement run in fp32 and in fp64)
  map       the same rule per pixel, d32 = the largest per-pixel deviation, reflect borders and corners included
  gradient  m = max|g - g64| / max|g64| <= max(8 * m32, 16 * 2^-24),  m32 = the same measure of ssim_torch's fp32 autograd
The floor: d32 can be 0 by luck, and S is a ratio of magnitude at most 1 out of about a dozen fp32 roundings.
Every case prints its error / bound ratio (pytest -s); the largest observed are recorded in profiles/ssim.md.

Shapes: the kernel's tile is T_h x T_w = 16 x 64 pixels (SHACIRA_SSIM_TILE_H / _W), tiles counted from pixel (0, 0).
"""
import ctypes

import numpy as np
import pytest
import torch

import ssim_ref

pytestmark = pytest.mark.gpu
TH, TW = 16, 64
FLOOR = 16 * 2.0 ** -24

SHAPES = [(11, 11), (11, 40), (40, 11), (12, 75)]
# the last tile of the valid region at one valid row / column short of full, exactly full, one over, and two tiles and one over
SHAPES += [(h, w) for h in (TH + 9, TH + 10, TH + 11, 2 * TH + 11) for w in (TW + 9, TW + 10, TW + 11, 2 * TW + 11)]
# tiles are counted from pixel 0: a second tile that holds one row / column of the map only, none of the valid region (the first
# tile's last row is the last valid one), exactly one valid row / column
SHAPES += [(TH + 1, TW + 1), (TH + 5, TW + 5), (TH + 6, TW + 6)]
CASES = [(h, w, 3, 3) for h, w in SHAPES] + [(97, 131, 1, 1), (97, 131, 3, 3), (97, 131, 3, 4)]     # (H, W, C, Cin)
KINDS = ("noise002", "noise02", "sinusoid", "inverted", "flat")
GRAD_CASES = [(11, 11, 3, 3), (12, 75, 3, 3), (TH + 11, TW + 11, 3, 3), (2 * TH + 11, TW + 9, 3, 3), (97, 131, 3, 4)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    assert (_lib.SSIM_TILE_H, _lib.SSIM_TILE_W) == (TH, TW)
    _lib.lib()
    return torch.device("cuda:0")


def images(kind, h, w, cin, seed=0):
    """(prediction x, target y) fp32 [h, w, cin] of one of the input kinds."""
    rng = np.random.default_rng([seed, h, w, cin, KINDS.index(kind)])
    n1, n2 = rng.uniform(0, 1, (h, w, cin)), rng.uniform(-1, 1, (h, w, cin))
    if kind in ("noise002", "noise02"):
        x = 0.2 + 0.6 * n1
        y = x + (0.02 if kind == "noise002" else 0.2) * n2
    elif kind == "sinusoid":
        r, c, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(cin), indexing="ij")
        y = 0.5 + 0.4 * np.sin(0.23 * r + 0.4 * k) * np.cos(0.17 * c - 0.3 * k)
        x = y + 0.05 * n2
    elif kind == "inverted":
        x = n1
        y = 1.0 - x            # the value is negative
    else:
        x, y = 0.7 + 1e-3 * n1, 0.7 + 1e-3 * (0.5 + 0.5 * n2)      # uxx - ux * ux cancels
    return x.astype(np.float32), y.astype(np.float32)


_FORWARD = {}


def forward_case(dev, h, w, c, cin):
    """Per input kind: the restatement in fp64 and fp32 and the kernel's (value, map), computed once per shape."""
    key = (h, w, c, cin)
    if key not in _FORWARD:
        from shacira_amd import hip_ops
        out = {}
        for kind in KINDS:
            x, y = images(kind, h, w, cin)
            v64, m64 = ssim_ref.ssim(x[..., :c], y[..., :c], np.float64)
            v32, m32 = ssim_ref.ssim(x[..., :c], y[..., :c], np.float32)
            value, smap = hip_ops.ssim_forward(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), channels=c,
                                               with_map=True)
            assert value.dtype == torch.float64 and smap.dtype == torch.float32 and tuple(smap.shape) == (h, w, c)
            only, none = hip_ops.ssim_forward(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), channels=c)
            assert none is None
            out[kind] = dict(v64=v64, v32=v32, m64=m64, m32=m32, value=value.item(), map=smap.cpu().numpy(),
                             value_only=only.item())
        _FORWARD[key] = out
    return _FORWARD[key]


@pytest.mark.parametrize("h,w,c,cin", CASES)
def test_value_against_the_fp64_restatement(dev, h, w, c, cin):
    for kind, r in forward_case(dev, h, w, c, cin).items():
        bound = max(8 * abs(r["v32"] - r["v64"]), FLOOR)
        err = abs(r["value"] - r["v64"])
        print(f"SSIM_VALUE {h}x{w}x{c}/{cin} {kind}: ssim {r['v64']:+.9f} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound, (kind, err, bound)
        assert r["value_only"] == r["value"], kind         # with or without the map: one tiling, one order of the sums
        if kind == "inverted":
            assert r["value"] < 0


@pytest.mark.parametrize("h,w,c,cin", CASES)
def test_full_map_against_the_fp64_restatement(dev, h, w, c, cin):
    for kind, r in forward_case(dev, h, w, c, cin).items():
        bound = max(8 * float(np.abs(r["m32"].astype(np.float64) - r["m64"]).max()), FLOOR)
        diff = np.abs(r["map"].astype(np.float64) - r["m64"])
        err = float(diff.max())
        print(f"SSIM_MAP {h}x{w}x{c}/{cin} {kind}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound, (kind, err, bound, np.unravel_index(diff.argmax(), diff.shape))


def reference_gradients(x, y, c, data_range=1.0):
    """d ssim / d x over the first c channels by autograd of ssim_torch, in fp64 and in fp32 (host)."""
    from shacira_amd.wisp.ops.image.metrics import ssim_torch
    out = []
    for dtype in (torch.float64, torch.float32):
        a = torch.from_numpy(x[..., :c]).to(dtype).requires_grad_(True)
        (g,) = torch.autograd.grad(ssim_torch(a, torch.from_numpy(y[..., :c]).to(dtype), data_range=data_range), a)
        out.append(g.double().numpy())
    return out


def gradient_check(label, g, g64, g32):
    scale = float(np.abs(g64).max())
    m = float(np.abs(g - g64).max())
    m32 = float(np.abs(g32 - g64).max())
    bound = max(8 * m32, FLOOR * scale)                      # the measures times max|g64|: no division by a zero gradient
    print(f"SSIM_GRAD {label}: max|g64| {scale:.3e} m {m / scale if scale else 0.0:.3e} m32 {m32 / scale if scale else 0.0:.3e} "
          f"ratio {m / bound if bound else 0.0:.3f}")
    assert np.isfinite(g).all() and m <= bound, (label, m, bound)


@pytest.mark.parametrize("h,w,c,cin", GRAD_CASES)
def test_backward_against_fp64_autograd(dev, h, w, c, cin):
    from shacira_amd import hip_ops
    for kind in KINDS:
        x, y = images(kind, h, w, cin, seed=1)
        g64, g32 = reference_gradients(x, y, c)
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        g = hip_ops.ssim_backward(xd, yd, torch.ones((), device=dev), channels=c)
        assert g.dtype == torch.float32 and tuple(g.shape) == (h, w, cin)
        gradient_check(f"{h}x{w}x{c}/{cin} {kind}", g[..., :c].double().cpu().numpy(), g64, g32)
        assert torch.count_nonzero(g[..., c:]) == 0                              # channels beyond C: exactly zero
        assert torch.equal(hip_ops.ssim_backward(xd, yd, 1.0, channels=c), g)     # a number for the scalar
        half = hip_ops.ssim_backward(xd, yd, torch.full((1,), -0.5, device=dev), channels=c)
        assert torch.equal(half, g * -0.5)                                        # the scalar scales, exactly for a power of two
        zero = hip_ops.ssim_backward(xd, yd, torch.zeros((), device=dev), channels=c)
        assert torch.count_nonzero(zero) == 0                                     # grad_output 0: exactly zero


def test_identical_images(dev):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.image import metrics
    for h, w, cin in ((11, 11, 3), (TH + 11, TW + 11, 3), (97, 131, 1)):
        x, _ = images("noise02", h, w, cin)
        xd = torch.from_numpy(x).to(dev)
        assert metrics.ssim(xd, xd.clone()) == 1.0
        value, smap = hip_ops.ssim_forward(xd, xd.clone(), with_map=True)
        assert value.item() == 1.0 and bool((smap == 1.0).all())
        g = hip_ops.ssim_backward(xd, xd.clone(), 1.0)
        g64, g32 = reference_gradients(x, x, cin)
        gradient_check(f"{h}x{w}x{cin} x == y", g.double().cpu().numpy(), g64, g32)


def test_two_calls_return_identical_bits(dev):
    from shacira_amd import hip_ops
    x, y = (torch.from_numpy(t).to(dev) for t in images("noise02", 2 * TH + 11, 2 * TW + 11, 4))
    first = hip_ops.ssim_forward(x, y, channels=3, with_map=True) + (hip_ops.ssim_backward(x, y, 1.0, channels=3),)
    hip_ops.ssim_forward(y, x, channels=3, with_map=True)                 # other work through the same workspace in between
    again = hip_ops.ssim_forward(x, y, channels=3, with_map=True) + (hip_ops.ssim_backward(x, y, 1.0, channels=3),)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def test_rgb_of_an_rgba_buffer_without_a_copy(dev):
    from shacira_amd.wisp.ops.image import metrics
    x, y = (torch.from_numpy(t).to(dev) for t in images("noise02", 40, 70, 4))
    x[..., 3], y[..., 3] = 0.25, 0.75                                      # an alpha channel that must not count
    want = metrics.ssim(x[..., :3].contiguous(), y[..., :3].contiguous())
    assert metrics.ssim(x, y) == want and metrics.ssim(x[..., :3], y[..., :3]) == want
    assert torch.equal(metrics.ssim_map(x, y), metrics.ssim_map(x[..., :3].contiguous(), y[..., :3].contiguous()))
    ref, _ = ssim_ref.ssim(x[..., :3].cpu().numpy(), y[..., :3].cpu().numpy())
    assert abs(want - ref) <= 1e-5


def test_a_nan_pixel(dev):
    from shacira_amd import hip_ops
    h, w, r, c, ch = 48, 80, 20, 30, 1
    x, y = images("noise02", h, w, 3)
    x[r, c, ch] = np.nan
    value, smap = hip_ops.ssim_forward(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), with_map=True)
    assert np.isnan(value.item())
    want = np.zeros((h, w, 3), bool)
    want[r - 5:r + 6, c - 5:c + 6, ch] = True                              # the pixel's 11 x 11 neighbourhood, its channel only
    assert np.array_equal(np.isnan(smap.cpu().numpy()), want)
    g = hip_ops.ssim_backward(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), 1.0)
    assert bool(torch.isnan(g[r, c, ch])) and bool(torch.isfinite(g[..., 0]).all())


def test_contract_edges(dev):
    from shacira_amd import _lib, hip_ops
    from shacira_amd.wisp.ops.image import metrics
    for h, w in ((10, 40), (40, 10)):
        a = torch.rand(h, w, 3, device=dev)
        for call in (lambda: hip_ops.ssim_forward(a, a), lambda: hip_ops.ssim_backward(a, a, 1.0), lambda: metrics.ssim(a, a),
                     lambda: metrics.ssim_loss(a, a)):
            with pytest.raises(ValueError):
                call()
    L = _lib.lib()
    a = torch.rand(16, 16, 4, device=dev)
    out, ws = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros(1024, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fwd = lambda h, w, cin, c, x=a, value=out: L.shacira_ssim_forward(h, w, cin, c, p(x) if x is not None else None, p(a), 1.0,
                                                                       p(value) if value is not None else None, None, p(ws),
                                                                       1024, None)
    assert fwd(10, 16, 4, 3) == _lib.EINVAL and fwd(16, 10, 4, 3) == _lib.EINVAL          # below the window
    assert fwd(16, 16, 4, 0) == _lib.EINVAL and fwd(16, 16, 3, 4) == _lib.EINVAL          # C < 1, C > Cin
    assert fwd(16, 16, 4, 3, x=None) == _lib.EINVAL and fwd(16, 16, 4, 3, value=None) == _lib.EINVAL
    g = torch.ones(1, device=dev)
    assert L.shacira_ssim_backward(10, 16, 4, 3, p(a), p(a), 1.0, p(g), p(a), p(ws), 1024, None) == _lib.EINVAL
    assert L.shacira_ssim_backward(16, 16, 4, 3, p(a), p(a), 1.0, None, p(a), p(ws), 1024, None) == _lib.EINVAL
    assert L.shacira_ssim_backward(16, 16, 4, 3, p(a), p(a), 1.0, p(g), p(a), p(ws), 1024, None) == _lib.EWORKSPACE
    assert L.shacira_ssim_workspace_bytes(10, 16, 3, 0) == 0
    assert L.shacira_ssim_workspace_bytes(16, 16, 3, 0) == 3 * 8 and L.shacira_ssim_workspace_bytes(16, 16, 3, 1) == 3 * 3 * 256 * 4
    assert fwd(16, 16, 4, 3) == 0
    torch.cuda.synchronize()
    assert out.item() == 1.0                                               # nothing above was enqueued over it: a is a
    with pytest.raises(RuntimeError):
        hip_ops.ssim_forward(torch.rand(16, 16, 3), torch.rand(16, 16, 3))             # host tensors
    with pytest.raises(RuntimeError):
        hip_ops.ssim_forward(a.double(), a.double())


def test_ssim_loss_is_differentiable_and_capturable(dev):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.image import metrics
    x, y = (torch.from_numpy(t).to(dev) for t in images("noise02", 64, 48, 3))
    pred = x.clone().requires_grad_(True)
    loss = metrics.ssim_loss(pred, y)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.device == dev
    (3.0 * loss).backward()
    value, _ = hip_ops.ssim_forward(x, y)
    assert loss.item() == np.float32(1.0 - value.item())
    assert torch.equal(pred.grad, hip_ops.ssim_backward(x, y, -3.0))
    g64, g32 = reference_gradients(x.cpu().numpy(), y.cpu().numpy(), 3)
    gradient_check("ssim_loss 64x48x3", pred.grad.double().cpu().numpy() / -3.0, g64, g32)
    # one captured step: loss and gradient without a host read-back
    static = x.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.autograd.grad(metrics.ssim_loss(static, y), static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured_loss = metrics.ssim_loss(static, y)
        (captured_grad,) = torch.autograd.grad(captured_loss, static)
    captured_loss.fill_(7.0)
    captured_grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = x.clone().requires_grad_(True)
    (eager_grad,) = torch.autograd.grad(metrics.ssim_loss(eager, y), eager)
    assert torch.equal(captured_loss, loss.detach()) and torch.equal(captured_grad, eager_grad)


def test_evaluate_image(dev):
    from shacira_amd import harness, hip_ops
    from shacira_amd.wisp.ops.image import metrics
    x, y = (torch.from_numpy(t).to(dev) for t in images("noise002", 64, 96, 3))
    got = harness.evaluate_image(x, y)
    assert set(got) == {"psnr", "ssim"}
    assert got["psnr"] == metrics.psnr(x, y)
    assert got["ssim"] == hip_ops.ssim_forward(x, y)[0].item()
    ref, _ = ssim_ref.ssim(x.cpu().numpy(), y.cpu().numpy())
    assert abs(got["ssim"] - ref) <= 1e-5
    host = harness.evaluate_image(x.cpu(), y.cpu())
    assert abs(host["ssim"] - ref) <= 1e-5 and abs(host["psnr"] - got["psnr"]) <= 1e-4
