"""SSIM without a GPU: the numpy/scipy restatement (tests/ssim_ref.py) against its stated properties, and `ssim_torch` -- the torch
statement of the same definition, which the GPU tests use as the oracle of the backward -- against the restatement in fp64."""
import numpy as np
import pytest
import torch

import ssim_ref
from shacira_amd.wisp.ops.image import metrics

WEIGHTS = (0.00102838, 0.00759876, 0.03600077, 0.10936069, 0.21300554, 0.26601172)   # from the edge inwards


def pair(h, w, c, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (h, w, c))
    return a, np.clip(a + rng.uniform(-0.1, 0.1, (h, w, c)), 0, 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_is_exactly_one_on_identical_images(dtype):
    a, _ = pair(64, 48, 3)
    value, smap = ssim_ref.ssim(a, a, dtype)
    assert value == 1.0 and np.all(smap == 1.0)


def test_shifted_restatement_is_the_same_definition():
    """`shift=True` subtracts the channel mean before the fields and adds it back to the means: in fp64 the same numbers on every
    input kind of the GPU suite, in fp32 the one of the two that keeps its accuracy on a flat image."""
    from test_gpu_ssim import KINDS, images
    for h, w in ((11, 11), (27, 75)):
        for kind in KINDS:
            x, y = images(kind, h, w, 3)
            value, smap = ssim_ref.ssim(x, y)
            shifted_value, shifted_map = ssim_ref.ssim(x, y, shift=True)
            assert shifted_map.dtype == np.float64 and abs(shifted_value - value) <= 1e-12, kind
            assert np.abs(shifted_map - smap).max() <= 1e-12, kind
    x, y = images("flat", 27, 75, 3)
    _, smap = ssim_ref.ssim(x, y)
    plain = np.abs(ssim_ref.ssim(x, y, np.float32)[1] - smap).max()
    shifted_map = ssim_ref.ssim(x, y, np.float32, shift=True)[1]
    assert shifted_map.dtype == np.float32 and 50 * np.abs(shifted_map - smap).max() < plain
    a, _ = pair(27, 75, 3)
    value, smap = ssim_ref.ssim(a, a, np.float32, shift=True)
    assert value == 1.0 and np.all(smap == 1.0)


def test_preconditions_of_the_tile_centre_cases():
    """tests/test_gpu_ssim_edges.py, B1: every position is the pixel `ssim_stencil_kernel` calls the centre of some tile, the
    fp64 map is finite wherever the GPU test compares it, and the left-out pixels are few."""
    import test_gpu_ssim_edges as edges
    from shacira_amd import _lib
    from test_gpu_ssim import images
    th, tw = _lib.SSIM_TILE_H, _lib.SSIM_TILE_W
    assert len(edges.B1_POSITIONS) == 3 and len(edges.B1_VALUES) == 7
    for position, (h, w, r, c) in edges.B1_POSITIONS.items():
        centres = {(min(r0 + th // 2, h - 1), min(c0 + tw // 2, w - 1)) for r0 in range(0, h, th) for c0 in range(0, w, tw)}
        assert (r, c) in centres, position
        x0, y0 = images("noise02", h, w, 3)
        for which in edges.B1_WHICH:
            for value in edges.B1_VALUES:
                x, y, window, reach = edges.b1_inputs(position, which, value)
                for image, base, touched in ((x, x0, which != "y"), (y, y0, which != "x")):
                    changed = np.argwhere(~((image == base) | (np.isnan(image) & np.isnan(base))))
                    assert changed.tolist() == ([[r, c, edges.B1_CHANNEL]] if touched else []), (position, which, value)
                with np.errstate(all="ignore"):
                    _, smap = ssim_ref.ssim(x, y)
                keep = ~window if edges.b1_excludes(value) else np.ones_like(window)
                assert np.isfinite(smap[keep]).all(), (position, which, value)
                assert window.sum() <= 0.05 * h * w and reach.sum() <= 0.16 * h * w
                assert window[..., edges.B1_CHANNEL].sum() == window.sum() <= 121 and reach.sum() <= 441


def test_window_weights():
    w = ssim_ref.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15
    assert np.abs(w[:6] - np.array(WEIGHTS)).max() <= 1e-8 and np.array_equal(w, w[::-1])
    assert np.abs(metrics.ssim_window().numpy() - w).max() <= 1e-15


def test_images_below_the_window_raise():
    a, b = pair(10, 40, 3)
    with pytest.raises(ValueError):
        ssim_ref.ssim(a, b)
    for h, w in ((10, 40), (40, 10)):
        a, b = (torch.from_numpy(t) for t in pair(h, w, 3))
        with pytest.raises(ValueError):
            metrics.ssim_torch(a, b)
        with pytest.raises(ValueError):
            metrics.ssim(a, b)


@pytest.mark.parametrize("shape", [(11, 11), (12, 75), (40, 11), (64, 48)])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_ssim_torch_fp64_equals_the_restatement(shape, channels):
    a, b = pair(*shape, channels, seed=shape[1] + channels)
    value, smap = ssim_ref.ssim(a[..., :3], b[..., :3])          # a fourth channel is ignored
    got, got_map = metrics.ssim_torch(torch.from_numpy(a), torch.from_numpy(b), full=True)
    assert got.dtype == torch.float64 and got_map.shape == smap.shape
    assert abs(got.item() - value) <= 1e-12
    assert np.abs(got_map.numpy() - smap).max() <= 1e-12
    assert metrics.ssim_torch(torch.from_numpy(a), torch.from_numpy(b)).item() == got.item()


def test_ssim_on_host_tensors_is_ssim_torch():
    a, b = (torch.from_numpy(t).float() for t in pair(40, 33, 3))
    value = metrics.ssim(a, b)
    assert isinstance(value, float) and value == metrics.ssim_torch(a, b).item()
    assert torch.equal(metrics.ssim_map(a, b), metrics.ssim_torch(a, b, full=True)[1])
    assert metrics.ssim(a, a) == 1.0
    with pytest.raises(AssertionError):
        metrics.ssim(a + 2.0, b)                                 # the reference's range asserts


def test_clamped_mse():
    rng = np.random.default_rng(3)
    a, b = rng.uniform(-0.2, 1.2, (17, 9, 3)).astype(np.float32), rng.uniform(0, 1, (17, 9, 3)).astype(np.float32)
    qa = (np.clip(a, 0, 1) * np.float32(255)).astype(np.uint8).astype(np.float32)
    qb = (np.clip(b, 0, 1) * np.float32(255)).astype(np.uint8).astype(np.float32)
    want = float(np.mean((qa - qb) ** 2, dtype=np.float64))
    got = metrics.clamped_mse(torch.from_numpy(a), torch.from_numpy(b))
    assert abs(got - want) <= 1e-6 * want


def test_lpips_is_not_available():
    a = torch.rand(16, 16, 3)
    with pytest.raises(Exception, match="Module lpips not available"):
        metrics.lpips(a, a)


def test_ssim_torch_gradient():
    """The oracle of the kernel's backward has to be right itself: autograd of ssim_torch against finite differences."""
    a, b = (torch.from_numpy(t) for t in pair(13, 12, 1, seed=5))
    a.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: metrics.ssim_torch(t, b), (a,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """shacira_ssim_*: sizes below the window, bad channel counts and NULL operands return SHACIRA_EINVAL, a short workspace
    SHACIRA_EWORKSPACE; validation precedes every HIP call, so this needs no GPU."""
    import ctypes

    from shacira_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)        # never dereferenced
    fwd = lambda h, w, cin, c, x=one, value=one, r=1.0, ws=one, n=1 << 20: L.shacira_ssim_forward(h, w, cin, c, x, one, r, value,
                                                                                                 None, ws, n, None)
    bwd = lambda h, w, cin, c, g=one, n=1 << 20: L.shacira_ssim_backward(h, w, cin, c, one, one, 1.0, g, one, one, n, None)
    for call in (fwd, bwd):
        assert call(10, 16, 3, 3) == _lib.EINVAL and call(16, 10, 3, 3) == _lib.EINVAL
        assert call(16, 16, 3, 0) == _lib.EINVAL and call(16, 16, 3, 4) == _lib.EINVAL
    assert fwd(16, 16, 3, 3, x=None) == _lib.EINVAL and fwd(16, 16, 3, 3, value=None) == _lib.EINVAL
    assert fwd(16, 16, 3, 3, r=0.0) == _lib.EINVAL and fwd(16, 16, 3, 3, r=float("nan")) == _lib.EINVAL
    assert bwd(16, 16, 3, 3, g=None) == _lib.EINVAL
    assert fwd(16, 16, 3, 3, ws=None) == _lib.EWORKSPACE and fwd(16, 16, 3, 3, n=23) == _lib.EWORKSPACE
    assert bwd(16, 16, 3, 3, n=3 * 3 * 256 * 4 - 1) == _lib.EWORKSPACE
    size = L.shacira_ssim_workspace_bytes
    assert size(10, 16, 3, 0) == 0 and size(16, 16, 0, 0) == 0
    assert size(16, 16, 3, 0) == 3 * 8 and size(17, 65, 3, 0) == 3 * 4 * 8 and size(16, 16, 3, 1) == 3 * 3 * 256 * 4
    assert size(32768, 32768, 3, 0) == 3 * 2048 * 512 * 8                 # a gigapixel image is in range
    assert _lib.SSIM_WINDOW == 11 and (_lib.SSIM_TILE_H, _lib.SSIM_TILE_W) == (16, 64)
