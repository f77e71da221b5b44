"""SSIM on the MI355X, the parts of ssim.hip that tests/test_gpu_ssim.py does not run: a special value on the pixels a tile's
shift is taken from (B1), the accuracy the shift is there for (B2), `data_range` (B3), more partials than the finish kernel has
lanes (B4), constant images (B5). The references and the rules are the sibling's:
  value     |got - ref64| <= max(8 * d32, 16 * 2^-24),  d32 = |ref32 - ref64| of tests/ssim_ref.py run in fp32 and in fp64
  map       the same rule per pixel, d32 the largest per-pixel deviation over the compared pixels
  gradient  test_gpu_ssim.gradient_check against fp64 autograd of metrics.ssim_torch, over the compared pixels
Nothing in a bound is taken from the kernel. Every case prints its error / bound ratio (pytest -s); the largest are recorded in
profiles/ssim.md.

B1. The stencil takes its fields of x - mx, y - my, one shift per (tile, channel). A shift that one pixel decides lets that
pixel's value into the rounding of all 16 x 64 pixels of the tile: when the shift was the tile's centre pixel, 50 there cost
1e-2 of the map, 1e4 0.97, and 1e20 made the tile NaN (profiles/ssim.md). The
cases put 2, +-50, 1e4, 1e20, inf and NaN on a tile's centre pixel (interior, clamped to the last column, clamped to the last
row), in x, in y and in both. Up to 1e4 the whole map and gradient are compared. From 1e20 on the map's non-finite pixels must
be those of the fp32 restatement, and the pixel's 11 x 11 neighbourhood (the gradient: 21 x 21) in its channel is left out of
the comparison. What the restatement itself does there: inf and NaN make exactly the neighbourhood NaN; so does 1e20 in both
images (G xy overflows, inf / inf); 1e20 in one image overflows G xx alone, S = finite / inf = 0, and no pixel is non-finite.
tests/test_ssim_cpu.py checks that the positions are tile centres and that the fp64 map is finite outside the neighbourhood.

B2. `flat` and `offset100` are held to d32 of the restatement with `shift=True` (the channel mean subtracted first), which is
600 (flat) to 200 000 (offset100) times tighter there than the plain one; the ratio plain error / kernel error is printed as the evidence that the
shift works and is no pass condition. ssim_torch cannot express the shifted arithmetic (shifting its inputs changes the
luminance term), so under that bound only value and map are compared; the gradient is held to the sibling's rule, the plain fp32
autograd. `ramp` rises by 40 over the width, so neighbouring tiles shift by very different amounts: its per-pixel map comparison
is the test that no tile seam shows.

B3. `data_range` 255 and 0.5 scale C1 and C2; range 2 with pixels in [-1, 1] also puts the means near zero, where a shift far
from the tile's mean rounds ux = mx + G(x - mx) at the size of mx: with the centre pixel as the shift the map missed its bound
there by 1.3 to 1.6. B4. 1026 tiles: two lanes of the finish kernel take a second partial, and its tree over 1024 sums is
full. B5. Constant images: the variances are exactly zero, S is its luminance term.
"""
import numpy as np
import pytest
import torch

import ssim_ref
from shacira_amd import _lib
from test_gpu_ssim import FLOOR, gradient_check, images, reference_gradients

pytestmark = pytest.mark.gpu
TH, TW = _lib.SSIM_TILE_H, _lib.SSIM_TILE_W
RAD = ssim_ref.RADIUS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _lib.lib()
    return torch.device("cuda:0")


def value_rule(label, got, v64, v32):
    bound = max(8 * abs(v32 - v64), FLOOR)
    err = abs(got - v64)
    print(f"SSIM_EDGE_VALUE {label}: ssim {v64:+.9f} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (label, err, bound)


def map_rule(label, got, m64, m32, keep=None):
    """The sibling's map rule over the pixels of `keep` (all by default); returns the largest error."""
    keep = np.ones(m64.shape, bool) if keep is None else keep
    assert np.isfinite(m64[keep]).all() and np.isfinite(m32[keep]).all(), label
    with np.errstate(invalid="ignore"):
        bound = max(8 * float(np.abs(m32.astype(np.float64) - m64)[keep].max()), FLOOR)
        diff = np.where(keep, np.abs(got.astype(np.float64) - m64), 0.0)
    err = float(np.nan_to_num(diff, nan=np.inf).max())
    print(f"SSIM_EDGE_MAP {label}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (label, err, bound, np.unravel_index(np.nan_to_num(diff, nan=np.inf).argmax(), diff.shape))
    return err


def forward(dev, x, y, data_range=1.0):
    """The kernel's (value, map) as a float and an array; the value without the map must be the same bits."""
    from shacira_amd import hip_ops
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    value, smap = hip_ops.ssim_forward(xd, yd, data_range=data_range, with_map=True)
    only, none = hip_ops.ssim_forward(xd, yd, data_range=data_range)
    assert none is None and value.dtype == torch.float64 and tuple(smap.shape) == x.shape
    assert torch.equal(value.view(torch.int64), only.view(torch.int64))
    return value.item(), smap.cpu().numpy()


def backward(dev, x, y, data_range=1.0):
    from shacira_amd import hip_ops
    g = hip_ops.ssim_backward(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), 1.0, data_range=data_range)
    assert g.dtype == torch.float32 and tuple(g.shape) == x.shape
    return g.double().cpu().numpy()


# ---- B1: a special value at a tile centre ----------------------------------------------------------------------------------------
B1_CHANNEL = 1
B1_POSITIONS = {                                    # name: (H, W, row, column)
    "interior": (48, 80, TH + TH // 2, TW // 2),
    "last_column": (48, 80, TH + TH // 2, 80 - 1),
    "last_row": (40, 70, 40 - 1, TW // 2),
}
B1_WHICH = ("x", "y", "both")
B1_VALUES = (2.0, -50.0, 50.0, 1e4, 1e20, float("inf"), float("nan"))


def b1_excludes(value):
    """From 1e20 on (inf and NaN with it) the pixel's neighbourhood is not compared."""
    return not abs(value) < 1e20


def b1_inputs(position, which, value):
    """(x, y, window, reach): noise02 with `value` on the position in channel 1 of x, y or both; `window` marks the pixel's 11 x 11
    neighbourhood in that channel (what its value reaches in the map), `reach` the 21 x 21 one (in the gradient)."""
    h, w, r, c = B1_POSITIONS[position]
    x, y = images("noise02", h, w, 3)
    if which in ("x", "both"):
        x[r, c, B1_CHANNEL] = value
    if which in ("y", "both"):
        y[r, c, B1_CHANNEL] = value
    window, reach = np.zeros((h, w, 3), bool), np.zeros((h, w, 3), bool)
    window[max(r - RAD, 0):r + RAD + 1, max(c - RAD, 0):c + RAD + 1, B1_CHANNEL] = True
    reach[max(r - 2 * RAD, 0):r + 2 * RAD + 1, max(c - 2 * RAD, 0):c + 2 * RAD + 1, B1_CHANNEL] = True
    return x, y, window, reach


@pytest.mark.parametrize("value", B1_VALUES)
@pytest.mark.parametrize("which", B1_WHICH)
@pytest.mark.parametrize("position", list(B1_POSITIONS))
def test_a_special_value_at_a_tile_centre_forward(dev, position, which, value):
    x, y, window, _ = b1_inputs(position, which, value)
    label = f"B1 {position} {which} {value:g}"
    with np.errstate(all="ignore"):
        v64, m64 = ssim_ref.ssim(x, y, np.float64)
        v32, m32 = ssim_ref.ssim(x, y, np.float32)
    got_value, got_map = forward(dev, x, y)
    if not b1_excludes(value):
        map_rule(label, got_map, m64, m32)
        value_rule(label, got_value, v64, v32)
        return
    # the restatement alone first: inf, NaN and an overflowing G xy spoil exactly the neighbourhood, an overflowing G xx nothing
    spoilt = window if (not np.isfinite(value) or which == "both") else np.zeros_like(window)
    assert np.array_equal(~np.isfinite(m32), spoilt), label
    assert np.array_equal(~np.isfinite(got_map), ~np.isfinite(m32)), (label, int((~np.isfinite(got_map)).sum()))
    assert window.sum() <= 0.05 * window.shape[0] * window.shape[1]
    map_rule(label, got_map, m64, m32, keep=~window)
    if np.isfinite(v32):
        value_rule(label, got_value, v64, v32)
    else:
        assert np.isnan(got_value), label


@pytest.mark.parametrize("value", B1_VALUES)
@pytest.mark.parametrize("which", B1_WHICH)
@pytest.mark.parametrize("position", list(B1_POSITIONS))
def test_a_special_value_at_a_tile_centre_backward(dev, position, which, value):
    x, y, _, reach = b1_inputs(position, which, value)
    label = f"B1 {position} {which} {value:g}"
    g64, g32 = reference_gradients(x, y, 3)
    g = backward(dev, x, y)
    keep = np.ones(reach.shape, bool)
    if b1_excludes(value):
        keep = ~reach
        assert reach.sum() <= 0.16 * reach.shape[0] * reach.shape[1]
    assert np.isfinite(g64[keep]).all() and np.isfinite(g32[keep]).all(), label
    gradient_check(label, g[keep], g64[keep], g32[keep])
    others = [ch for ch in range(3) if ch != B1_CHANNEL]
    gradient_check(label + " other channels", g[..., others], g64[..., others], g32[..., others])


# ---- B2: what the shift is for -----------------------------------------------------------------------------------------------------
B2_SHAPES = [(TH + 11, TW + 11), (2 * TH + 11, 2 * TW + 11)]


def b2_images(kind, h, w):
    if kind == "flat":
        return images("flat", h, w, 3)
    if kind == "offset100":
        x, y = images("noise002", h, w, 3)
        return (x.astype(np.float64) + 100.0).astype(np.float32), (y.astype(np.float64) + 100.0).astype(np.float32)
    rng = np.random.default_rng([2, h, w])
    n1, n2 = rng.uniform(0, 1, (h, w, 3)), rng.uniform(-1, 1, (h, w, 3))
    x = 40.0 * np.arange(w)[None, :, None] / w + 0.2 * n1
    return x.astype(np.float32), (x + 0.02 * n2).astype(np.float32)


@pytest.mark.parametrize("h,w", B2_SHAPES)
@pytest.mark.parametrize("kind", ["flat", "offset100"])
def test_flat_and_offset_images_to_the_shifted_fp32_error(dev, kind, h, w):
    x, y = b2_images(kind, h, w)
    label = f"B2 {kind} {h}x{w}"
    v64, m64 = ssim_ref.ssim(x, y, np.float64)
    v32, m32 = ssim_ref.ssim(x, y, np.float32, shift=True)
    plain_value, plain_map = ssim_ref.ssim(x, y, np.float32)
    got_value, got_map = forward(dev, x, y)
    err = map_rule(label, got_map, m64, m32)
    value_rule(label, got_value, v64, v32)
    plain = float(np.abs(plain_map.astype(np.float64) - m64).max())
    print(f"SSIM_EDGE_SHIFT {label}: map error plain fp32 {plain:.3e} kernel {err:.3e} plain / kernel {plain / max(err, 1e-300):.1f}; "
          f"value error plain fp32 {abs(plain_value - v64):.3e} kernel {abs(got_value - v64):.3e}")
    g64, g32 = reference_gradients(x, y, 3)
    gradient_check(label, backward(dev, x, y), g64, g32)


@pytest.mark.parametrize("h,w", B2_SHAPES)
def test_a_ramp_shows_no_tile_seam(dev, h, w):
    x, y = b2_images("ramp", h, w)
    label = f"B2 ramp {h}x{w}"
    v64, m64 = ssim_ref.ssim(x, y, np.float64)
    v32, m32 = ssim_ref.ssim(x, y, np.float32)
    got_value, got_map = forward(dev, x, y)
    map_rule(label, got_map, m64, m32)
    value_rule(label, got_value, v64, v32)
    g64, g32 = reference_gradients(x, y, 3)
    gradient_check(label, backward(dev, x, y), g64, g32)


# ---- B3: data_range ----------------------------------------------------------------------------------------------------------------
def b3_images(case, h, w):
    """(x, y, data_range)"""
    kind, scale = case.split("/")
    x, y = (t.astype(np.float64) for t in images(kind, h, w, 3))
    if scale == "255":
        return (255.0 * x).astype(np.float32), (255.0 * y).astype(np.float32), 255.0
    if scale == "signed":
        return (2.0 * x - 1.0).astype(np.float32), (2.0 * y - 1.0).astype(np.float32), 2.0
    return x.astype(np.float32), y.astype(np.float32), 0.5


@pytest.mark.parametrize("h,w", [(11, 11), (TH + 11, TW + 11)])
@pytest.mark.parametrize("case", ["noise02/255", "inverted/255", "noise02/signed", "inverted/signed", "noise02/half"])
def test_data_range(dev, case, h, w):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.image import metrics
    x, y, R = b3_images(case, h, w)
    label = f"B3 {case} R={R:g} {h}x{w}"
    if case.endswith("signed"):
        assert x.min() < 0 and y.min() < 0
    if case == "inverted/signed":
        assert np.abs(x + y).max() <= 2.0 ** -22        # y == -x to rounding: ux * uy = -ux^2, negative wherever it counts
    v64, m64 = ssim_ref.ssim(x, y, np.float64, data_range=R)
    v32, m32 = ssim_ref.ssim(x, y, np.float32, data_range=R)
    got_value, got_map = forward(dev, x, y, data_range=R)
    map_rule(label, got_map, m64, m32)
    value_rule(label, got_value, v64, v32)
    if case == "inverted/255":
        assert got_value < 0
    g64, g32 = reference_gradients(x, y, 3, data_range=R)
    gradient_check(label, backward(dev, x, y, data_range=R), g64, g32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    pred = xd.clone().requires_grad_(True)
    loss = metrics.ssim_loss(pred, yd, data_range=R)
    loss.backward()
    assert loss.item() == np.float32(1.0 - got_value)
    want = hip_ops.ssim_backward(xd, yd, -1.0, data_range=R)
    assert torch.equal(pred.grad.view(torch.int32), want.view(torch.int32))


# ---- B4: more than 1024 tiles ------------------------------------------------------------------------------------------------------
def b4_images(h, w, c):
    x, y = images("noise02", h, w, c)
    if h > w:
        y[h // 2:] *= np.float32(0.9)
    else:
        y[:, w // 2:] *= np.float32(0.9)
    return x, y


@pytest.mark.parametrize("h,w,c", [(1025 * TH + 5, 11, 3), (11, 1025 * TW + 5, 1)])
def test_more_partials_than_the_finish_kernel_has_lanes(dev, h, w, c):
    from shacira_amd import hip_ops
    assert _lib.lib().shacira_ssim_workspace_bytes(h, w, c, 0) == c * 1026 * 8          # 1026 tiles: two lanes take a second turn
    x, y = b4_images(h, w, c)
    label = f"B4 {h}x{w}x{c}"
    v64, _ = ssim_ref.ssim(x, y, np.float64)
    v32, _ = ssim_ref.ssim(x, y, np.float32)
    got_value, got_map = forward(dev, x, y)             # asserts the same bits with and without the map
    value_rule(label, got_value, v64, v32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    hip_ops.ssim_forward(yd, xd)                        # other work through the same workspace in between
    again, again_map = hip_ops.ssim_forward(xd, yd, with_map=True)
    assert np.float64(got_value).tobytes() == np.float64(again.item()).tobytes()
    assert np.array_equal(got_map.view(np.int32), again_map.cpu().numpy().view(np.int32))
    if h > w:
        g64, g32 = reference_gradients(x, y, c)
        gradient_check(label, backward(dev, x, y), g64, g32)


# ---- B5: constant images -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(0.0, 0.0), (0.5, 0.5), (0.25, 0.75), (0.0, 1.0)])
def test_constant_images(dev, a, b):
    h, w = TH + 11, TW + 11
    x, y = np.full((h, w, 3), a, np.float32), np.full((h, w, 3), b, np.float32)
    label = f"B5 x == {a:g} y == {b:g}"
    c1 = 0.01 ** 2
    want = np.full((h, w, 3), (2 * a * b + c1) / (a * a + b * b + c1), np.float64)
    v32, m32 = ssim_ref.ssim(x, y, np.float32)
    got_value, got_map = forward(dev, x, y)
    map_rule(label, got_map, want, m32)
    value_rule(label, got_value, float(want[0, 0, 0]), v32)
    if a == b:
        assert got_value == 1.0 and bool((got_map == 1.0).all())
    g64, g32 = reference_gradients(x, y, 3)
    gradient_check(label, backward(dev, x, y), g64, g32)
