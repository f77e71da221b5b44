"""The ray-generation kernel (shacira_amd/csrc/raygen.hip) on the MI355X against the fp64 restatement tests/raygen_ref.py, at the
smallest shapes that cross its edges: a wavefront of 64 and a block of 256 lanes (n = 0, 1, 63 .. 65, 257, 1025), 5x3, 1x1 and
17x9 images, one and three views with the last view and the corner pixels, both lenses, principal-point offsets, fx != fy,
jitter up to +-0.5, the identity and a rotated and translated pose, both index forms, 3 and 4 channels over both backgrounds,
no images, indices out of range, and a side stream.

Every call goes through ``launch``: the raw entry point on outputs pre-filled with a sentinel, so a row the kernel skipped shows.
Bounds (tests/raygen_ref.py): directions within the bound carried through the fp32 sequence, itself asserted below 32 * 2^-24;
pinhole origins the record's bits; orthographic origins within their carried bound; colours and masks bit for bit the fp32 torch
chain. The worst direction error is printed in units of 2^-24 (``pytest -s``) for profiles/raygen.md."""
import ctypes

import numpy as np
import pytest
import torch

import raygen_ref as R
from shacira_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
worst = {"dirs": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def records(V, width, height, lens="pinhole", pose="rotated", offsets=(0.0, 0.0), focal=None):
    """fp32 records [V, K] built without the package's Camera. focal: (fx, fy) in pixels."""
    fx, fy = focal if focal is not None else (1.2 * width, 1.2 * width)
    out = []
    for i in range(V):
        if pose == "identity":
            rot, pos = np.eye(3), np.zeros(3)
        else:
            rot = rotation([0.3 + i, -1.0, 0.5], 0.7 + 1.1 * i)
            pos = np.array([1.5 - i, -2.25 + 0.5 * i, 0.75 * (i + 1)])
        out.append(R.make_record(rot, pos, width / (2 * fx), height / (2 * fy), offsets[0], offsets[1],
                                 1.75 if lens == "ortho" else None, width / height))
    return np.stack(out)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def launch(dev, rec, width, height, view=None, pixel=None, jitter=None, images=None, bg_black=False, n=None, stream=None):
    """The raw entry point on sentinel-filled outputs -> numpy (origins, dirs, rgb, mask); rgb / mask None without images."""
    V = rec.shape[0]
    if view is not None:
        n = len(view)
    elif n is None:
        n = V * width * height
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    rec_d, view_d, pixel_d = t(rec, torch.float32), t(view, torch.int32), t(pixel, torch.int32)
    jit_d, img_d = t(jitter, torch.float32), t(images, torch.uint8)
    origins = torch.full((n, 3), SENTINEL, device=dev)
    dirs = torch.full((n, 3), SENTINEL, device=dev)
    rgb = torch.full((n, 3), SENTINEL, device=dev) if images is not None else None
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev) if images is not None else None
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    rc = _lib.lib().shacira_raygen(_p(rec_d), V, width, height, _p(view_d), _p(pixel_d), _p(jit_d), n, _p(img_d),
                                   images.shape[-1] if images is not None else 4, int(bg_black), _p(origins), _p(dirs), _p(rgb),
                                   _p(mask), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    s.synchronize()
    out = [origins.cpu().numpy(), dirs.cpu().numpy(), None, None]
    assert not (out[0] == SENTINEL).any() and not (out[1] == SENTINEL).any()          # every row written
    if images is not None:
        out[2], out[3] = rgb.cpu().numpy(), mask.cpu().numpy()
        assert not (out[2] == SENTINEL).any() and np.isin(out[3], (0, 1)).all()
    return out


def check(dev, rec, width, height, view=None, pixel=None, jitter=None, images=None, bg_black=False, n=None, stream=None):
    got = launch(dev, rec, width, height, view, pixel, jitter, images, bg_black, n, stream)
    ref = R.raygen_ref(rec, width, height, view, pixel, jitter, images, bg_black, n)
    assert len(ref["valid"]) == got[0].shape[0]                                       # no case dropped
    worst["dirs"] = max(worst["dirs"], R.check_against_ref(ref, *got))
    return got


def draw(V, width, height, n, seed, corners=True):
    rng = np.random.default_rng([seed, V, width, height, n])
    view = rng.integers(0, V, n).astype(np.int32)
    pixel = rng.integers(0, width * height, n).astype(np.int32)
    if corners and n >= 2:                        # the last view's first and last pixel
        view[0], pixel[0] = V - 1, 0
        view[-1], pixel[-1] = V - 1, width * height - 1
    jitter = (rng.random((n, 2)) - 0.5).astype(np.float32)
    jitter[: min(n, 4)] = np.array([[0.5, 0.5], [-0.5, -0.5], [0.5, -0.5], [0.0, 0.0]], np.float32)[: min(n, 4)]
    return view, pixel, jitter


def make_images(V, width, height, channels, seed=0):
    rng = np.random.default_rng([seed, V, width, height, channels])
    img = rng.integers(0, 256, (V, height, width, channels), dtype=np.uint8)
    if channels == 4:                             # alpha: both ends, both sides of 0.5, and anything
        img[..., 3] = rng.choice(np.array([0, 1, 127, 128, 254, 255, 60, 200], np.uint8), (V, height, width))
    return img


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025])
def test_wave_and_block_tails(dev, n):
    rec = records(3, 17, 9)
    view, pixel, jitter = draw(3, 17, 9, n, 1)
    check(dev, rec, 17, 9, view, pixel, jitter, make_images(3, 17, 9, 4))
    print(f"raygen n={n}: worst direction error {worst['dirs']:.2f} U")


@pytest.mark.parametrize("size", [(5, 3), (1, 1), (17, 9)])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("lens", ["pinhole", "ortho"])
def test_sizes_views_lenses(dev, size, V, lens):
    width, height = size
    rec = records(V, width, height, lens, offsets=(0.75, -0.5), focal=(1.3 * width, 0.9 * width))
    view, pixel, jitter = draw(V, width, height, 257, 2)
    check(dev, rec, width, height, view, pixel, jitter, make_images(V, width, height, 4))
    check(dev, rec, width, height, view, pixel, None)                    # no jitter, no images
    print(f"raygen {size} V={V} {lens}: worst direction error {worst['dirs']:.2f} U")


@pytest.mark.parametrize("lens", ["pinhole", "ortho"])
def test_identity_pose(dev, lens):
    rec = records(1, 5, 3, lens, pose="identity")
    origins, dirs, _, _ = check(dev, rec, 5, 3)
    centre = dirs[7]                                                     # pixel (2, 1) of 5x3: straight down -z
    assert np.array_equal(centre, np.array([0.0, 0.0, -1.0], np.float32))
    if lens == "pinhole":
        assert (origins == 0).all() and dirs[0, 0] < 0 < dirs[0, 1]      # top-left pixel: left and up
    else:
        assert (dirs == np.array([0.0, 0.0, -1.0], np.float32)).all() and origins[0, 0] < 0 < origins[0, 1]


@pytest.mark.parametrize("lens", ["pinhole", "ortho"])
def test_whole_view_form_equals_indexed_form(dev, lens):
    V, width, height = 3, 17, 9
    rec, images = records(V, width, height, lens, offsets=(0.4, 0.3)), make_images(V, width, height, 4)
    total = V * width * height
    flat = np.arange(total)
    whole = check(dev, rec, width, height, images=images)
    indexed = check(dev, rec, width, height, (flat // (width * height)).astype(np.int32),
                    (flat % (width * height)).astype(np.int32), None, images)
    for a, b in zip(whole, indexed):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    part = check(dev, rec, width, height, images=images, n=total - 100)  # n < V H W, ending inside the last view
    for a, b in zip(part, whole):
        assert np.array_equal(a, b[: total - 100])
    jitter = draw(V, width, height, total, 3)[2]
    check(dev, rec, width, height, jitter=jitter, images=images, bg_black=True)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("bg_black", [False, True])
def test_channels_and_backgrounds(dev, channels, bg_black):
    V, width, height = 3, 17, 9
    rec = records(V, width, height)
    images = make_images(V, width, height, channels)
    _, _, rgb, mask = check(dev, rec, width, height, images=images, bg_black=bg_black)
    assert mask.all() if channels == 3 else 0 < mask.sum() < mask.size
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0


def test_every_byte_value_composites_exactly(dev):
    """All 256 x 256 (colour, alpha) pairs over both backgrounds: one 256x256 RGBA view."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    images = np.stack([c, 255 - c, c ^ 0x55, a], -1)[None]
    rec = records(1, 256, 256)
    for bg_black in (False, True):
        check(dev, rec, 256, 256, images=images, bg_black=bg_black)


def test_out_of_range_indices_give_nan_rows_and_leave_neighbours_alone(dev):
    V, width, height = 3, 5, 3
    rec, images = records(V, width, height), make_images(V, width, height, 4)
    view, pixel, jitter = draw(V, width, height, 257, 4)
    clean = check(dev, rec, width, height, view, pixel, jitter, images)
    bad_view, bad_pixel = view.copy(), pixel.copy()
    bad = {3: (V, 0), 64: (-1, 0), 65: (0, width * height), 130: (0, -1), 200: (2 ** 31 - 1, 3), 256: (1, -2 ** 31)}
    for row, (v, p) in bad.items():
        bad_view[row], bad_pixel[row] = v, p
    got = check(dev, rec, width, height, bad_view, bad_pixel, jitter, images)
    rows = np.array(sorted(bad))
    keep = np.setdiff1d(np.arange(257), rows)
    for g, c in zip(got, clean):
        assert np.array_equal(g[keep], c[keep])
    assert np.isnan(got[0][rows]).all() and np.isnan(got[1][rows]).all() and np.isnan(got[2][rows]).all()
    assert (got[3][rows] == 0).all()


def test_argument_validation(dev):
    L = _lib.lib()
    EINVAL = _lib.EINVAL
    assert L.shacira_raygen_record_floats() == R.K == _lib.RAYGEN_RECORD_FLOATS
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)      # never dereferenced: validation fails first or n == 0

    def call(cams=one, V=2, W=5, H=3, vi=one, pi=one, jit=None, n=4, img=one, ch=4, bg=0, o=one, d=one, rgb=one, mask=one):
        return L.shacira_raygen(cams, V, W, H, vi, pi, jit, n, img, ch, bg, o, d, rgb, mask, None)

    assert call(n=0) == 0 and call(n=0, o=None, d=None, cams=None) == 0
    for bad in (dict(o=None), dict(d=None), dict(rgb=None), dict(mask=None), dict(cams=None), dict(ch=2), dict(ch=5), dict(ch=1),
                dict(V=0), dict(W=0), dict(H=-1), dict(n=-1), dict(bg=2), dict(vi=None), dict(pi=None),
                dict(vi=None, pi=None, n=31), dict(W=65536, H=32768), dict(cams=odd), dict(jit=odd)):
        assert call(**bad) == EINVAL, bad
    assert call(n=0, ch=2) == EINVAL and call(n=0, W=0) == EINVAL    # the shape is checked before the empty batch returns
    # without images rgb, mask and channels are not looked at; the whole-view form takes exactly V H W rays
    rec = records(2, 5, 3)
    check(dev, rec, 5, 3, n=30)
    with pytest.raises(RuntimeError):
        hip_ops.raygen(torch.zeros(2, 19, device=dev), 5, 3)
    with pytest.raises(RuntimeError):
        hip_ops.raygen(torch.zeros(2, 20, device=dev), 5, 3, torch.zeros(4, dtype=torch.int64, device=dev),
                       torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError):
        hip_ops.raygen(torch.zeros(2, 20, device=dev), 5, 3, num_rays=31)


def test_side_stream_and_wrapper(dev):
    V, width, height = 3, 17, 9
    rec, images = records(V, width, height), make_images(V, width, height, 4)
    view, pixel, jitter = draw(V, width, height, 1025, 6)
    base = check(dev, rec, width, height, view, pixel, jitter, images)
    side = torch.cuda.Stream(dev)
    other = check(dev, rec, width, height, view, pixel, jitter, images, stream=side)
    t = lambda a: torch.from_numpy(a).to(dev)
    with torch.cuda.stream(side):
        o, d, rgb, mask = hip_ops.raygen(t(rec), width, height, t(view), t(pixel), t(jitter), t(images), "white")
    side.synchronize()
    assert mask.dtype == torch.bool and mask.shape == (1025, 1) and o.shape == d.shape == rgb.shape == (1025, 3)
    for a, b, c in zip(base, other, (o, d, rgb, mask.reshape(-1).to(torch.uint8))):
        assert np.array_equal(a, b) and np.array_equal(a, c.cpu().numpy())
    o, d, rgb, mask = hip_ops.raygen(t(rec), width, height)
    assert rgb is None and mask is None and o.shape == (V * width * height, 3)
    o0, d0, rgb0, mask0 = hip_ops.raygen(t(rec), width, height, t(view[:0]), t(pixel[:0]), None, t(images))
    assert o0.shape == (0, 3) and rgb0.shape == (0, 3) and mask0.shape == (0, 1)


@pytest.mark.parametrize("name", ["pinhole_5x3", "pinhole_5x3_offset_fxfy", "pinhole_1x1", "ortho_5x3", "ortho_1x1"])
def test_golden_cases_on_the_device(dev, golden, name):
    """The reference's arithmetic over our camera (tests/golden/make_raygen_golden.py), through the public path: Camera on the
    device -> generate_*_rays with the full centred grid -> the kernel. Tolerance: the records' rounding to fp32 (below 6 U on a
    direction, tests/test_raygen_cpu.py) plus the kernel's carried bound (below 32 U, asserted there)."""
    from shacira_amd.wisp.core import Camera
    from shacira_amd.wisp.ops import raygen as rg
    g = golden("raygen.npz")
    w, h = (int(v) for v in g[f"{name}.size"])
    fx, fy, x0, y0, fd = g[f"{name}.intrinsics"]
    cam = Camera.from_args(view_matrix=torch.from_numpy(g[f"{name}.view_matrix"]), focal_x=fx, focal_y=fy, width=w, height=h,
                           near=0.0, far=6.0, x0=x0, y0=y0, fov_distance=None if np.isnan(fd) else fd).to(dev)
    grid = rg.generate_centered_pixel_coords(w, h, w, h, device=dev)
    rays = (rg.generate_pinhole_rays if np.isnan(fd) else rg.generate_ortho_rays)(cam, grid)
    ref = R.raygen_ref(rg.camera_records(cam).cpu().numpy(), w, h)
    R.check_against_ref(ref, rays.origins.cpu().numpy(), rays.dirs.cpu().numpy())
    assert rays.dist_min == 0.0 and rays.dist_max == 6.0
    assert np.abs(rays.dirs.cpu().numpy() - g[f"{name}.dirs"]).max() <= (6 + 32) * R.U
    assert np.abs(rays.origins.cpu().numpy() - g[f"{name}.origins"]).max() <= 4 * (6 + 32) * R.U
    # a grid without the mark (any operator drops it) takes the composite on the device: the same rays within the same bound
    comp = (rg.generate_pinhole_rays if np.isnan(fd) else rg.generate_ortho_rays)(cam, (grid[0] + 0.0, grid[1] + 0.0))
    assert np.abs(comp.dirs.cpu().numpy() - g[f"{name}.dirs"]).max() <= R.U
