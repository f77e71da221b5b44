"""The offline renderer's host side (no GPU): the fp64 restatement tests/shade_ref.py and the torch host paths against the outputs
the reference's own functions gave (tests/golden/shade.npz, recorded by tests/golden/make_shade_golden.py), the blur against
scipy, the ``RenderBuffer`` / ``Rays`` additions, ``OfflineRenderer`` on host tensors with an analytic sphere as tracer, and the
validation codes of the four entry points of shade.hip."""
import ctypes
import os

import numpy as np
import pytest
import torch

import shade_ref as R
from shacira_amd import _lib, hip_ops
from shacira_amd.wisp.core import Rays, RenderBuffer
from shacira_amd.wisp.models.pipeline import Pipeline
from shacira_amd.wisp.offline_renderer import OfflineRenderer, sdf_slice_colors_torch
from shacira_amd.wisp.ops.geometric import (look_at_rays, normalized_grid, normalized_slice, spherical_envmap,
                                            spherical_envmap_torch)
from shacira_amd.wisp.ops.image import linear_to_srgb, srgb_to_linear
from shacira_amd.wisp.ops.shaders import (default_matcap, gaussian_blur_torch, matcap_sampler, matcap_shader,
                                          pointlight_shadow_shader, sample_matcap_torch)

F = np.float32
U = 2.0 ** -24
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade.npz"))


# ---- the restatement and the host paths against the reference's outputs ----------------------------------------------------------
def test_shade_ref_envmap_and_matcap_equal_the_reference():
    normal, dirs = GOLDEN["envmap_normal"], GOLDEN["envmap_dirs"]
    uv, m = R.envmap(dirs, normal)
    gold = GOLDEN["envmap_uv"].astype(np.float64)
    # the reference computes in fp32: our fp64 coordinates are within its rounding, (82 / m + 2.5) u of the derivation in
    # tests/test_gpu_shade.py without the rotation; degenerate rows (m = 0 or NaN) are exact zeros on both sides
    fine = np.isfinite(m) & (m > 0)
    assert (np.abs(uv[fine] - gold[fine]).max(axis=1) <= (82 / m[fine] + 2.5) * U).all()
    assert np.array_equal(uv[~fine], gold[~fine]) and not uv[~fine].any() and (~fine).sum() == 3
    # exact rows
    assert uv[5, 0] == 0.0 and uv[5, 1] == 0.5 and uv[6, 0] == 1.0 and uv[7, 1] == 1.0
    # the sampler at the reference's own coordinates: scipy's interpolator in fp64, then float32 and / 255
    tex = GOLDEN["matcap_tex"]
    want = R.sample_matcap(tex, gold)
    assert np.abs(want - GOLDEN["matcap_rgb_nomm"]).max() <= 2 * U
    # and end to end with the rotation: the coordinates differ by the fp32 rounding of the reference, times the texture's slope
    t = tex[..., :3].astype(np.int64)
    step = max(np.abs(np.diff(t, axis=0)).max(), np.abs(np.diff(t, axis=1)).max())
    mm = GOLDEN["matcap_mm"]
    ours = R.shade_view(R.MATCAP, normal, dirs, mm=mm, tex=tex)
    ok = np.isfinite(ours["m"]) & (ours["m"] >= 0.25)
    bound = 2 * U + 2 * (128 * U / ours["m"][ok]) * 6 * step / 255.0
    assert (np.abs(ours["rgb"][ok] - GOLDEN["matcap_rgb_mm"][ok]).max(axis=1) <= bound).all()


def test_shade_ref_slice_colours_equal_the_reference():
    d = GOLDEN["sdf_slice_d"]
    w, h = GOLDEN["sdf_slice_res"]
    gold = GOLDEN["sdf_slice_vis"].reshape(-1, 3)
    vis, cls = R.sdf_slice_colors(d)
    fixed = {R.SLICE_INSIDE: (1.0, 0.38, 0.0), R.SLICE_LINE: (0.8, 0.8, 0.8), R.SLICE_ZERO: (0.0, 0.0, 0.0)}
    gold_cls = np.full(d.shape[0], R.SLICE_BASE)
    gold_cls[np.isnan(gold).any(axis=1)] = R.SLICE_NAN
    for c, colour in fixed.items():
        gold_cls[(gold == np.array(colour)).all(axis=1)] = c
    assert np.array_equal(cls, gold_cls)                                     # the classes: bit for bit
    assert {R.SLICE_BASE, R.SLICE_INSIDE, R.SLICE_LINE, R.SLICE_NAN} <= set(cls.tolist())
    for c, colour in fixed.items():
        assert np.array_equal(vis[cls == c], np.tile(np.array(colour, dtype=F), (int((cls == c).sum()), 1)))
    base = cls == R.SLICE_BASE
    assert np.abs(vis[base].astype(np.float64) - gold[base]).max() <= 2.0 ** -22     # the reference accumulates in double
    host = sdf_slice_colors_torch(torch.from_numpy(d)).numpy()
    assert np.array_equal(host[cls != R.SLICE_NAN].view(np.uint32), vis[cls != R.SLICE_NAN].view(np.uint32))
    assert np.isnan(host[cls == R.SLICE_NAN]).all()
    renderer = OfflineRenderer(render_res=[int(w), int(h)], device="cpu")
    out = renderer.sdf_slice(lambda pts: torch.from_numpy(d).reshape(-1, 1))
    assert tuple(out.shape) == (w, h, 3) and np.array_equal(out.reshape(-1, 3).numpy(), host, equal_nan=True)


def test_host_grids_and_look_at_rays_equal_the_reference():
    for h, w in ((5, 3), (3, 5), (4, 4), (1, 1)):
        assert np.abs(normalized_grid(h, w, device="cpu").numpy() - GOLDEN[f"grid_{h}x{w}"]).max() <= 2 * U * 2
        got = normalized_grid(h, w, device="cpu", use_aspect=False).numpy()
        assert got.shape == (h, w, 2) and np.abs(got - GOLDEN[f"grid_{h}x{w}_noaspect"]).max() <= 2 * U
    for dim in range(3):
        got = normalized_slice(3, 5, dim=dim, depth=0.25, device="cpu").numpy()
        assert got.shape == (3, 5, 3) and np.abs(got - GOLDEN[f"slice_dim{dim}"]).max() <= 4 * U
    assert (normalized_slice(3, 5, dim=1, depth=0.25, device="cpu")[..., 1] == -0.25).all()        # the reference's y *= -1
    with pytest.raises(ValueError):
        normalized_slice(3, 5, dim=3, device="cpu")
    jit = normalized_grid(4, 6, jitter=True, device="cpu", use_aspect=False)
    plain = normalized_grid(4, 6, device="cpu", use_aspect=False)
    assert (jit - plain)[..., 0].abs().max() <= 1 / 6 + 1e-6 and (jit - plain)[..., 1].abs().max() <= 1 / 4 + 1e-6
    assert not torch.equal(jit, plain)
    for mode in ("persp", "ortho"):
        o, d = look_at_rays([1.5, 1.2, 2.0], [0.1, -0.2, 0.0], 5, 3, mode=mode, fov=40.0, device="cpu")
        assert tuple(o.shape) == (15, 3) and tuple(d.shape) == (15, 3)
        # origins up to |o| <= 4, directions unit: a few units of 2^-24 each
        assert np.abs(o.numpy() - GOLDEN[f"lookat_{mode}_origins"]).max() <= 8 * U * 4
        assert np.abs(d.numpy() - GOLDEN[f"lookat_{mode}_dirs"]).max() <= 8 * U
    with pytest.raises(ValueError):
        look_at_rays([0, 0, 1], [0, 0, 0], 2, 2, mode="fisheye", device="cpu")


def test_host_envmap_matcap_and_srgb_equal_the_reference(tmp_path):
    normal, dirs = torch.from_numpy(GOLDEN["envmap_normal"]), torch.from_numpy(GOLDEN["envmap_dirs"])
    keep = normal.clone()
    uv = spherical_envmap(dirs, normal)
    assert torch.equal(uv, spherical_envmap_torch(dirs, normal)) and tuple(uv.shape) == (64, 2)
    assert np.array_equal(uv.numpy(), GOLDEN["envmap_uv"])               # the same torch operators: the same bits
    assert torch.equal(normal.nan_to_num(7.0), keep.nan_to_num(7.0))     # the inputs are not modified
    tex = torch.from_numpy(GOLDEN["matcap_tex"])
    import PIL.Image
    path = str(tmp_path / "matcap.png")
    PIL.Image.fromarray(GOLDEN["matcap_tex"], "RGBA").save(path)
    assert torch.equal(matcap_sampler(path), tex) and matcap_sampler(path) is matcap_sampler(path)
    with pytest.raises(Exception, match="does not exist"):
        matcap_sampler(str(tmp_path / "nope.png"))
    for name, mm in (("nomm", None), ("mm", torch.from_numpy(GOLDEN["matcap_mm"]))):
        for source in (path, tex):
            rb = matcap_shader(RenderBuffer(normal=normal.clone()), Rays(torch.zeros(64, 3), dirs.clone()), source, mm=mm)
            assert tuple(rb.rgb.shape) == (64, 3) and rb.rgb.dtype == torch.float32
            assert np.abs(rb.rgb.numpy() - GOLDEN[f"matcap_rgb_{name}"]).max() <= 4 * U
    with pytest.raises(ValueError):
        sample_matcap_torch(torch.zeros(1, 5, 3, dtype=torch.uint8), uv)
    lin = torch.from_numpy(GOLDEN["srgb_in"])
    assert np.abs(linear_to_srgb(lin.clone()).numpy() - GOLDEN["srgb_out"]).max() <= 4 * U
    x = torch.linspace(0.0, 1.0, 41)
    assert (srgb_to_linear(linear_to_srgb(x.clone())) - x).abs().max() <= 1e-6
    assert srgb_to_linear(torch.tensor([0.04045]))[0] == torch.tensor(0.04045) / 12.92


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 9)])
def test_blur_restatements_equal_scipy(shape):
    from scipy.ndimage import gaussian_filter
    a = np.random.default_rng(shape[0]).random(shape)
    want = gaussian_filter(a, sigma=2)
    assert np.abs(R.gaussian_blur(a) - want).max() <= 4e-16
    assert np.abs(gaussian_blur_torch(torch.from_numpy(a)).numpy() - want).max() <= 4e-16
    assert np.abs(R.blur_taps().sum() - 1.0) <= 1e-15 and R.blur_taps().shape == (17,)


def test_shadow_jitter_host_restatement_is_the_oracles():
    from shacira_amd.wisp.ops.shaders.shadow_rays import _shadow_gaussians
    for seed in (0, 5, (1 << 40) + 5):
        assert np.abs(_shadow_gaussians(300, seed).numpy() - R.shadow_gaussians(300, seed)).max() <= 4 * U * 6
    assert not np.array_equal(R.shadow_gaussians(8, 5), R.shadow_gaussians(8, (1 << 40) + 5))
    # a stream of its own: not the words of a dataset's sample with the same seed
    import mesh_sample_ref as msr
    mesh = msr.gaussians64(msr.sample_words(8, 5))
    assert not np.isclose(R.shadow_gaussians(8, 5), mesh).any()


# ---- RenderBuffer and Rays ---------------------------------------------------------------------------------------------------------
def test_render_buffer_image_equals_the_reference():
    chans = {k: torch.from_numpy(GOLDEN[f"image_in_{k}"]) for k in ("rgb", "alpha", "depth", "hit", "normal")}
    img = RenderBuffer(**chans).image()
    for k in chans:
        assert np.abs(getattr(img, k).numpy() - GOLDEN[f"image_out_{k}"]).max() <= 255 * 2 * U, k
        assert np.array_equal(getattr(img.byte(), k).numpy(), GOLDEN[f"image_byte_{k}"]), k
    bare = RenderBuffer(rgb=chans["rgb"]).image()
    assert bare.hit is None and bare.normal is None and bare.depth is None and "hit" in bare.channels


def test_render_buffer_channels_cat_mean_reshape_transpose():
    a = RenderBuffer(rgb=torch.ones(4, 3), depth=torch.zeros(4, 1), hit=torch.tensor([True, False, True, True]),
                     normal=torch.zeros(4, 3))
    b = RenderBuffer(rgb=torch.zeros(2, 3), depth=torch.ones(2, 1), hit=torch.tensor([[False], [True]]), err=torch.ones(2, 1))
    assert a.xyz is None and a.shadow is None and a.ao is None and a.dirs is None
    assert a.channels == {"rgb", "alpha", "depth", "hit", "normal"} and dict(iter(a))["alpha"] is None
    c = a + b
    assert tuple(c.rgb.shape) == (6, 3) and tuple(c.hit.shape) == (6, 1) and c.alpha is None       # [N] meets [N, 1]
    assert torch.equal(c.normal, a.normal) and torch.equal(c.err, b.err)                               # None absorbs
    empty = RenderBuffer(xyz=None, hit=None, normal=None, shadow=None, ao=None, dirs=None)
    d = empty + a
    assert torch.equal(d.rgb, a.rgb) and torch.equal(d.hit, a.hit) and d.xyz is None and "shadow" in d.channels
    side = RenderBuffer(rgb=torch.ones(4, 3), depth=torch.zeros(4, 1))
    assert torch.equal(side.cat(side, dim=1).rgb, torch.ones(4, 6)) and tuple(side.cat(side, dim=1).depth.shape) == (4, 2)
    m = RenderBuffer.mean(a, RenderBuffer(rgb=torch.zeros(4, 3), depth=torch.ones(4, 1)), RenderBuffer(rgb=torch.ones(4, 3)))
    assert torch.allclose(m.rgb, torch.full((4, 3), 2 / 3)) and torch.allclose(m.depth, torch.full((4, 1), 1 / 3))
    assert m.alpha is None
    r = a.reshape(2, 2, -1)
    assert tuple(r.rgb.shape) == (2, 2, 3) and tuple(r.hit.shape) == (2, 2, 1) and r.alpha is None
    wide = RenderBuffer(rgb=torch.arange(18.0).reshape(2, 3, 3)).transpose()
    assert tuple(wide.rgb.shape) == (3, 2, 3) and wide.rgb[2, 1, 0] == 15.0
    assert a.byte().rgb.dtype == torch.uint8 and a.float().hit.dtype == torch.float32
    assert a.to(torch.float64).rgb.dtype == torch.float64 and a.cpu().detach().rgb.device.type == "cpu"
    assert set(a.numpy_dict()) == {"rgb", "depth", "hit", "normal"} and a.numpy_dict()["rgb"].shape == (4, 3)
    assert tuple(RenderBuffer(rgb=torch.ones(2, 3), alpha=torch.ones(2, 1)).rgba.shape) == (2, 4) and a.rgba is None


def test_rays_split_with_a_remainder_and_reshape():
    rays = Rays(torch.arange(30.0).reshape(10, 3), torch.ones(10, 3), dist_min=0.5, dist_max=7.0)
    packs = rays.split(4)
    assert [len(p) for p in packs] == [4, 4, 2] and all(p.dist_min == 0.5 and p.dist_max == 7.0 for p in packs)
    assert torch.equal(torch.cat([p.origins for p in packs]), rays.origins)
    img = rays.reshape(2, 5, 3)
    assert tuple(img.origins.shape) == (2, 5, 3) and tuple(img.shape) == (2, 5) and img.dist_max == 7.0


# ---- OfflineRenderer on host tensors ---------------------------------------------------------------------------------------------
RADIUS = 0.7


class SphereTracer:
    """The analytic intersection of every ray with the sphere |x| = 0.7: per-ray arithmetic only, so batches cannot differ."""

    def __init__(self):
        self.calls = []

    def __call__(self, nef, rays=None, lod_idx=None, **kwargs):
        self.calls.append((rays.origins.shape[0], lod_idx, kwargs))
        o, d = rays.origins, rays.dirs
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - RADIUS * RADIUS)
        t = -b - torch.sqrt(torch.clamp(disc, min=0.0))
        hit = (disc > 0) & (t > rays.dist_min) & (t < rays.dist_max)
        xyz = torch.where(hit[:, None], o + d * t[:, None], torch.zeros_like(o))
        normal = torch.where(hit[:, None], xyz / RADIUS, torch.zeros_like(o))
        return RenderBuffer(xyz=xyz, depth=torch.where(hit, t, torch.zeros_like(t))[:, None], hit=hit, normal=normal,
                            rgb=(normal + 1.0) / 2.0, alpha=hit[:, None].float())


W, H = 12, 10


@pytest.fixture(scope="module")
def host_view():
    o, d = look_at_rays([1.5, 1.2, 2.0], [0, 0, 0], H, W, fov=40.0, device="cpu")
    return Pipeline(None, SphereTracer()), Rays(o, d, dist_min=0, dist_max=10)


@pytest.mark.parametrize("mode", ["rb", "normal", "matcap"])
def test_host_renderer_modes_batches_and_segmentation(host_view, mode):
    pipeline, rays = host_view
    whole = OfflineRenderer(render_res=[W, H], shading_mode=mode, device="cpu").render(pipeline, rays)
    batched = OfflineRenderer(render_res=[W, H], shading_mode=mode, render_batch=50, device="cpu", num_steps=3)
    pipeline.tracer.calls.clear()
    parts = batched.render(pipeline, rays, lod_idx=2)
    assert [c[0] for c in pipeline.tracer.calls] == [50, 50, 20]                      # 120 rays: a remainder
    assert all(c[1] == 2 and c[2] == {"num_steps": 3} for c in pipeline.tracer.calls)  # lod_idx and the tracer keywords
    for name in ("rgb", "normal", "hit", "xyz", "depth", "alpha"):
        assert torch.equal(getattr(whole, name).reshape(W * H, -1), getattr(parts, name).reshape(W * H, -1)), name
    traced = pipeline.tracer(None, rays=rays)
    hit = traced.hit.numpy()
    assert 0.1 < hit.mean() < 0.9
    want = R.shade_view({"rb": R.RB, "normal": R.NORMAL, "matcap": R.MATCAP}[mode], traced.normal.numpy(), rays.dirs.numpy(),
                        hit=hit, tex=default_matcap().numpy(), rgb=traced.rgb.numpy())
    assert (whole.rgb.numpy()[~hit] == 1.0).all() and (whole.normal.numpy()[~hit] == 1.0).all()      # segmentation
    assert torch.equal(whole.normal[traced.hit], traced.normal[traced.hit])
    tol = 2e-4 if mode == "matcap" else 4 * U            # matcap: fp32 coordinates times the texture's slope
    assert np.abs(whole.rgb.numpy() - want["rgb"]).max() <= tol
    assert not torch.equal(traced.normal, whole.normal) and (traced.normal[~traced.hit] == 0).all()    # the tracer's own stay


def test_host_renderer_lookat_aa_and_matcap_sources(host_view, tmp_path):
    pipeline, rays = host_view
    r = OfflineRenderer(render_res=[W, H], shading_mode="normal", device="cpu")
    rb = r.render_lookat(pipeline, f=[1.5, 1.2, 2.0], t=[0, 0, 0], fov=40.0, camera_clamp=[0, 10])
    assert tuple(rb.rgb.shape) == (H, W, 3) and tuple(rb.hit.shape) == (H, W, 1) and tuple(rb.depth.shape) == (H, W, 1)
    flat = r.render(pipeline, rays)
    assert torch.equal(rb.rgb.reshape(-1, 3), flat.rgb)
    one = r.shade_images(pipeline, f=[1.5, 1.2, 2.0], fov=40.0)
    two = r.shade_images(pipeline, f=[1.5, 1.2, 2.0], fov=40.0, aa=2)
    assert tuple(one.rgb.shape) == (W, H, 3) and tuple(two.rgb.shape) == (W, H, 3)                   # transposed
    assert torch.allclose(one.rgb, two.rgb, atol=1e-6) and torch.equal(one.rgb, rb.rgb.permute(1, 0, 2))
    assert two.hit.dtype == torch.float32                                                              # a mean, not a mask
    ortho = r.render_lookat(pipeline, f=[0, 0, 2.0], fov=40.0, camera_proj="ortho", camera_clamp=[0, 10])
    assert ortho.hit.any() and not torch.equal(ortho.hit, rb.hit)
    tex = torch.from_numpy(GOLDEN["matcap_tex"])
    import PIL.Image
    path = str(tmp_path / "m.png")
    PIL.Image.fromarray(GOLDEN["matcap_tex"], "RGBA").save(path)
    a = OfflineRenderer(render_res=[W, H], shading_mode="matcap", matcap_path=path, device="cpu").render(pipeline, rays)
    b = OfflineRenderer(render_res=[W, H], shading_mode="matcap", matcap_path=tex, device="cpu").render(pipeline, rays)
    assert torch.equal(a.rgb, b.rgb) and a.rgb[a.hit].std() > 0.05


def test_host_renderer_refusals_and_shadows(host_view):
    pipeline, rays = host_view
    with pytest.raises(NotImplementedError, match="Ambient occlusion"):
        OfflineRenderer(render_res=[W, H], ao=True, device="cpu")
    with pytest.raises(NotImplementedError):
        OfflineRenderer(render_res=[W, H], shading_mode="phong", device="cpu")
    shadowed = OfflineRenderer(render_res=[W, H], shading_mode="normal", shadow=True, seed=3, device="cpu")
    with pytest.raises(ValueError, match="height \\* width"):
        shadowed.render(pipeline, rays[:50])
    with pytest.raises(ValueError, match="height \\* width"):
        pointlight_shadow_shader(RenderBuffer(), rays, pipeline)
    shadowed.min_y = 0.1
    plain = OfflineRenderer(render_res=[W, H], shading_mode="normal", device="cpu").render(pipeline, rays)
    rb = shadowed.render(pipeline, rays)
    again = shadowed.render(pipeline, rays)
    assert torch.equal(rb.rgb, again.rgb) and rb.shadow.dtype == torch.bool and tuple(rb.shadow.shape) == (W * H,)
    taken = plain.hit & ~rb.hit
    assert taken.any() and (rb.normal[taken] == torch.tensor([0.0, 1.0, 0.0])).all() and (rb.xyz[taken, 1] - 0.1).abs().max() < 1e-5
    want = R.shadow_apply(H, W, rb.shadow.numpy(), np.ones(W * H, bool), plain.rgb.numpy())
    assert np.abs(rb.rgb.numpy() - want["rgb"]).max() <= 40 * U


# ---- the entry points' validation, without a GPU ---------------------------------------------------------------------------------
def test_shade_entry_points_validate_before_any_hip_call():
    L = _lib.lib()
    one = ctypes.c_void_p(16)               # never dereferenced: validation fails first, or n == 0
    mm = (ctypes.c_float * 9)(*range(9))
    light = (ctypes.c_float * 3)(1, 2, 3)
    sv = L.shacira_shade_view
    E = _lib.EINVAL
    assert sv(-1, _lib.SHADE_RB, one, one, one, None, one, 4, 4, 3, one, None, None, None) == E             # n < 0
    assert sv(0, 3, one, one, one, None, one, 4, 4, 3, one, None, None, None) == E                          # unknown mode
    assert sv(0, -1, one, one, one, None, one, 4, 4, 3, one, None, None, None) == E
    assert sv(0, _lib.SHADE_MATCAP, one, one, one, None, one, 1, 4, 3, one, None, None, None) == E          # mh == 1
    assert sv(0, _lib.SHADE_MATCAP, one, one, one, None, one, 4, 1, 3, one, None, None, None) == E          # mw == 1
    assert sv(0, _lib.SHADE_MATCAP, one, one, one, None, one, 4, 4, 2, one, None, None, None) == E          # channels
    assert sv(0, _lib.SHADE_MATCAP, one, one, one, None, one, 4, _lib.SHADE_MAX_TEX + 1, 3, one, None, None, None) == E
    assert sv(0, _lib.SHADE_NORMAL, one, one, one, None, None, 0, 0, 0, one, one, None, None) == E          # uv outside matcap
    for mode in (_lib.SHADE_RB, _lib.SHADE_NORMAL, _lib.SHADE_MATCAP):                                      # n == 0: nothing to do
        assert sv(0, mode, None, None, None, None, None, 4, 4, 3, None, None, None, None) == 0
    assert sv(0, _lib.SHADE_MATCAP, None, None, None, mm, one, 2, 2, 4, None, None, None, None) == 0
    assert sv(5, _lib.SHADE_RB, None, None, one, None, None, 0, 0, 0, None, None, None, None) == E          # rgb
    assert sv(5, _lib.SHADE_NORMAL, None, None, one, None, None, 0, 0, 0, one, None, None, None) == E       # normal
    assert sv(5, _lib.SHADE_MATCAP, one, None, one, None, one, 4, 4, 3, one, None, None, None) == E         # dirs
    assert sv(5, _lib.SHADE_MATCAP, one, one, None, None, None, 0, 0, 0, None, None, None, None) == E       # no tex, no uv_out
    assert sv(5, _lib.SHADE_MATCAP, one, one, None, None, None, 0, 0, 0, one, one, None, None) == E         # no tex but rgb
    assert sv(5, _lib.SHADE_MATCAP, one, one, one, None, one, 4, 4, 3, one, ctypes.c_void_p(20), None, None) == E   # uv alignment
    sr = L.shacira_shadow_rays
    assert sr(-1, one, one, light, -2.0, 0, one, one, one, one, one, one, one, one, None) == E
    assert sr(0, None, None, None, -2.0, 0, None, None, None, None, None, None, None, None, None) == 0
    args = [one, one, light, -2.0, 0, one, one, one, one, one, one, one, one]
    for k in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12):
        bad = list(args)
        bad[k] = None
        assert sr(5, *bad, None) == E, k
    sa, wsb = L.shacira_shadow_apply, L.shacira_shadow_apply_workspace_bytes
    assert wsb(3, 5) == 60 and wsb(0, 5) == 0 and wsb(5, -1) == 0 and wsb(1 << 20, 1 << 20) == 0 and wsb(1, 1) == 4
    two = ctypes.c_void_p(32)
    assert sa(0, 5, 3, one, one, two, one, one, 1 << 20, None) == E
    assert sa(3, 5, 2, one, one, two, one, one, 1 << 20, None) == E                                        # channels
    assert sa(3, 5, 5, one, one, two, one, one, 1 << 20, None) == E
    assert sa(1 << 20, 1 << 20, 3, one, one, two, one, one, 1 << 20, None) == E                            # H W >= 2^31
    assert sa(3, 5, 3, None, one, two, one, one, 1 << 20, None) == E
    assert sa(3, 5, 3, one, None, two, one, one, 1 << 20, None) == E
    assert sa(3, 5, 3, one, one, None, one, one, 1 << 20, None) == E
    assert sa(3, 5, 3, one, one, two, None, one, 1 << 20, None) == E
    assert sa(3, 5, 3, one, one, one, one, one, 1 << 20, None) == E                                        # shadow_out overlaps
    assert sa(3, 5, 3, one, two, ctypes.c_void_p(24), one, one, 1 << 20, None) == E                        # ... in part, both inputs
    assert sa(3, 5, 3, two, one, ctypes.c_void_p(18), one, one, 1 << 20, None) == E                        # ... each from either side
    assert sa(3, 5, 3, one, one, ctypes.c_void_p(31), one, None, 0, None) == _lib.EWORKSPACE               # adjacent is no overlap
    assert wsb(1 << 30, 1) == 0 and wsb(1, 1 << 30) == 0 and wsb((1 << 30) - 1, 2) == ((1 << 30) - 1) * 8  # a side of 2^30
    assert sa(1 << 30, 1, 3, one, one, two, one, one, 1 << 40, None) == E
    assert sa(3, 5, 4, one, one, two, ctypes.c_void_p(20), one, 1 << 20, None) == E                        # fp32 x 4 alignment
    assert sa(3, 5, 3, one, one, two, one, None, 1 << 20, None) == _lib.EWORKSPACE
    assert sa(3, 5, 3, one, one, two, one, one, 59, None) == _lib.EWORKSPACE
    sc = L.shacira_sdf_slice_colors
    assert sc(-1, one, one, None) == E and sc(0, None, None, None) == 0
    assert sc(5, None, one, None) == E and sc(5, one, None, None) == E
    assert L.shacira_abi_version() == 11


def test_hip_ops_wrappers_refuse_host_tensors_and_bad_operands():
    n3 = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.shade_view("normal", normal=n3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.shadow_rays(n3, n3, torch.zeros(4), n3, n3, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.shadow_apply(2, 2, torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), n3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.sdf_slice_colors(torch.zeros(4))
    with pytest.raises(RuntimeError, match="mode"):
        hip_ops.shade_view("phong", normal=n3)


def test_renderer_imports_under_the_reference_names():
    import sys
    import shacira_amd.wisp as mirror
    saved = {k: v for k, v in sys.modules.items() if k == "wisp" or k.startswith("wisp.")}
    try:
        mirror.install_as_wisp(force=True)
        from wisp.models.pipeline import Pipeline as P
        from wisp.offline_renderer import OfflineRenderer as O
        from wisp.ops.image.processing import linear_to_srgb as L2S
        from wisp.ops.shaders import matcap_shader as M, pointlight_shadow_shader as S
        assert O is OfflineRenderer and P is Pipeline and M is matcap_shader and S is pointlight_shadow_shader
        assert L2S is linear_to_srgb
    finally:
        for k in [k for k in sys.modules if k == "wisp" or k.startswith("wisp.")]:
            del sys.modules[k]
        sys.modules.update(saved)
