#!/usr/bin/env python3
"""Generate tests/golden/shade.npz by RUNNING the reference's offline-renderer helpers on the CPU (dev container only).

Run:  python tests/golden/make_shade_golden.py        (needs /root/reference, scipy and PIL)

The reference's wisp/ops/geometric.py, wisp/ops/shaders/matcap.py, wisp/ops/image/processing.py, wisp/core/render_buffer.py and
wisp/offline_renderer.py are executed from their files. What they import and this machine lacks is shimmed with empty modules
(``wisp._C``, ``cv2``, ``wisp.tracers``, ``wisp.ops.differential``, ``wisp.ops.shaders.shadow_rays``) or with this package's own
``Rays`` (``wisp.core``); ``wisp.core.channels`` is a two-name stub, which is enough for the reference's ``RenderBuffer`` class to
load, so ``RenderBuffer.image()`` IS recorded. Two things about ``normalized_slice``: the reference hands its ``device`` argument to
``normalized_grid`` in the place of ``jitter``, so its grid is jittered and lands on the default device 'cuda'. To record it here
the default device of ``normalized_grid`` is set to 'cpu' and ``torch.rand`` returns 0.5 during the call, which makes the jitter
term exactly zero: what is recorded is the unjittered slice.

Recorded: inputs this script draws itself and the outputs of the reference's functions. Nothing of the reference is copied:
plain arrays only."""
import importlib.util
import os
import sys
import tempfile
import types
import warnings

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from shacira_amd.wisp.core import Rays


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, f"{REF}/{rel}")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference_modules():
    def empty(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__all__ = list(attrs)
        sys.modules[name] = m
        return m
    wisp = empty("wisp")
    wisp.__path__ = []
    empty("wisp._C")
    empty("cv2", INTER_LINEAR=1)
    empty("wisp.tracers")
    empty("wisp.ops").__path__ = []
    empty("wisp.ops.differential", finitediff_gradient=None)
    core = empty("wisp.core")
    core.__path__ = []
    empty("wisp.core.channels", Channel=object, create_default_channel=lambda: None)
    rb_mod = _load("wisp.core.render_buffer", "wisp/core/render_buffer.py")
    core.RenderBuffer, core.Rays = rb_mod.RenderBuffer, Rays
    geo = _load("wisp.ops.geometric", "wisp/ops/geometric.py")
    matcap = _load("wisp.ops.shaders.matcap", "wisp/ops/shaders/matcap.py")
    empty("wisp.ops.shaders", matcap_shader=matcap.matcap_shader, pointlight_shadow_shader=None)
    proc = _load("wisp.ops.image.processing", "wisp/ops/image/processing.py")
    off = _load("wisp.offline_renderer", "wisp/offline_renderer.py")
    return geo, matcap, proc, off, rb_mod


def envmap_rows():
    """64 fixed rows (normal, dirs) fp32: the degenerate ones first, then unit vectors."""
    rng = np.random.default_rng(2024)
    normal = rng.normal(size=(64, 3))
    dirs = rng.normal(size=(64, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    head = [((0, 0, 0), (0.3, -0.4, 0.5)), ((0, 0, 0), (0, 0, -1)), ((np.nan, 0, 1), (0, 0, -1)), ((0, 0, 1), (1, 0, 0)),
            ((1, 0, 0), (0, 0, -1)), ((0, 0, 0), (4, 0, -1)), ((0, 0, 0), (-4, 0, -1)), ((0, 0, 0), (0, -4, -1))]
    for i, (n, d) in enumerate(head):
        normal[i], dirs[i] = n, d
    return normal.astype(np.float32), dirs.astype(np.float32)


def matcap_texture():
    """uint8 [5, 7, 4] RGBA (height 5, width 7), drawn here."""
    y, x = np.mgrid[0:5, 0:7]
    return np.stack([30 * x + 5 * y, 250 - 40 * y - 3 * x, (x * y * 11) % 256, 255 - 20 * x], axis=-1).astype(np.uint8)


def rotation():
    a, b = 0.7, -0.4
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (rz @ rx).astype(np.float32)


def slice_distances(n):
    """fp32 [n]: a ramp over [-1.3, 1.3] with NaN and the infinities at the end."""
    d = np.linspace(-1.3, 1.3, n).astype(np.float32)
    d[-3:] = (np.nan, np.inf, -np.inf)
    return d


def main():
    warnings.simplefilter("ignore")
    geo, matcap, proc, off, rb_mod = _reference_modules()
    out = {}
    for h, w in ((5, 3), (3, 5), (4, 4), (1, 1)):
        out[f"grid_{h}x{w}"] = geo.normalized_grid(h, w, device="cpu").numpy()
        out[f"grid_{h}x{w}_noaspect"] = geo.normalized_grid(h, w, device="cpu", use_aspect=False).numpy()

    defaults, rand = geo.normalized_grid.__defaults__, torch.rand
    geo.normalized_grid.__defaults__ = (False, "cpu", True)
    torch.rand = lambda *shape, **kw: torch.full(shape, 0.5)
    try:
        for dim in range(3):
            out[f"slice_dim{dim}"] = geo.normalized_slice(3, 5, dim=dim, depth=0.25, device="cpu").numpy()
        w, h = 6, 4
        d = slice_distances(w * h)
        renderer = off.OfflineRenderer(render_res=[w, h], device="cpu")
        vis = renderer.sdf_slice(lambda pts: torch.from_numpy(d).reshape(-1, 1), dim=0, depth=0)
        out["sdf_slice_d"], out["sdf_slice_vis"] = d, np.asarray(vis)
        out["sdf_slice_res"] = np.array([w, h], np.int64)
    finally:
        geo.normalized_grid.__defaults__, torch.rand = defaults, rand

    for mode in ("persp", "ortho"):
        o, dr = off._look_at([1.5, 1.2, 2.0], [0.1, -0.2, 0.0], 5, 3, mode=mode, fov=40.0, device="cpu")
        out[f"lookat_{mode}_origins"], out[f"lookat_{mode}_dirs"] = o.numpy(), dr.numpy()

    normal, dirs = envmap_rows()
    out["envmap_normal"], out["envmap_dirs"] = normal, dirs
    out["envmap_uv"] = geo.spherical_envmap(torch.from_numpy(dirs), torch.from_numpy(normal)).numpy()

    tex = matcap_texture()
    out["matcap_tex"] = tex
    import PIL.Image
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "matcap.png")
        PIL.Image.fromarray(tex, "RGBA").save(path)
        keep = np.ones(normal.shape[0], dtype=bool)       # every row: a NaN normal has coordinates (0, 0)
        for name, mm in (("nomm", None), ("mm", torch.from_numpy(rotation()))):
            rb = rb_mod.RenderBuffer(normal=torch.from_numpy(normal[keep]))
            rays = Rays(torch.zeros(int(keep.sum()), 3), torch.from_numpy(dirs[keep]))
            out[f"matcap_rgb_{name}"] = matcap.matcap_shader(rb, rays, path, mm=mm).rgb.numpy()
        out["matcap_rows"] = np.nonzero(keep)[0]
        out["matcap_mm"] = rotation()

    lin = torch.linspace(-0.1, 1.3, 57)
    out["srgb_in"], out["srgb_out"] = lin.numpy().copy(), proc.linear_to_srgb(lin.clone()).numpy()

    rng = np.random.default_rng(7)
    chans = dict(rgb=rng.random((4, 3, 3)).astype(np.float32), alpha=rng.random((4, 3, 1)).astype(np.float32),
                 depth=(rng.random((4, 3, 1)) * 3).astype(np.float32), hit=rng.random((4, 3, 1)) < 0.5,
                 normal=(rng.random((4, 3, 3)) * 2 - 1).astype(np.float32))
    img = rb_mod.RenderBuffer(**{k: torch.from_numpy(v) for k, v in chans.items()}).image()
    for k, v in chans.items():
        out[f"image_in_{k}"] = v
        out[f"image_out_{k}"] = getattr(img, k).numpy()
        out[f"image_byte_{k}"] = getattr(img.byte(), k).numpy()

    path = os.path.join(HERE, "shade.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
