#!/usr/bin/env python3
"""Generate tests/golden/raygen.npz by RUNNING the reference's ray generation on the CPU (dev container only).

Run:  python tests/golden/make_raygen_golden.py        (needs /root/reference)

The reference's wisp/ops/raygen/raygen.py is executed from its file. It imports ``kaolin.render.camera`` (not installed) and
``wisp.core.Rays``: both are shimmed, the camera by this package's own Camera, which serves the attributes the file reads
(device, dtype, width, height, x0, y0, near, far, fov_distance, tan_half_fov, extrinsics.inv_transform_rays). So the
pixel-to-direction arithmetic recorded here is the reference's own executed text; the camera underneath is ours. Recorded per
case: the camera's arguments and the fp64 origins and directions of every pixel. Nothing of the reference is copied: outputs are
plain arrays."""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from shacira_amd.wisp.core import Camera, CameraFOV, Rays

CASES = {      # name: dict(lens, width, height, eye, at, up, focal_x, focal_y, x0, y0, fov_distance)
    "pinhole_5x3": dict(lens="pinhole", width=5, height=3, eye=[2.0, 1.5, -2.5], at=[0.1, -0.2, 0.3], up=[0.0, 1.0, 0.0],
                        focal_x=4.0, focal_y=4.0, x0=0.0, y0=0.0),
    "pinhole_5x3_offset_fxfy": dict(lens="pinhole", width=5, height=3, eye=[-1.0, 2.0, 3.0], at=[0.0, 0.0, 0.0],
                                    up=[0.0, 0.0, 1.0], focal_x=3.5, focal_y=2.25, x0=0.75, y0=-0.5),
    "pinhole_1x1": dict(lens="pinhole", width=1, height=1, eye=[0.0, 0.0, 3.0], at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0],
                        focal_x=0.8, focal_y=0.6, x0=0.25, y0=0.125),
    "ortho_5x3": dict(lens="ortho", width=5, height=3, eye=[2.0, 1.5, -2.5], at=[0.1, -0.2, 0.3], up=[0.0, 1.0, 0.0],
                      focal_x=4.0, focal_y=4.0, x0=0.75, y0=-0.5, fov_distance=1.75),
    "ortho_1x1": dict(lens="ortho", width=1, height=1, eye=[1.0, 1.0, 1.0], at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0],
                      focal_x=1.0, focal_y=1.0, x0=0.0, y0=0.0, fov_distance=0.5),
}


def _reference_module():
    kaolin = types.ModuleType("kaolin")
    render = types.ModuleType("kaolin.render")
    camera = types.ModuleType("kaolin.render.camera")
    intrinsics = types.ModuleType("kaolin.render.camera.intrinsics")
    camera.Camera, intrinsics.CameraFOV = Camera, CameraFOV
    kaolin.render, render.camera, camera.intrinsics = render, camera, intrinsics
    core = types.ModuleType("wisp.core")
    core.Rays = Rays
    wisp = types.ModuleType("wisp")
    wisp.__path__ = []
    wisp.core = core
    sys.modules.update({"kaolin": kaolin, "kaolin.render": render, "kaolin.render.camera": camera,
                        "kaolin.render.camera.intrinsics": intrinsics, "wisp": wisp, "wisp.core": core})
    spec = importlib.util.spec_from_file_location("reference_raygen", f"{REF}/wisp/ops/raygen/raygen.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_camera(c):
    return Camera.from_args(eye=c["eye"], at=c["at"], up=c["up"], focal_x=c["focal_x"], focal_y=c["focal_y"], width=c["width"],
                            height=c["height"], near=0.0, far=6.0, x0=c["x0"], y0=c["y0"], fov_distance=c.get("fov_distance"),
                            dtype=torch.float64)


def main():
    ref = _reference_module()
    out = {}
    for name, c in CASES.items():
        cam = make_camera(c)
        grid = ref.generate_centered_pixel_coords(c["width"], c["height"], c["width"], c["height"])
        gen = ref.generate_pinhole_rays if c["lens"] == "pinhole" else ref.generate_ortho_rays
        with torch.no_grad():
            rays = gen(cam, grid)
        assert rays.origins.dtype == torch.float64 and rays.origins.shape == (c["width"] * c["height"], 3)
        out[f"{name}.size"] = np.array([c["width"], c["height"]], np.int64)
        out[f"{name}.view_matrix"] = cam.view_matrix()[0].numpy()
        out[f"{name}.intrinsics"] = np.array([c["focal_x"], c["focal_y"], c["x0"], c["y0"],
                                              c.get("fov_distance", float("nan"))], np.float64)
        out[f"{name}.origins"] = rays.origins.numpy()
        out[f"{name}.dirs"] = rays.dirs.numpy()
    path = os.path.join(HERE, "raygen.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
