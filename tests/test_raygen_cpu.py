"""Cameras and the host path of wisp.ops.raygen (no GPU): the composite against arrays recorded from the reference's own
raygen.py (run over OUR camera: tests/golden/make_raygen_golden.py) and against the fp64 restatement of the kernel's contract
(tests/raygen_ref.py); Camera construction, batching and the coordinate change."""
import numpy as np
import pytest
import torch

import raygen_ref
from raygen_ref import U
from shacira_amd.wisp.core import Camera, CameraFOV, Rays, blender_coords
from shacira_amd.wisp.ops import raygen as rg
from shacira_amd.wisp.ops.raygen.raygen import _camera_rays

GOLDEN_CASES = ("pinhole_5x3", "pinhole_5x3_offset_fxfy", "pinhole_1x1", "ortho_5x3", "ortho_1x1")
# The kernel's records are the fp64 camera rounded to fp32: each of R, tan, x0, y0 moves by at most U relative. With
# w = R d_cam, |dw| <= U (sqrt(3) |d_cam| + |d_cam|) and a normalised direction moves by at most 2 |dw| / |w|: below 6 U. The
# composite's cast of its fp64 result to fp32 adds U / 2.
RECORD_ROUNDING = 8 * U


def golden_camera(g, name, dtype=torch.float64):
    w, h = (int(v) for v in g[f"{name}.size"])
    fx, fy, x0, y0, fd = g[f"{name}.intrinsics"]
    return Camera.from_args(view_matrix=torch.from_numpy(g[f"{name}.view_matrix"]), focal_x=fx, focal_y=fy, width=w, height=h,
                            near=0.0, far=6.0, x0=x0, y0=y0, fov_distance=None if np.isnan(fd) else fd, dtype=dtype)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_composite_matches_the_reference_arithmetic_over_our_camera(golden, name):
    g = golden("raygen.npz")
    cam = golden_camera(g, name)
    grid = rg.generate_centered_pixel_coords(cam.width, cam.height, cam.width, cam.height)
    gen = rg.generate_pinhole_rays if cam.lens_type == "pinhole" else rg.generate_ortho_rays
    rays = gen(cam, grid)
    assert isinstance(rays, Rays) and rays.dist_min == 0.0 and rays.dist_max == 6.0
    assert rays.origins.dtype == torch.float32 and rays.dirs.shape == (cam.width * cam.height, 3)
    # fp64 chain: the same operators, summed in another order inside the 3x3 product: a few fp64 roundings
    view = torch.zeros(cam.width * cam.height, dtype=torch.long)
    o64, d64 = _camera_rays(cam, view, grid[1].reshape(-1), grid[0].reshape(-1))
    assert np.abs(o64.numpy() - g[f"{name}.origins"]).max() <= 1e-14
    assert np.abs(d64.numpy() - g[f"{name}.dirs"]).max() <= 1e-14
    assert np.abs(rays.dirs.numpy() - g[f"{name}.dirs"]).max() <= U          # the cast
    assert np.abs(rays.origins.numpy() - g[f"{name}.origins"]).max() <= 4 * U  # |origin| < 4
    # generate_rays' whole-view form is the same thing
    rays2, rgb, mask = rg.generate_rays(cam)
    assert rgb is None and mask is None
    assert torch.equal(rays2.dirs, rays.dirs) and torch.equal(rays2.origins, rays.origins)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_fp64_restatement_matches_the_reference_arithmetic(golden, name):
    g = golden("raygen.npz")
    cam = golden_camera(g, name)
    ref = raygen_ref.raygen_ref(rg.camera_records(cam).numpy(), cam.width, cam.height)
    assert ref["valid"].all() and ref["dirs_bound"].max() < raygen_ref.CAP
    assert np.abs(ref["dirs"] - g[f"{name}.dirs"]).max() <= RECORD_ROUNDING
    assert np.abs(ref["origins"] - g[f"{name}.origins"]).max() <= 4 * RECORD_ROUNDING


def random_cameras(V, width, height, ortho=False, seed=0):
    gen = torch.Generator().manual_seed(seed)
    eye = torch.randn(V, 3, generator=gen, dtype=torch.float64)
    eye = 3.0 * eye / eye.norm(dim=1, keepdim=True)
    at = 0.3 * torch.randn(V, 3, generator=gen, dtype=torch.float64)
    return Camera.from_args(eye=eye, at=at, up=[0.0, 1.0, 0.0], focal_x=1.3 * width, focal_y=1.1 * width, width=width,
                            height=height, near=0.0, far=6.0, x0=0.4, y0=-0.3, fov_distance=1.5 if ortho else None)


@pytest.mark.parametrize("ortho", [False, True])
def test_host_generate_rays_against_the_restatement(ortho):
    cams = random_cameras(3, 7, 5, ortho)
    gen = torch.Generator().manual_seed(5)
    n = 200
    view = torch.randint(0, 3, (n,), generator=gen, dtype=torch.int32)
    pixel = torch.randint(0, 35, (n,), generator=gen, dtype=torch.int32)
    jitter = torch.rand(n, 2, generator=gen) - 0.5
    images = torch.randint(0, 256, (3, 5, 7, 4), generator=gen, dtype=torch.uint8)
    for bg in ("white", "black"):
        rays, rgb, mask = rg.generate_rays(cams, view, pixel, jitter, images, bg)
        ref = raygen_ref.raygen_ref(rg.camera_records(cams).numpy(), 7, 5, view.numpy(), pixel.numpy(), jitter.numpy(),
                                    images.numpy(), bg == "black")
        assert np.abs(rays.dirs.numpy() - ref["dirs"]).max() <= RECORD_ROUNDING
        assert np.abs(rays.origins.numpy() - ref["origins"]).max() <= 4 * RECORD_ROUNDING
        assert np.array_equal(rgb.numpy(), ref["rgb"]) and np.array_equal(mask.numpy()[:, 0], ref["mask"])
        assert mask.dtype == torch.bool and mask.shape == (n, 1) and rays.dirs.dtype == torch.float32
    rgb3, mask3 = rg.generate_rays(cams, view, pixel, None, images[..., :3].contiguous())[1:]
    assert torch.equal(rgb3, images.reshape(3, 35, 4)[view.long(), pixel.long(), :3].float() / 255.0) and mask3.all()


def test_a_grid_that_is_not_the_full_centred_one_runs_the_composite():
    cam = random_cameras(1, 8, 6)
    half = rg.generate_centered_pixel_coords(8, 6, 4, 3)
    assert not hasattr(half[0], "_shacira_full_grid")
    rays = rg.generate_pinhole_rays(cam, half)
    full = rg.generate_pinhole_rays(cam, rg.generate_centered_pixel_coords(8, 6, 8, 6))
    assert rays.dirs.shape == (12, 3)
    # the reference places coarse pixel (r, c) at (r * 2 + 0.5, c * 2 + 0.5): the centre of fine pixel (2 r, 2 c)
    assert torch.equal(rays.dirs.reshape(3, 4, 3), full.dirs.reshape(6, 8, 3)[::2, ::2])
    py, px = rg.generate_2d_grid(8, 6)
    assert py.shape == (6, 8) and px[0, 7] == 7 and py[5, 0] == 5
    with pytest.raises(ValueError):
        rg.generate_ortho_rays(cam, half)


def test_camera_by_view_matrix_and_by_look_at_agree():
    a = Camera.from_args(eye=[1.0, 2.0, 3.0], at=[0.0, 0.5, 0.0], up=[0.0, 1.0, 0.0], fov=0.7, width=8, height=6)
    b = Camera.from_args(view_matrix=a.view_matrix()[0], focal_x=a.focal_x[0].item(), focal_y=a.focal_y[0].item(), width=8,
                         height=6)
    assert a.lens_type == b.lens_type == "pinhole" and len(a) == 1 and a.dtype == torch.float64
    assert torch.allclose(a.cam_pos(), torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64), atol=1e-14)
    assert torch.equal(a.cam_pos(), b.cam_pos())
    assert torch.allclose(a.focal_y, torch.tensor([6 / (2 * np.tan(0.35))], dtype=torch.float64))
    assert torch.equal(a.tan_half_fov(CameraFOV.HORIZONTAL), 8 / (2 * a.focal_x))
    assert torch.equal(a.tan_half_fov(CameraFOV.VERTICAL), 6 / (2 * a.focal_y))
    assert torch.allclose(a.view_matrix() @ a.inv_view_matrix(), torch.eye(4, dtype=torch.float64)[None], atol=1e-14)
    # the camera looks down -z at `at`
    to_at = a.view_matrix()[0] @ torch.tensor([0.0, 0.5, 0.0, 1.0], dtype=torch.float64)
    assert abs(to_at[0]) < 1e-14 and abs(to_at[1]) < 1e-14 and to_at[2] < 0
    o, d = a.extrinsics.inv_transform_rays(torch.zeros(2, 3), torch.tensor([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]))
    assert o.shape == d.shape == (1, 2, 3) and torch.allclose(o[0, 0], a.cam_pos()[0])
    grid = rg.generate_centered_pixel_coords(8, 6, 8, 6)
    assert torch.equal(rg.generate_pinhole_rays(a, grid).dirs, rg.generate_pinhole_rays(b, grid).dirs)
    with pytest.raises(ValueError):
        Camera.from_args(view_matrix=a.view_matrix(), eye=[0.0, 0.0, 1.0], focal_x=1.0, width=2, height=2)
    assert Camera.from_args(view_matrix=torch.eye(4), fov_distance=2.0, width=4, height=2).lens_type == "ortho"


@pytest.mark.parametrize("ortho", [False, True])
def test_coordinate_change_moves_positions_and_rays_by_the_basis(ortho):
    """change_coordinate_system(blender_coords()): a world point p becomes B p, (x, y, z) -> (x, z, -y); the picture stays. So
    the camera position and every pixel ray after the change are B times what they were."""
    B = blender_coords()
    assert torch.equal(B @ torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), torch.tensor([1.0, 3.0, -2.0], dtype=torch.float64))
    cam = random_cameras(2, 5, 3, ortho, seed=3)
    before_pos = cam.cam_pos().clone()
    before, _, _ = rg.generate_rays(cam)
    o64, d64 = _camera_rays(cam, torch.arange(30) // 15, (torch.arange(30) % 5) + 0.5, ((torch.arange(30) % 15) // 5) + 0.5)
    cam.change_coordinate_system(B)
    assert torch.allclose(cam.cam_pos(), before_pos @ B.T, atol=1e-14)
    o64b, d64b = _camera_rays(cam, torch.arange(30) // 15, (torch.arange(30) % 5) + 0.5, ((torch.arange(30) % 15) // 5) + 0.5)
    assert torch.allclose(d64b, d64 @ B.T, atol=1e-14) and torch.allclose(o64b, o64 @ B.T, atol=1e-14)
    after, _, _ = rg.generate_rays(cam)
    assert torch.allclose(after.dirs, before.dirs @ B.T.float(), atol=2 * U)


def test_camera_cat_index_and_to():
    cams = random_cameras(4, 6, 4)
    assert len(cams) == 4 and cams.width == 6 and cams.height == 4 and cams.near == 0.0 and cams.far == 6.0
    one = cams[2]
    assert len(one) == 1 and torch.equal(one.view_matrix()[0], cams.view_matrix()[2])
    assert torch.equal(cams[-1].cam_pos()[0], cams.cam_pos()[3])
    assert len(cams[1:3]) == 2
    back = Camera.cat([cams[i] for i in range(4)])
    assert torch.equal(back.view_matrix(), cams.view_matrix()) and torch.equal(back.focal_x, cams.focal_x)
    assert torch.equal(back.x0, cams.x0) and torch.equal(back.y0, cams.y0)
    f32 = cams.to(torch.float32)
    assert f32.dtype == torch.float32 and f32.device == cams.device and cams.dtype == torch.float64
    assert f32.focal_y.dtype == torch.float32
    with pytest.raises(ValueError):
        Camera.cat([cams, random_cameras(1, 5, 4)])
    rec = rg.camera_records(cams)
    assert rec.shape == (4, 20) and rec.dtype == torch.float32
    assert torch.equal(rec[:, 9:12], cams.cam_pos().float()) and torch.equal(rec[:, 16:], torch.zeros(4, 4))
    assert torch.equal(rec[:, 12], (6 / (2 * cams.focal_x)).float())


def test_reference_import_names():
    from shacira_amd.wisp import install_as_wisp
    install_as_wisp()
    from wisp.core import Camera as C2
    from wisp.datasets import NeRFSyntheticDataset, SampleRays            # noqa: F401
    from wisp.datasets.multiview_dataset import NeRFSyntheticDataset as D2
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_ortho_rays, generate_pinhole_rays  # noqa: F401
    from wisp.ops.raygen.raygen import generate_2d_grid, generate_rays    # noqa: F401
    assert C2 is Camera and D2 is NeRFSyntheticDataset


def test_host_wrapper_refuses_host_tensors():
    from shacira_amd import hip_ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.raygen(torch.zeros(1, 20), 4, 4)
