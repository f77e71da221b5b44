"""wisp.datasets on the host (no GPU): a NeRF-synthetic style dataset written into tmp_path and read back -- metadata keys,
pose handling, compositing, sampling, SampleRays and the residency counters."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import raygen_ref
from shacira_amd.wisp.core import Camera, blender_coords
from shacira_amd.wisp.datasets import NeRFSyntheticDataset, SampleRays
from shacira_amd.wisp.ops import raygen as rg

V, H, W = 3, 4, 6


def blender_pose(eye):
    """Camera-to-world matrix of a z-up camera at `eye` looking at the origin (columns: right, up, backward, position)."""
    eye = np.asarray(eye, np.float64)
    back = eye / np.linalg.norm(eye)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, up, back, eye
    return pose


def write_dataset(root, channels=4, meta=None, split_name="transforms_train.json", with_ext=False, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    images, frames = [], []
    for i in range(V):
        img = rng.integers(0, 256, (H, W, channels), dtype=np.uint8)
        if channels == 4:
            img[..., 3] = rng.choice(np.array([0, 128, 255], np.uint8), (H, W))
            img[0, :3, 3] = [0, 128, 255]
        Image.fromarray(img, "RGBA" if channels == 4 else "RGB").save(os.path.join(root, "train", f"r_{i}.png"))
        images.append(img)
        pose = blender_pose([3.0 * math.cos(1.0 + i), 3.0 * math.sin(1.0 + i), 1.0 + 0.5 * i])
        frames.append(dict(file_path=f"./train/r_{i}" + (".png" if with_ext else ""), transform_matrix=pose.tolist()))
    meta = dict(meta if meta is not None else {"camera_angle_x": 0.6911})
    meta["frames"] = frames
    with open(os.path.join(root, split_name), "w") as fh:
        json.dump(meta, fh)
    return np.stack(images), np.stack([np.array(f["transform_matrix"]) for f in frames])


def test_loader_round_trip_rgba(tmp_path):
    images, poses = write_dataset(str(tmp_path))
    ds = NeRFSyntheticDataset(str(tmp_path), split="train", bg_color="white")
    assert len(ds) == V and ds.img_shape == torch.Size((H, W, 3)) and ds.basenames == ["r_0", "r_1", "r_2"]
    assert ds.images.dtype == torch.uint8 and np.array_equal(ds.images.numpy(), images)
    assert isinstance(ds.cameras, Camera) and len(ds.cameras) == V and ds.cameras.dtype == torch.float64
    assert ds.cameras.near == 0.0 and ds.cameras.far == 6.0 and (ds.cameras.width, ds.cameras.height) == (W, H)
    fx = 0.5 * W / math.tan(0.5 * 0.6911)
    assert torch.allclose(ds.cameras.focal_x, torch.full((V,), fx, dtype=torch.float64), rtol=1e-15)
    assert torch.equal(ds.cameras.focal_y, ds.cameras.focal_x)
    assert torch.equal(ds.cameras.x0, torch.zeros(V, dtype=torch.float64))
    # positions: translation / aabb_scale (1.25 by default), then the Blender-to-y-up change (x, y, z) -> (x, z, -y)
    want = torch.from_numpy(poses[:, :3, 3] / 1.25) @ blender_coords().T
    assert torch.allclose(ds.cameras.cam_pos(), want, atol=1e-14)
    assert ds.records.shape == (V, 20) and ds.records.dtype == torch.float32
    # the camera looks at the origin: the central ray of an even-sized image passes it within a pixel
    item = ds[1]
    assert set(item) == {"rays", "rgb", "masks"}
    assert item["rays"].origins.shape == (H * W, 3) and item["rgb"].shape == (H * W, 3) and item["masks"].shape == (H * W, 1)
    assert item["rays"].dist_min == 0.0 and item["rays"].dist_max == 6.0
    o, d = item["rays"].origins[0].double(), item["rays"].dirs.double().mean(0)
    d = d / d.norm()
    assert torch.linalg.norm(torch.linalg.cross(-o / o.norm(), d)) < 1e-6
    # colours: the reference's fp32 chain on the PNG bytes
    rgb, mask = raygen_ref.colors_ref(images[1].reshape(-1, 4), False)
    assert torch.equal(item["rgb"], rgb) and torch.equal(item["masks"][:, 0], mask)
    assert mask[:3].tolist() == [False, True, True]                # alpha 0, 128, 255
    assert torch.equal(item["rgb"][0], torch.ones(3))              # alpha 0 over white
    black = NeRFSyntheticDataset(str(tmp_path), bg_color="black")[1]
    rgb_b, _ = raygen_ref.colors_ref(images[1].reshape(-1, 4), True)
    assert torch.equal(black["rgb"], rgb_b) and torch.equal(black["rgb"][0], torch.zeros(3))
    assert torch.equal(ds[-1]["rgb"], ds[2]["rgb"])
    with pytest.raises(IndexError):
        ds[3]


def test_loader_rgb_only_and_missing_split_file(tmp_path):
    images, _ = write_dataset(str(tmp_path), channels=3, split_name="transforms.json", with_ext=True)
    ds = NeRFSyntheticDataset(str(tmp_path), split="val")           # no transforms_val.json: transforms.json
    assert ds.images.shape == (V, H, W, 3)
    item = ds[0]
    assert torch.equal(item["rgb"], torch.from_numpy(images[0].reshape(-1, 3)).float() / 255.0) and item["masks"].all()
    assert ds.resident_bytes() == V * H * W * 3 + V * 20 * 4
    with pytest.raises(FileNotFoundError):
        NeRFSyntheticDataset(str(tmp_path / "nowhere"))


@pytest.mark.parametrize("meta,fx,fy", [
    ({"x_fov": 40.0}, 0.5 * W / math.tan(math.radians(20.0)), None),
    ({"x_fov": 40.0, "y_fov": 30.0}, 0.5 * W / math.tan(math.radians(20.0)), 0.5 * H / math.tan(math.radians(15.0))),
    ({"x_fov": 40.0, "camera_angle_x": 1.0}, 0.5 * W / math.tan(math.radians(20.0)), None),     # degrees take precedence
    ({"camera_angle_x": 0.8}, 0.5 * W / math.tan(0.4), None),
    ({"camera_angle_x": 0.8, "camera_angle_y": 0.5}, 0.5 * W / math.tan(0.4), 0.5 * H / math.tan(0.25)),
])
def test_focal_keys(tmp_path, meta, fx, fy):
    write_dataset(str(tmp_path), meta=meta)
    cams = NeRFSyntheticDataset(str(tmp_path)).cameras
    assert cams.focal_x[0].item() == pytest.approx(fx, rel=1e-15)
    assert cams.focal_y[0].item() == pytest.approx(fx if fy is None else fy, rel=1e-15)


def test_principal_point_scale_offset_aabb_and_mip(tmp_path):
    meta = {"camera_angle_x": 0.7, "cx": 3.75, "cy": 1.5, "scale": 0.5, "offset": [0.25, -0.5, 1.0], "aabb_scale": 2.0}
    _, poses = write_dataset(str(tmp_path), meta=meta)
    ds = NeRFSyntheticDataset(str(tmp_path))
    assert ds.cameras.x0.tolist() == [3.75 - W // 2] * V and ds.cameras.y0.tolist() == [1.5 - H // 2] * V
    want = torch.from_numpy(poses[:, :3, 3] / 2.0 * 0.5 + np.array([0.25, -0.5, 1.0])) @ blender_coords().T
    assert torch.allclose(ds.cameras.cam_pos(), want, atol=1e-14)
    assert ds.records[0, 14].item() == 0.75 and ds.records[0, 15].item() == -0.5
    with pytest.raises(NotImplementedError):
        NeRFSyntheticDataset(str(tmp_path), mip=1)
    with pytest.raises(ValueError):
        NeRFSyntheticDataset(str(tmp_path), bg_color="green")


def test_sample_and_sample_rays(tmp_path):
    images, _ = write_dataset(str(tmp_path))
    ds = NeRFSyntheticDataset(str(tmp_path))
    whole = [ds[i] for i in range(V)]
    gen = torch.Generator().manual_seed(11)
    s = ds.sample(500, generator=gen)
    assert set(s) == {"rays", "rgb", "masks", "view_idx", "pixel_idx"}
    vi, pi = s["view_idx"], s["pixel_idx"]
    assert vi.dtype == pi.dtype == torch.int32 and vi.shape == pi.shape == (500,)
    assert set(vi.tolist()) == {0, 1, 2} and 0 <= int(pi.min()) and int(pi.max()) < H * W
    all_rgb = torch.stack([w["rgb"] for w in whole])
    all_dirs = torch.stack([w["rays"].dirs for w in whole])
    all_masks = torch.stack([w["masks"] for w in whole])
    assert torch.equal(s["rgb"], all_rgb[vi.long(), pi.long()])
    assert torch.equal(s["masks"], all_masks[vi.long(), pi.long()])
    assert torch.equal(s["rays"].dirs, all_dirs[vi.long(), pi.long()])
    rgb, _ = raygen_ref.colors_ref(images.reshape(V, H * W, 4)[vi.numpy(), pi.numpy()], False)
    assert torch.equal(s["rgb"], rgb)
    one = ds.sample(64, view=2, generator=gen)
    assert (one["view_idx"] == 2).all() and torch.equal(one["rgb"], whole[2]["rgb"][one["pixel_idx"].long()])
    assert torch.equal(one["rays"].origins, whole[2]["rays"].origins[:1].expand(64, 3))
    with pytest.raises(IndexError):
        ds.sample(4, view=V)
    torch.manual_seed(3)
    picked = SampleRays(10)(whole[0])
    torch.manual_seed(3)
    idx = torch.randint(0, H * W, [10])
    assert torch.equal(picked["rgb"], whole[0]["rgb"][idx]) and torch.equal(picked["rays"].dirs, whole[0]["rays"].dirs[idx])
    assert picked["masks"].shape == (10, 1) and len(picked["rays"]) == 10


def test_resident_bytes_arithmetic(tmp_path):
    write_dataset(str(tmp_path))
    ds = NeRFSyntheticDataset(str(tmp_path))
    assert ds.resident_bytes() == V * H * W * 4 + V * 20 * 4
    assert ds.reference_resident_bytes() == V * H * W * 37
    # per pixel the ratio is 37 / 4 = 9.25; the records add 80 bytes a view
    assert ds.reference_resident_bytes() / (ds.images.numel()) == 9.25
