"""``RTMVDataset``: multiview images WITH depth, the RTMV format (reference wisp/datasets/formats/rtmv_dataset.py), kept the
way this device wants it.

The reference keeps every pixel's fp32 origin, direction, colour and depth and a mask byte on the host -- 41 bytes per pixel --
and a 12-byte point per valid pixel next to them. Here the device holds the uint8 images (or a mip level's uint16 sums), ONE
fp32 depth plane and the camera records: 8 bytes per RGBA pixel, 7 per RGB pixel. Rays and colours of a batch come from the ray
kernel (``hip_ops.raygen``), and the point cloud, its bounds and the coloured structured point cloud come straight from (view,
pixel) through the kernels of spc.hip (``depth_bounds``, ``depth_points``, ``spc_from_depth``): the cloud is made on demand
and not kept, and ``as_spc`` never makes it.

Files per view: ``NNNNN.json`` (``camera_data.camera_look_at.{eye, at, up}``, ``width``, ``height``, ``intrinsics.{fx, fy}``;
Blender coordinates; near 0, far 6; principal point at the centre), an image of the same basename (PNG or JPG; EXR only when
``pyexr`` imports) and ``NNNNN.depth.npz`` (``arr_0[..., 0]``) or an EXR depth. EXR input is UNTESTED: an EXR reader is
not among this package's dependencies, so the suite cannot exercise it.

A pixel's depth is valid iff the raw value lies in (-1000, 1000), the reference's rule; invalid pixels are stored as NaN, so
that "valid" is "finite" on the device, and read back as ``-coords_scale`` (the reference's -1, scaled like every depth).

Deviations, deliberate: (1) the reference passes PNG / JPG bytes through ``linear_to_srgb`` because its loader assumes linear EXR
input; 8-bit files are already display-encoded and are taken as they are here. (2) ``mip`` = m keeps the colours as
``NeRFSyntheticDataset`` does (exact block sums, OpenCV's INTER_AREA) and takes the depth of a block's top-left pixel
(``depth[::2^m, ::2^m]``), OpenCV's INTER_NEAREST for an integer factor -- restated from its documentation, not checked against
cv2, which is not a dependency of this package."""
import glob
import json
import math
import os
import re

import numpy as np
import torch

from ..core import Camera, Rays, blender_coords
from ..ops.pointcloud import create_pointcloud_from_images, normalization_from_bounds
from ..ops.raygen import camera_records, generate_rays
from .multiview_dataset import MAX_MIP, _load_image, _upload_mip

REFERENCE_BYTES_PER_PIXEL = 41        # fp32 origin, direction, colour and depth (10 floats) and one mask byte

_NO_PYEXR = ("The RTMV dataset provided uses EXR, but module pyexr is not available. To install, run `pip install pyexr`. "
             "You will likely also need `libopenexr`, which through apt you can install with `apt-get install libopenexr-dev` "
             "and on Windows you can install with `pipwin install openexr`.")


def _open_exr(path):
    try:
        import pyexr
    except ImportError:
        raise Exception(_NO_PYEXR)
    return pyexr.open(path)


def _load_view(root, basename):
    """(image uint8 [H, W, 3 or 4], depth fp32 [H, W] with NaN where invalid) of one view."""
    image = None
    for ext in (".png", ".PNG", ".jpg", ".JPG", ".jpeg", ".JPEG"):
        path = os.path.join(root, basename + ext)
        if os.path.exists(path):
            image = _load_image(path)
            break
    if image is None:
        for ext in (".exr", ".EXR"):
            path = os.path.join(root, basename + ext)
            if os.path.exists(path):      # untested: linear floats, display-encoded and quantised to the bytes this class keeps
                from ..ops.image import linear_to_srgb
                img = torch.from_numpy(_open_exr(path).get().astype(np.float32))
                img[..., :3] = linear_to_srgb(img[..., :3].clamp(0.0, 1.0))
                image = (img.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
                break
    if image is None:
        raise Exception("No images found! Check if your dataset path contains an actual RTMV dataset.")
    depth = None
    npz = os.path.join(root, basename + ".depth.npz")
    if os.path.exists(npz):
        depth = np.load(npz)["arr_0"][..., 0]
    else:
        for ext in (".depth.exr", ".exr", ".EXR"):
            path = os.path.join(root, basename + ext)
            if os.path.exists(path):      # untested
                f = _open_exr(path)
                if ext == ".depth.exr":
                    depth = f.get("default")[..., 0]
                elif "depth" in f.channel_map:
                    depth = f.get("depth")[..., 0]
                else:
                    raise Exception("Depth channel not found in the EXR file provided!")
                break
    if depth is None:
        raise Exception("No depth found! Check if your dataset path contains an actual RTMV dataset.")
    depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))
    valid = (depth > -1000) & (depth < 1000)
    return image, torch.where(valid, depth, torch.full_like(depth, float("nan")))


class RTMVDataset:
    def __init__(self, dataset_path, bg_color, mip=0, split="train", train_ratio=2.0 / 3.0, val_ratio=1.0 / 30.0,
                 coords_center=None, coords_scale=None, device=None):
        mip = 0 if mip is None else int(mip)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        if mip > 0 and self.device.type != "cuda":
            raise NotImplementedError("RTMVDataset: mip levels are built on the device (hip_ops.image_mip); a host dataset "
                                      "takes mip=0")
        if not 0 <= mip <= MAX_MIP:
            raise ValueError(f"RTMVDataset: mip must be 0..{MAX_MIP}, got {mip}")
        if bg_color not in ("white", "black"):
            raise ValueError(f"bg_color must be 'white' or 'black', got {bg_color!r}")
        self.dataset_path, self.bg_color, self.mip, self.split = dataset_path, bg_color, mip, split
        self._train_ratio, self._val_ratio = train_ratio, val_ratio
        self._json_files = self._list_jsons_for_split(dataset_path, split, train_ratio, val_ratio)
        imgs, depths, eyes, ats, ups, self.basenames = [], [], [], [], [], []
        meta = None
        for path in self._json_files:
            base = os.path.splitext(os.path.basename(path))[0]
            with open(path) as fh:
                cam = json.load(fh)["camera_data"]
            if meta is None:
                meta = (cam["width"], cam["height"], cam["intrinsics"]["fx"], cam["intrinsics"]["fy"])
            elif meta != (cam["width"], cam["height"], cam["intrinsics"]["fx"], cam["intrinsics"]["fy"]):
                raise ValueError("RTMVDataset: all views must have one image size and one pair of focal lengths")
            image, depth = _load_view(dataset_path, base)
            imgs.append(image)
            depths.append(depth)
            look = cam["camera_look_at"]
            eyes.append(look["eye"]), ats.append(look["at"]), ups.append(look["up"])
            self.basenames.append(base)
        w0, h0, fx, fy = meta
        if any(im.shape != imgs[0].shape for im in imgs) or tuple(imgs[0].shape[:2]) != (h0, w0) or \
                any(tuple(d.shape) != (h0, w0) for d in depths):
            raise ValueError("RTMVDataset: images and depth planes must have the size their json files state")
        f = 1 << mip
        if h0 % f or w0 % f:
            raise ValueError(f"RTMVDataset: mip={mip} needs a height and width divisible by {f}, the views are {h0} x {w0}")
        w, h = w0 // f, h0 // f
        # the intrinsics follow the image plane (the reference's _transform_rtmv_camera): focal lengths scale with the height
        ratio = h / h0
        cameras = Camera.from_args(eye=torch.tensor(eyes, dtype=torch.float64), at=torch.tensor(ats, dtype=torch.float64),
                                   up=torch.tensor(ups, dtype=torch.float64), focal_x=fx * ratio, focal_y=fy * ratio, width=w,
                                   height=h, near=0.0, far=6.0, x0=0.0, y0=0.0, dtype=torch.float64)
        cameras.change_coordinate_system(blender_coords())
        if mip > 0:
            self.images = _upload_mip(imgs, mip, self.device)                  # uint16 sums [V, h, w, C]
        else:
            self.images = torch.stack(imgs).to(self.device).contiguous()       # uint8 [V, h, w, C]
        self.depth = torch.stack([d[::f, ::f] for d in depths]).to(self.device).contiguous()      # fp32 [V, h, w], NaN = invalid
        self.cameras = cameras.to(self.device)
        self.records = camera_records(self.cameras)
        self._img_shape = torch.Size((h, w, 3))
        self._computed_normalization = coords_center is None or coords_scale is None
        if self._computed_normalization:
            lo, hi = self._bounds()
            coords_center, coords_scale = normalization_from_bounds(lo, hi)
        self.coords_center = torch.as_tensor(coords_center, dtype=torch.float32).reshape(3).cpu()
        self.coords_scale = float(coords_scale)
        # cameras moved in fp64, records rebuilt from them; depth scaled in place
        self.cameras.normalize(self.coords_center.to(torch.float64), self.coords_scale)
        self.records = camera_records(self.cameras)
        self.depth *= self.coords_scale

    # ------------------------------------------------------------------------------------------------------- the splits
    @staticmethod
    def _list_jsons_for_split(dataset_path, split, train_ratio, val_ratio):
        """The json files of ``split``: the sorted files cut at floor(n train_ratio) and floor(n val_ratio) after it."""
        files = sorted(glob.glob(os.path.join(dataset_path, "*.json")))
        train_end = math.floor(len(files) * train_ratio)
        val_end = train_end + math.floor(len(files) * val_ratio)
        if split == "train":
            files = files[:train_end]
        elif split == "val":
            files = files[train_end:val_end]
        elif split == "test":
            files = files[val_end:]
        else:
            raise RuntimeError(f"Unknown split type: {split}, split should be any of: ('train', 'val', 'test')")
        if not files:
            raise ValueError(f"RTMVDataset: No JSON files found for split {split} under {dataset_path}")
        return files

    @classmethod
    def is_root_of_dataset(cls, root, files_list):
        """True when ``files_list`` (names without directory) holds NNNNN.json files and as many NNNNN.exr files -- the
        reference's rule, which names EXR scenes only."""
        jsons = [f for f in files_list if re.match(r"\d{5}\.json", f)]
        exrs = [f for f in files_list if re.match(r"\d{5}\.exr", f)]
        return len(jsons) == len(exrs) and len(jsons) > 0

    def create_split(self, split, transform=None):
        """Another split of the same scene, in THIS split's normalisation (centre and scale are passed on)."""
        return RTMVDataset(self.dataset_path, self.bg_color, mip=self.mip, split=split, train_ratio=self._train_ratio,
                           val_ratio=self._val_ratio, coords_center=self.coords_center, coords_scale=self.coords_scale,
                           device=self.device)

    # ------------------------------------------------------------------------------------------------------------ access
    def __len__(self):
        return self.images.shape[0]

    @property
    def img_shape(self):
        return self._img_shape

    @property
    def num_images(self):
        return len(self)

    def supports_depth(self):
        return True

    def _host_views(self):
        """Per view: (rgb [H, W, 3], valid [H, W, 1], Rays [H, W, 3], depth [H, W, 1]) by the torch restatements."""
        V, (H, W) = len(self), self.depth.shape[1:]
        rays, rgb, _ = generate_rays(self.cameras, None, None, None, self.images, self.bg_color, mip=self.mip)
        shape = (V, H, W, 3)
        o, d = rays.origins.reshape(shape), rays.dirs.reshape(shape)
        return ([c for c in rgb.reshape(shape)], [m for m in torch.isfinite(self.depth)[..., None]],
                [Rays(o[v], d[v]) for v in range(V)], [z for z in torch.nan_to_num(self.depth, nan=0.0)[..., None]])

    def _bounds(self):
        """(min [3], max [3]) of the point cloud, on the host: one launch and one 6-float read-back on the device."""
        if self.device.type == "cuda":
            from ... import hip_ops
            bounds, _ = hip_ops.depth_bounds(self.records, self.depth)
            bounds = bounds.cpu()
            return bounds[:3], bounds[3:]
        coords, _ = create_pointcloud_from_images(*self._host_views())
        return coords.min(dim=0).values, coords.max(dim=0).values

    def as_colored_pointcloud(self):
        """(coords fp32 [M, 3], colors uint8 [M, 3]): the points of the valid pixels in (view, pixel) order and their composited
        colours as bytes, made now and not kept."""
        if self.device.type == "cuda":
            from ... import hip_ops
            return hip_ops.depth_points(self.records, self.depth, self.images, self.bg_color, self.mip)
        coords, colors = create_pointcloud_from_images(*self._host_views())
        return coords, torch.round(255.0 * colors).to(torch.uint8)

    def as_pointcloud(self):
        """The point cloud of the valid pixels, fp32 [M, 3] in [-1, 1]^3 (made on demand, not kept)."""
        if self.device.type == "cuda":
            from ... import hip_ops
            return hip_ops.depth_points(self.records, self.depth)[0]
        return self.as_colored_pointcloud()[0]

    def as_spc(self, level):
        """The coloured ``StructuredPointCloud`` of ``level`` of the scene; on the device the cloud is never made."""
        from ..ops.spc import StructuredPointCloud
        if self.device.type == "cuda":
            return StructuredPointCloud.from_depth(self.records, self.depth, self.images, level, self.bg_color, self.mip)
        return StructuredPointCloud.from_pointcloud(*self.as_colored_pointcloud(), level)

    def _batch(self, out, depth):
        valid = torch.isfinite(depth)
        out["depth"] = torch.where(valid, depth, torch.full_like(depth, -self.coords_scale)).reshape(-1, 1)
        out["alpha"] = valid.reshape(-1, 1)
        return out

    def _rays(self, view_idx, pixel_idx, cameras=None, images=None):
        cameras = self.cameras if cameras is None else cameras
        images = self.images if images is None else images
        if self.device.type == "cuda" and cameras is self.cameras:
            from ... import hip_ops
            o, d, rgb, masks = hip_ops.raygen(self.records, cameras.width, cameras.height, view_idx, pixel_idx, None, images,
                                              self.bg_color, mip=self.mip)
            return dict(rays=Rays(o, d, dist_min=cameras.near, dist_max=cameras.far), rgb=rgb, masks=masks)
        rays, rgb, masks = generate_rays(cameras, view_idx, pixel_idx, None, images, self.bg_color, mip=self.mip)
        return dict(rays=rays, rgb=rgb, masks=masks)

    def __getitem__(self, i):
        """View i whole: dict(rays [H W], rgb [H W, 3], masks [H W, 1], depth [H W, 1], alpha bool [H W, 1])."""
        V = len(self)
        if not -V <= i < V:
            raise IndexError(i)
        i = i % V
        hw = self.images.shape[1] * self.images.shape[2]
        if self.device.type == "cuda":
            from ... import hip_ops
            o, d, rgb, masks = hip_ops.raygen(self.records[i:i + 1], self.cameras.width, self.cameras.height, None, None, None,
                                              self.images[i:i + 1], self.bg_color, num_rays=hw, mip=self.mip)
            out = dict(rays=Rays(o, d, dist_min=self.cameras.near, dist_max=self.cameras.far), rgb=rgb, masks=masks)
        else:
            out = self._rays(None, None, self.cameras[i], self.images[i:i + 1])
        return self._batch(out, self.depth[i].reshape(-1))

    def sample(self, num_rays, view=None, generator=None):
        """``num_rays`` random pixels (with replacement) of all views, or of view ``view``: __getitem__'s dict plus ``view_idx``
        and ``pixel_idx`` (int32 [num_rays]). Nothing is read back."""
        V, H, W = self.images.shape[:3]
        draw = lambda high: torch.randint(0, high, (num_rays,), device=self.device, dtype=torch.int32, generator=generator)
        if view is None:
            view_idx = draw(V)
        else:
            if not 0 <= view < V:
                raise IndexError(view)
            view_idx = torch.full((num_rays,), view, device=self.device, dtype=torch.int32)
        pixel_idx = draw(H * W)
        out = self._rays(view_idx, pixel_idx)
        out.update(view_idx=view_idx, pixel_idx=pixel_idx)
        return self._batch(out, self.depth.reshape(V, H * W)[view_idx.long(), pixel_idx.long()])

    def resident_bytes(self):
        """Bytes kept per pixel and per camera: the images (or a mip level's sums), the depth plane and the fp32 records."""
        return sum(t.numel() * t.element_size() for t in (self.images, self.depth, self.records))

    def reference_resident_bytes(self):
        """What the reference's layout keeps for the same views: fp32 origin, direction, colour and depth and a mask byte."""
        V, H, W = self.images.shape[:3]
        return V * H * W * REFERENCE_BYTES_PER_PIXEL
