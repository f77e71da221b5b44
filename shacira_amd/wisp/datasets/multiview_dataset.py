"""``NeRFSyntheticDataset``: the NeRF-synthetic / instant-ngp "standard" multiview format
(wisp/datasets/formats/nerf_standard_dataset.py), kept the way this device wants it.

The reference generates every ray of every view once and keeps origins, directions and colours as fp32 next to a mask byte:
37 bytes per pixel on the host, indexed per step and copied over. Here the uint8 images and one small record per camera live on
the device -- 3 or 4 bytes per pixel -- and every batch's origins, directions and composited colours are made from (view, pixel)
indices by one kernel (``wisp.ops.raygen.generate_rays``). Nothing per pixel is stored besides the image bytes -- or, at a mip
level, the exact uint16 sums of its pixel blocks (``hip_ops.image_mip``)."""
import json
import os

import numpy as np
import torch

from ..core import Camera, blender_coords
from ..ops.raygen import camera_records, generate_rays

REFERENCE_BYTES_PER_PIXEL = 37        # fp32 origin, direction and colour (9 floats) and one mask byte
MAX_MIP = 4                           # 255 * 4^4 = 65280 fits the uint16 sums; SHACIRA_IMAGE_MIP_MAX
MIP_UPLOAD_BYTES = 256 << 20          # full-resolution bytes on the device at a time while a mip level is built


def _load_image(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        return torch.from_numpy(np.array(im, dtype=np.uint8))


def _upload_mip(imgs, mip, device):
    """The uint16 block sums [V, H >> mip, W >> mip, C] of the host images ``imgs`` on ``device``. The views go up in chunks of
    at most MIP_UPLOAD_BYTES (one view at least) and each chunk's bytes are dropped once its sums are made: the device never
    holds the full-resolution set."""
    from ... import hip_ops
    per_chunk = max(1, MIP_UPLOAD_BYTES // max(1, imgs[0].numel()))
    H, W, C = imgs[0].shape
    sums = torch.empty((len(imgs), H >> mip, W >> mip, C), dtype=torch.uint16, device=device)
    for start in range(0, len(imgs), per_chunk):
        chunk = torch.stack(imgs[start:start + per_chunk]).to(device)
        hip_ops.image_mip(chunk, mip, out=sums[start:start + per_chunk])
        del chunk
    return sums


class NeRFSyntheticDataset:
    """``mip`` = m in 1 .. 4 (device datasets only) trains on the views scaled down by 2^m, as the reference does with cv2's
    INTER_AREA: ``images`` are then the exact uint16 sums of the 2^m x 2^m blocks (8 bytes per RGBA pixel of the level),
    cameras and ``img_shape`` have the level's size, and the ray kernel divides a sum by 255 * 4^m where it makes a colour."""

    def __init__(self, dataset_path, split="train", bg_color="white", device=None, mip=0):
        mip = 0 if mip is None else int(mip)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        if mip > 0 and self.device.type != "cuda":
            raise NotImplementedError("NeRFSyntheticDataset: mip levels are built on the device (hip_ops.image_mip); a host "
                                      "dataset takes mip=0")
        if not 0 <= mip <= MAX_MIP:
            raise ValueError(f"NeRFSyntheticDataset: mip must be 0..{MAX_MIP} (a sum of 4^mip bytes must fit 16 bits), got {mip}")
        if bg_color not in ("white", "black"):
            raise ValueError(f"bg_color must be 'white' or 'black', got {bg_color!r}")
        self.dataset_path, self.split, self.bg_color, self.mip = dataset_path, split, bg_color, mip
        path = os.path.join(dataset_path, f"transforms_{split}.json")
        if not os.path.exists(path):
            path = os.path.join(dataset_path, "transforms.json")
        if not os.path.exists(path):
            raise FileNotFoundError(f"neither transforms_{split}.json nor transforms.json in {dataset_path}")
        with open(path) as fh:
            meta = json.load(fh)
        imgs, poses, self.basenames = [], [], []
        for frame in meta["frames"]:
            fpath = os.path.join(dataset_path, frame["file_path"].replace("\\", "/"))
            if os.path.splitext(fpath)[1] == "":
                fpath += ".png"
            if not os.path.exists(fpath):      # instant-ngp allows frames whose image is missing
                continue
            imgs.append(_load_image(fpath))
            poses.append(torch.tensor(frame["transform_matrix"], dtype=torch.float64))
            self.basenames.append(os.path.basename(os.path.splitext(fpath)[0]))
        if not imgs:
            raise FileNotFoundError(f"{path} names no image that exists")
        if any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError("NeRFSyntheticDataset: all views must have one image size and channel count")
        poses = torch.stack(poses)
        h, w = imgs[0].shape[:2]
        if h % (1 << mip) or w % (1 << mip):
            raise ValueError(f"NeRFSyntheticDataset: mip={mip} needs a height and width divisible by {1 << mip}, the views are "
                             f"{h} x {w}")
        if mip > 0:
            images = _upload_mip(imgs, mip, self.device)               # uint16 [V, H >> mip, W >> mip, C] on the device
        else:
            images = torch.stack(imgs)                                 # uint8 [V, H, W, C]
        h, w = images.shape[1:3]                                       # the level's size from here on
        if "x_fov" in meta:                    # degrees
            fx = (0.5 * w) / np.tan(0.5 * float(meta["x_fov"]) * (np.pi / 180.0))
            fy = (0.5 * h) / np.tan(0.5 * float(meta["y_fov"]) * (np.pi / 180.0)) if "y_fov" in meta else fx
        elif "camera_angle_x" in meta:         # radians
            fx = (0.5 * w) / np.tan(0.5 * float(meta["camera_angle_x"]))
            fy = (0.5 * h) / np.tan(0.5 * float(meta["camera_angle_y"])) if "camera_angle_y" in meta else fx
        else:
            raise ValueError(f"{path} gives no field of view (x_fov or camera_angle_x)")
        x0 = float(meta["cx"]) / (1 << mip) - (w // 2) if "cx" in meta else 0.0
        y0 = float(meta["cy"]) / (1 << mip) - (h // 2) if "cy" in meta else 0.0
        poses[:, :3, 3] /= meta.get("aabb_scale", 1.25)
        poses[:, :3, 3] *= meta.get("scale", 1.0)
        poses[:, :3, 3] += torch.tensor(meta.get("offset", [0.0, 0.0, 0.0]), dtype=torch.float64)
        view = torch.zeros_like(poses)
        view[:, :3, :3] = poses[:, :3, :3].transpose(1, 2)
        view[:, :3, 3] = -(view[:, :3, :3] @ poses[:, :3, 3:4]).squeeze(-1)
        view[:, 3, 3] = 1.0
        cameras = Camera.from_args(view_matrix=view, focal_x=fx, focal_y=fy, width=w, height=h, near=0.0, far=6.0, x0=x0,
                                   y0=y0, dtype=torch.float64)
        cameras.change_coordinate_system(blender_coords())
        self.cameras = cameras.to(self.device)
        self.images = images.to(self.device).contiguous()
        self.records = camera_records(self.cameras)
        self._img_shape = torch.Size((h, w, 3))

    def __len__(self):
        return self.images.shape[0]

    @property
    def img_shape(self):
        return self._img_shape

    @property
    def num_images(self):
        return len(self)

    def _rays(self, view_idx, pixel_idx, cameras=None, images=None):
        cameras = self.cameras if cameras is None else cameras
        images = self.images if images is None else images
        if self.device.type == "cuda" and cameras is self.cameras:     # the records are already on the device
            from ... import hip_ops
            from ..core import Rays
            o, d, rgb, masks = hip_ops.raygen(self.records, cameras.width, cameras.height, view_idx, pixel_idx, None, images,
                                              self.bg_color, mip=self.mip)
            return dict(rays=Rays(o, d, dist_min=cameras.near, dist_max=cameras.far), rgb=rgb, masks=masks)
        rays, rgb, masks = generate_rays(cameras, view_idx, pixel_idx, None, images, self.bg_color, mip=self.mip)
        return dict(rays=rays, rgb=rgb, masks=masks)

    def __getitem__(self, i):
        """View i whole: dict(rays [H W], rgb [H W, 3], masks [H W, 1]), made now and not kept."""
        V = len(self)
        if not -V <= i < V:
            raise IndexError(i)
        i = i % V
        hw = self.images.shape[1] * self.images.shape[2]
        if self.device.type == "cuda":
            from ... import hip_ops
            from ..core import Rays
            # the whole-view form on this view's record and image alone: no index tensors
            o, d, rgb, masks = hip_ops.raygen(self.records[i:i + 1], self.cameras.width, self.cameras.height, None, None, None,
                                              self.images[i:i + 1], self.bg_color, num_rays=hw, mip=self.mip)
            return dict(rays=Rays(o, d, dist_min=self.cameras.near, dist_max=self.cameras.far), rgb=rgb, masks=masks)
        return self._rays(None, None, self.cameras[i], self.images[i:i + 1])

    def sample(self, num_rays, view=None, generator=None):
        """``num_rays`` random pixels (with replacement): of all views with ``view=None``, of view ``view`` otherwise. Returns
        __getitem__'s dict plus ``view_idx`` and ``pixel_idx`` (int32 [num_rays]). Indices and outputs are tensors on the dataset's
        device and nothing is read back."""
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
        return out

    def resident_bytes(self):
        """Bytes this dataset keeps per pixel and per camera: the images (or a mip level's 2-byte sums) and the fp32 records."""
        return self.images.numel() * self.images.element_size() + self.records.numel() * self.records.element_size()

    def reference_resident_bytes(self):
        """What the reference's layout keeps for the same views (at the mip level's size): fp32 origins, directions and colours
        and a mask byte."""
        V, H, W = self.images.shape[:3]
        return V * H * W * REFERENCE_BYTES_PER_PIXEL
