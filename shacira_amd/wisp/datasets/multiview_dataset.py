"""``NeRFSyntheticDataset``: the NeRF-synthetic / instant-ngp "standard" multiview format
(wisp/datasets/formats/nerf_standard_dataset.py), kept the way this device wants it.

The reference generates every ray of every view once and keeps origins, directions and colours as fp32 next to a mask byte:
37 bytes per pixel on the host, indexed per step and copied over. Here the uint8 images and one small record per camera live on
the device -- 3 or 4 bytes per pixel -- and every batch's origins, directions and composited colours are made from (view, pixel)
indices by one kernel (``wisp.ops.raygen.generate_rays``). Nothing per pixel is stored besides the image bytes."""
import json
import os

import numpy as np
import torch

from ..core import Camera, blender_coords
from ..ops.raygen import camera_records, generate_rays

REFERENCE_BYTES_PER_PIXEL = 37        # fp32 origin, direction and colour (9 floats) and one mask byte


def _load_image(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        return torch.from_numpy(np.array(im, dtype=np.uint8))


class NeRFSyntheticDataset:
    def __init__(self, dataset_path, split="train", bg_color="white", device=None, mip=0):
        if mip not in (0, None):
            raise NotImplementedError("NeRFSyntheticDataset: mip resizing is not implemented (it needs cv2's INTER_AREA)")
        if bg_color not in ("white", "black"):
            raise ValueError(f"bg_color must be 'white' or 'black', got {bg_color!r}")
        self.dataset_path, self.split, self.bg_color = dataset_path, split, bg_color
        self.device = torch.device(device) if device is not None else torch.device("cpu")
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
        images = torch.stack(imgs)                                     # uint8 [V, H, W, C]
        poses = torch.stack(poses)
        h, w = images.shape[1:3]
        if "x_fov" in meta:                    # degrees
            fx = (0.5 * w) / np.tan(0.5 * float(meta["x_fov"]) * (np.pi / 180.0))
            fy = (0.5 * h) / np.tan(0.5 * float(meta["y_fov"]) * (np.pi / 180.0)) if "y_fov" in meta else fx
        elif "camera_angle_x" in meta:         # radians
            fx = (0.5 * w) / np.tan(0.5 * float(meta["camera_angle_x"]))
            fy = (0.5 * h) / np.tan(0.5 * float(meta["camera_angle_y"])) if "camera_angle_y" in meta else fx
        else:
            raise ValueError(f"{path} gives no field of view (x_fov or camera_angle_x)")
        x0 = float(meta["cx"]) - (w // 2) if "cx" in meta else 0.0
        y0 = float(meta["cy"]) - (h // 2) if "cy" in meta else 0.0
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
                                              self.bg_color)
            return dict(rays=Rays(o, d, dist_min=cameras.near, dist_max=cameras.far), rgb=rgb, masks=masks)
        rays, rgb, masks = generate_rays(cameras, view_idx, pixel_idx, None, images, self.bg_color)
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
                                              self.images[i:i + 1], self.bg_color, num_rays=hw)
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
        """Bytes this dataset keeps per pixel and per camera: the images and the fp32 records."""
        return self.images.numel() * self.images.element_size() + self.records.numel() * self.records.element_size()

    def reference_resident_bytes(self):
        """What the reference's layout keeps for the same views: fp32 origins, directions and colours and a mask byte."""
        V, H, W = self.images.shape[:3]
        return V * H * W * REFERENCE_BYTES_PER_PIXEL
