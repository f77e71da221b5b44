"""Point clouds from depth images (reference wisp/ops/pointcloud): torch restatements that run on host and device tensors.
The fused device path -- the cloud and the structured point cloud straight from (view, pixel) -- is ``hip_ops.depth_points`` /
``hip_ops.spc_from_depth``; these two functions are its yardstick and the host path of ``RTMVDataset``."""
import torch

__all__ = ["create_pointcloud_from_images", "normalize_pointcloud"]


def create_pointcloud_from_images(rgbs, masks, rays, depths):
    """(coords [M, 3], colors [M, 3]): for every view i the points ``origins + dirs * depth`` and the first three colour channels
    of the pixels where ``masks[i]`` is set, view by view in pixel order. ``rgbs[i]`` [H, W, 3 or 4], ``masks[i]`` [H, W, 1] or
    [H, W], ``rays[i]`` with ``origins`` / ``dirs`` [H, W, 3], ``depths[i]`` [H, W, 1] or [H, W]."""
    coords, colors = [], []
    for rgb, mask, ray, depth in zip(rgbs, masks, rays, depths):
        h, w = mask.shape[:2]
        keep = mask.reshape(h, w).bool()
        d = depth.reshape(h, w, 1)[keep]
        coords.append((ray.origins.reshape(h, w, 3)[keep] + ray.dirs.reshape(h, w, 3)[keep] * d).reshape(-1, 3))
        colors.append(rgb.reshape(h, w, -1)[keep][:, :3].reshape(-1, 3))
    return torch.cat(coords, dim=0), torch.cat(colors, dim=0)


def normalization_from_bounds(lo, hi):
    """(center [3], scale): the centre (max + min) / 2 per axis and 1 / the largest centred coordinate -- which, the cloud's
    box being symmetric about its centre, is the largest half extent -- from the per-axis minimum ``lo`` and maximum ``hi``."""
    center = (hi + lo) / 2.0
    return center, 1.0 / torch.max(hi - center)


def normalize_pointcloud(coords, return_scale=False):
    """``coords`` [N, 3] moved and scaled into [-1, 1]^3: centre = (max + min) / 2 per axis, scale = 1 / the largest of all
    centred coordinates. With ``return_scale``: (coords, center [3], scale)."""
    center = (coords.max(dim=0).values + coords.min(dim=0).values) / 2.0
    centred = coords - center
    scale = 1.0 / centred.max()
    centred = centred * scale
    return (centred, center, scale) if return_scale else centred
