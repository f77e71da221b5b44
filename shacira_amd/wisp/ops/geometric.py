"""Geometric helpers (reference wisp/ops/geometric.py): ``find_depth_bound`` on the HIP kernel of sphere_trace.hip, the two
sphere samplers, the normalised window and slice grids, ``spherical_envmap`` on the shading kernel of shade.hip and the look-at
rays of the offline renderer. Same names and argument orders as the reference."""
import numpy as np
import torch
import torch.nn.functional as F

from ... import render


def pack_ends(info):
    """bool [K] pack boundaries (True at every pack's first nugget) -> (first int32 [P], end int32 [P]): end[p] is
    first[p + 1], and the last pack ends at K. One device-to-host size read-back (``nonzero``)."""
    first = torch.nonzero(info).flatten().int()
    last = torch.full((1,), info.shape[0], dtype=torch.int32, device=info.device)
    return first, torch.cat([first[1:], last])


def find_depth_bound(query, nug_depth, info, curr_idxes=None):
    """For every ray pack the nugget that holds the depth ``query[p]``, or the next one behind it, searched in depth order
    from ``curr_idxes[p]`` to the end of the pack; -1 where there is none or ``curr_idxes[p]`` is -1.

    query fp32 [P] or [P, 1]; nug_depth fp32 [K, 2] (entry, exit); info bool [K], True at the first nugget of every pack;
    curr_idxes int32 [P], default: the pack starts. Returns int32 [P].

    The pack ends always come from ``info``. The reference ignores ``info`` when ``curr_idxes`` is given and bounds pack p by
    ``curr_idxes[p + 1]`` (and the last pack by the number of packs), which lets a walk run into the neighbour's nuggets and
    keeps the last ray from advancing; include/shacira_hip.h states both and the rule used here."""
    first, end = pack_ends(info)
    if curr_idxes is None:
        curr_idxes = first
    return render.find_depth_bound(query, curr_idxes, end, nug_depth)


def sample_unif_sphere(n):
    """n unit vectors, uniform on the sphere (normalised Gaussians), float64 [n, 3]."""
    u = np.random.randn(n, 3)
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def sample_fib_sphere(n):
    """n evenly spread unit vectors on the Fibonacci spiral (the order is not random), float64 [n, 3]."""
    k = np.arange(n, dtype=np.float64) + 0.5
    polar = np.arccos(1.0 - 2.0 * k / n)
    azimuth = 2.0 * np.pi * k / ((1.0 + np.sqrt(5.0)) / 2.0)
    return np.stack([np.cos(azimuth) * np.sin(polar), np.sin(azimuth) * np.sin(polar), np.cos(polar)], axis=-1)


def normalized_grid(height, width, jitter=False, device="cuda", use_aspect=True):
    """fp32 [height, width, 2]: the (x, y) coordinates of a normalised window, x from -1 to 1 along the width and y from 1 down
    to -1 along the height, both ends included (``linspace``: not the pixel-centre rule of ``Camera``). ``jitter`` moves every
    column and every row by up to one pixel (uniform, from the torch generator); ``use_aspect`` scales the longer side by the
    aspect ratio."""
    window_x = torch.linspace(-1, 1, steps=width, device=device)
    window_y = torch.linspace(1, -1, steps=height, device=device)
    if jitter:
        window_x = window_x + (2.0 * torch.rand(*window_x.shape, device=device) - 1.0) * (1.0 / width)
        window_y = window_y + (2.0 * torch.rand(*window_y.shape, device=device) - 1.0) * (1.0 / height)
    if use_aspect:
        if width > height:
            window_x = window_x * (width / height)
        elif height > width:
            window_y = window_y * (height / width)
    return torch.stack(torch.meshgrid(window_x, window_y, indexing="ij")).permute(2, 1, 0)


def normalized_slice(height, width, dim=0, depth=0.0, device="cuda"):
    """fp32 [height, width, 3]: the points of the axis-aligned plane ``x[dim] == depth`` over the normalised window, with the
    reference's ``y *= -1`` at the end. The reference hands ``device`` to ``normalized_grid`` in the place of ``jitter`` (so its
    slices are jittered and always on the default device); here the window is the plain one, on ``device``."""
    if dim not in (0, 1, 2):
        raise ValueError(f"normalized_slice: dim must be 0, 1 or 2, got {dim}")
    window = normalized_grid(height, width, device=device)
    depth_pts = torch.ones(height, width, 1, device=device) * depth
    parts = [window[..., 0:1], window[..., 1:2]]
    parts.insert(dim, depth_pts)
    pts = torch.cat(parts, dim=-1)
    pts[..., 1] *= -1
    return pts


def spherical_envmap_torch(ray_dir, normal):
    """The reference's ``spherical_envmap`` in torch, where the tensors live: fp32 [n, 2] matcap coordinates."""
    screen = ray_dir.clone()
    screen[..., 2] *= -1
    dot = torch.sum(normal * screen, dim=-1, keepdim=True)
    r = screen - 2.0 * dot * normal
    r[..., 2] -= 1.0
    m = 2.0 * torch.sqrt(torch.sum(r ** 2, dim=-1, keepdim=True))
    uv = 1.0 - ((r[..., :2] / m) + 0.5)
    uv = torch.clip(uv.reshape(-1, 2), 0.0, 1.0)
    uv[torch.isnan(uv)] = 0
    return uv


def spherical_envmap(ray_dir, normal):
    """Matcap coordinates of the view reflected about the normal: [..., 3] directions and normals -> fp32 [n, 2] in [0, 1]
    (NaN -> 0). Device tensors take the shading kernel (shade.hip, coordinates-only form); host tensors take
    ``spherical_envmap_torch``."""
    if not ray_dir.is_cuda:
        return spherical_envmap_torch(ray_dir, normal)
    from ... import hip_ops
    dirs = ray_dir.detach().reshape(-1, 3).float().contiguous()
    nrm = normal.detach().reshape(-1, 3).float().contiguous()
    return hip_ops.shade_view("matcap", normal=nrm, dirs=dirs, with_uv=True)[1]


def look_at_rays(f, t, height, width, mode="persp", fov=90.0, device="cuda"):
    """(origins, dirs) fp32 [height * width, 3] of a camera at ``f`` looking at ``t`` with the world's y axis up: the
    reference's ``_look_at`` and ``_generate_rays`` (wisp/offline_renderer.py). The image plane is ``normalized_grid``
    scaled by tan(fov / 2) at distance 1 -- ``linspace(-1, 1)`` with both ends included, not the pixel-centre rule of
    ``Camera``, so raygen.hip is not reused. ``mode``: 'persp' (one origin, normalised directions) or 'ortho' (origins on the
    plane, one direction). Stays in torch on purpose: it runs once per view, a dozen launches against the thousands of the
    trace that follows."""
    if mode not in ("persp", "ortho"):
        raise ValueError("Invalid camera mode!")
    origin = torch.tensor(list(f), dtype=torch.float32, device=device)
    view = F.normalize(torch.tensor(list(t), dtype=torch.float32, device=device) - origin, dim=0)
    right = F.normalize(torch.linalg.cross(view, torch.tensor([0.0, 1.0, 0.0], device=device)), dim=0)
    up = F.normalize(torch.linalg.cross(right, view), dim=0)
    coord = normalized_grid(height, width, device=device)
    tan = np.tan(np.radians(fov / 2))
    ray_origin = right * coord[..., 0, np.newaxis] * tan + up * coord[..., 1, np.newaxis] * tan + origin + view
    ray_origin = ray_origin.reshape(-1, 3)
    if mode == "ortho":
        ray_dir = F.normalize(view.unsqueeze(0).repeat(ray_origin.shape[0], 1), dim=-1)
    else:
        ray_dir = F.normalize(ray_origin - origin, dim=-1)
        ray_origin = origin.repeat(ray_dir.shape[0], 1)
    return ray_origin, ray_dir
