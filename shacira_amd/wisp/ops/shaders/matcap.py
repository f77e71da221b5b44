"""Matcap shading (reference wisp/ops/shaders/matcap.py). The reference copies the normals and directions to the host and samples
the texture there with a scipy interpolator; here device buffers take one pass of the shading kernel (shade.hip) and never
leave the device. Host tensors take the same arithmetic in torch."""
import os

import numpy as np
import torch

from .... import hip_ops
from ..geometric import spherical_envmap_torch

_TEXTURES = {}      # (absolute path, device) -> uint8 [mh, mw, 3 or 4]


def matcap_sampler(path, device="cpu"):
    """The matcap texture at ``path`` as a uint8 [mh, mw, 3 or 4] tensor on ``device``, row-major as PIL gives it. Loaded and
    uploaded once per (path, device). (The reference returns a scipy interpolator over the transposed image; the kernel and
    ``sample_matcap_torch`` compute that interpolator's values.)"""
    if not os.path.exists(path):
        raise Exception(f"The path [{path}] does not exist. Check your working directory or use an absolute path to the "
                        "matcap with --matcap-path")
    key = (os.path.abspath(path), str(torch.device(device)))
    if key not in _TEXTURES:
        import PIL.Image
        img = PIL.Image.open(path)
        if img.mode not in ("RGB", "RGBA"):
            img = img.convert("RGB")
        _TEXTURES[key] = torch.from_numpy(np.array(img, dtype=np.uint8)).contiguous().to(device)
    return _TEXTURES[key]


def default_matcap(size=128):
    """A procedural matcap, uint8 [size, size, 3]: a grey sphere lit from the upper left with a soft highlight, for renders that
    name no texture file."""
    y, x = torch.meshgrid(torch.linspace(1, -1, size), torch.linspace(-1, 1, size), indexing="ij")
    z = torch.sqrt(torch.clamp(1.0 - x * x - y * y, min=0.0))
    light = torch.tensor([-0.45, 0.55, 0.70])
    lambert = torch.clamp(x * light[0] + y * light[1] + z * light[2], min=0.0)
    shade = 0.18 + 0.62 * lambert + 0.35 * lambert ** 24
    rgb = torch.stack([shade * 0.96, shade * 0.93, shade * 0.88], dim=-1)
    return (torch.clamp(rgb, 0.0, 1.0) * 255.0).byte().contiguous()


def sample_matcap_torch(tex, uv):
    """fp32 [n, 3]: the bilinear sample of the uint8 [mh, mw, mc] texture at uv in [0, 1]^2 over 255 -- scipy's
    RegularGridInterpolator over linspace(0, 1, mw) x linspace(0, 1, mh), computed in fp64 and rounded as the reference rounds
    it (to fp32, then the division)."""
    mh, mw = tex.shape[:2]
    if mh < 2 or mw < 2:
        raise ValueError(f"a matcap needs at least 2 x 2 texels, got {mh} x {mw}")
    t = tex[..., :3].double()
    x, y = uv[:, 0].double() * (mw - 1), uv[:, 1].double() * (mh - 1)
    x0 = torch.clamp(torch.floor(x).long(), max=mw - 2)
    y0 = torch.clamp(torch.floor(y).long(), max=mh - 2)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    c = ((1 - fx) * (1 - fy) * t[y0, x0] + fx * (1 - fy) * t[y0, x0 + 1] + (1 - fx) * fy * t[y0 + 1, x0]
         + fx * fy * t[y0 + 1, x0 + 1])
    return c.float() / 255.0


def matcap_shader(rb, rays, matcap, mm=None):
    """Sets ``rb.rgb`` to the matcap colour of every pixel: the texture sampled at ``spherical_envmap`` of the (optionally
    rotated) view direction and the normal. ``matcap``: a path to an image or a uint8 [mh, mw, 3 or 4] tensor; ``mm``: 3x3
    rotation applied to the view directions (``dirs @ mm^T``) or None. Returns ``rb``."""
    normal, dirs = rb.normal, rays.dirs
    tex = matcap if torch.is_tensor(matcap) else matcap_sampler(matcap, normal.device)
    shape = dirs.shape
    if normal.is_cuda:
        rgb, _, _ = hip_ops.shade_view("matcap", normal=normal.detach().reshape(-1, 3).float().contiguous(),
                                       dirs=dirs.detach().reshape(-1, 3).float().contiguous(),
                                       matcap=tex.to(normal.device).contiguous(), mm=mm)
        rb.rgb = rgb.reshape(*shape)
        return rb
    view = dirs.clone()
    if mm is not None:
        view = torch.mm(view.reshape(-1, 3), mm.to(view.device).transpose(1, 0)).reshape(*shape)
    uv = spherical_envmap_torch(view, normal.clone())
    rb.rgb = sample_matcap_torch(tex.to(normal.device), uv).reshape(*shape)
    return rb
