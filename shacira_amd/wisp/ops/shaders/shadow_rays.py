"""Point-light shadows over a ground plane (reference wisp/ops/shaders/shadow_rays.py): the plane and the shadow rays in one
kernel, the tracer on the shadow rays, then the blurred shadow map times the colours in a second kernel pair (shade.hip). The
reference blurs on the host with scipy; device buffers never leave the device here.

Where the reference's text cannot be followed as written (include/shacira_hip.h states the same): it normalises the shadow
directions over the ray axis and keeps row [0] -- here every ray's direction is normalised; it blurs ``shadow_map[..., 0]`` of
a flat array -- here the blur runs over the [height, width] view, so the buffer must hold height * width pixels; its jitter
comes from the torch generator -- here it is a function of (seed, ray index)."""
import numpy as np
import torch
import torch.nn.functional as F

from .... import hip_ops
from ...core import Rays

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
_SHADOW_STREAM = 0x53484457
BLUR_RADIUS = 8


def _shadow_gaussians(n, seed):
    """fp32 [n, 3] on the host: the kernel's jitter -- Philox4x32-10 on (ray index, stream) under the seed, then Box-Muller."""
    idx = np.arange(n, dtype=np.uint64)
    c = [idx & np.uint64(_MASK), idx >> np.uint64(32), np.full(n, _SHADOW_STREAM, np.uint64), np.zeros(n, np.uint64)]
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & np.uint64(_MASK)]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    below = [((w >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24 for w in (c[0], c[2])]
    above = [(w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 for w in (c[1], c[3])]
    r0, r1 = np.sqrt(-2.0 * np.log(below[0])), np.sqrt(-2.0 * np.log(below[1]))
    g = np.stack([r0 * np.cos(2 * np.pi * above[0]), r0 * np.sin(2 * np.pi * above[0]), r1 * np.cos(2 * np.pi * above[1])], axis=1)
    return torch.from_numpy(g.astype(np.float32))


def gaussian_blur_torch(image):
    """[H, W] -> [H, W]: ``scipy.ndimage.gaussian_filter(sigma=2)`` in torch -- 17 normalised taps, axis 0 then axis 1, the
    border reflected (d c b a | a b c d) and continued periodically, so any H, W >= 1 works."""
    k = torch.arange(-BLUR_RADIUS, BLUR_RADIUS + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * k * k / 4.0)
    w = (w / w.sum()).to(image.dtype).to(image.device)
    out = image
    for axis in (0, 1):
        n = out.shape[axis]
        j = torch.remainder(torch.arange(n)[:, None] + torch.arange(-BLUR_RADIUS, BLUR_RADIUS + 1)[None, :], 2 * n)
        j = torch.where(j < n, j, 2 * n - 1 - j).to(image.device)                    # [n, 17]
        taken = out.index_select(axis, j.reshape(-1))
        taken = taken.reshape(n, 2 * BLUR_RADIUS + 1, out.shape[1]) if axis == 0 else taken.reshape(out.shape[0], n, -1)
        out = torch.einsum("nkw,k->nw", taken, w) if axis == 0 else torch.einsum("hnk,k->hn", taken, w)
    return out


def _trace_hits(pipeline, rays, render_batch):
    packs = rays.split(render_batch) if render_batch and render_batch > 0 else [rays]
    return torch.cat([pipeline.tracer(pipeline.nef, rays=pack).hit.reshape(-1) for pack in packs])


def pointlight_shadow_shader(rb, rays, pipeline, point_light=[1.5, 4.5, 1.5], min_y=-2.0, seed=0, height=None, width=None,
                             render_batch=-1):
    """Adds the ground plane y = ``min_y`` behind the traced surface and darkens every pixel whose shadow ray towards
    ``point_light`` is blocked: ``rb.hit``, ``rb.depth``, ``rb.xyz`` and ``rb.normal`` take the plane where it is in front,
    ``rb.shadow`` is set, and ``rb.rgb[..., :3]`` is multiplied by the blurred shadow map (1 lit, 0.7 shadowed). The buffer
    must be flat, [n, C] channels with n == height * width, the view the shadow map is blurred over. The shadow rays are
    traced with ``pipeline.tracer`` in batches of ``render_batch`` (-1: all at once). Returns ``rb``."""
    n = rays.origins.shape[0]
    if height is None or width is None or int(height) * int(width) != n:
        raise ValueError(f"pointlight_shadow_shader blurs the shadow map over the view: it needs height * width == the number "
                         f"of rays ({n}), got height={height}, width={width}")
    H, W = int(height), int(width)
    with torch.no_grad():
        if rays.origins.is_cuda:
            rb.depth, rb.xyz, rb.normal = (t.detach().float().contiguous() for t in (rb.depth, rb.xyz, rb.normal))
            rb.hit, rb.rgb = rb.hit.contiguous(), rb.rgb.detach().float().contiguous()
            so, sd, light_hit, _ = hip_ops.shadow_rays(rays.origins.float().contiguous(), rays.dirs.float().contiguous(),
                                                       rb.depth, rb.xyz, rb.normal, rb.hit, point_light, min_y, seed)
            occluded = _trace_hits(pipeline, Rays(so, sd, dist_min=0, dist_max=rays.dist_max), render_batch)
            rb.shadow = hip_ops.shadow_apply(H, W, occluded.contiguous(), light_hit, rb.rgb)
            return rb
        o, d = rays.origins, rays.dirs
        depth = rb.depth.reshape(-1)
        plane_t = (o[:, 1] - min_y) / (-d[:, 1])
        plane_hit = (plane_t > 0) & (plane_t < 500) & (plane_t < depth)
        rb.hit = (rb.hit.reshape(-1) & ~plane_hit).reshape(rb.hit.shape)
        rb.depth = torch.where(plane_hit, plane_t, depth).reshape(rb.depth.shape)
        rb.xyz = torch.where(plane_hit[:, None], o + d * plane_t[:, None], rb.xyz)
        rb.normal = torch.where(plane_hit[:, None], torch.tensor([0.0, 1.0, 0.0]), rb.normal)
        so = rb.xyz + 0.01 * rb.normal
        sd = F.normalize((torch.tensor([list(point_light)], dtype=torch.float32) + 0.01 * _shadow_gaussians(n, seed)) - so, dim=1)
        light_hit = (sd * rb.normal).sum(-1) > 0.0
        occluded = _trace_hits(pipeline, Rays(so, sd, dist_min=0, dist_max=rays.dist_max), render_batch)
        rb.shadow = occluded.bool() & light_hit
        shadow_map = torch.clamp((1.0 - rb.shadow.float()) + 0.7, 0.0, 1.0).reshape(H, W)
        rb.rgb = rb.rgb.clone()
        rb.rgb[..., :3] *= gaussian_blur_torch(shadow_map).reshape(n, 1)
    return rb
