"""``OfflineRenderer``: non-interactive rendering of a pipeline to ``RenderBuffer`` images (reference wisp/offline_renderer.py).
Trace, shade, segment, shadow: everything after the trace is per-pixel arithmetic that the reference does through the host
(scipy for the matcap lookup and the shadow blur, numpy for the slice colours); here device buffers take the kernels of
shade.hip in place and host buffers take the same arithmetic in torch.

Differences from the reference, all deliberate: the shadow shader's (see ``wisp.ops.shaders.shadow_rays``); ``ao=True`` raises,
because the reference's ambient-occlusion block reads an undefined name whenever shadows are on; ``sdf_slice`` and
``normal_slice`` return tensors where the field lives instead of numpy arrays; the model rotation ``mm`` is moved to the rays'
device, not to 'cuda'."""
import time

import numpy as np
import torch
import torch.nn.functional as F

from .. import hip_ops
from .core import RenderBuffer, Rays
from .ops.differential import finitediff_gradient
from .ops.geometric import look_at_rays, normalized_slice
from .ops.shaders import matcap_shader, matcap_sampler, default_matcap, pointlight_shadow_shader

SHADING_MODES = ("rb", "normal", "matcap")


def sdf_slice_colors_torch(d):
    """The slice colour map in torch fp32, one operator at a time, as the kernel computes it (include/shacira_hip.h,
    shacira_sdf_slice_colors): distances of any shape -> [*shape, 3]."""
    d = d.float()
    dd = torch.clip((d + 1.0) / 2.0, 0.0, 1.0)
    blue = torch.clip((dd - 0.5) * 2.0, 0.0, 1.0)
    yellow = 1.0 - blue
    vis = torch.stack([(0.0 + yellow * float(np.float32(0.4))) + float(np.float32(0.2)),
                       (0.0 + yellow * float(np.float32(0.3))) + float(np.float32(0.2)),
                       (blue + yellow * 0.0) + float(np.float32(0.2))], dim=-1)
    vis[dd - 0.5 < 0] = torch.tensor([1.0, 0.38, 0.0], device=d.device)
    for i in range(50):
        vis[torch.abs(dd - float(np.float32(0.02 * i))) < float(np.float32(0.0015))] = 0.8
    vis[torch.abs(dd - 0.5) < float(np.float32(0.004))] = 0.0
    return vis


class OfflineRenderer:
    def __init__(self, render_res=[1024, 720], camera_proj="persp", render_batch=-1, shading_mode="rb",
                 matcap_path=None, shadow=False, ao=False, perf=False, device="cuda", seed=0, **kwargs):
        """render_res: [width, height]; camera_proj: 'persp' or 'ortho'; render_batch: rays per tracer call (-1: all at once);
        shading_mode: 'rb' (the tracer's colours), 'normal' or 'matcap'; matcap_path: an image file, a uint8 [mh, mw, 3 or 4]
        tensor, or None for the procedural ``default_matcap``; shadow: point-light shadows over a ground plane; seed: of the
        shadow rays' jitter; further keywords go to the tracer. The shadow's light and ground plane are the attributes
        ``point_light`` and ``min_y`` (the shader's defaults), to be set on the instance."""
        if shading_mode not in SHADING_MODES:
            raise NotImplementedError(f"shading_mode must be one of {SHADING_MODES}, got {shading_mode!r}")
        if ao:
            raise NotImplementedError("Ambient occlusion is not implemented: the reference's block reads an undefined name "
                                      "whenever shadows are on.")
        self.render_res, self.camera_proj, self.render_batch = render_res, camera_proj, render_batch
        self.shading_mode, self.matcap_path, self.shadow, self.ao, self.perf = shading_mode, matcap_path, shadow, ao, perf
        self.device, self.seed = device, seed
        self.width, self.height = self.render_res
        self.kwargs = kwargs
        self.point_light, self.min_y = [1.5, 4.5, 1.5], -2.0
        self._matcap_source, self._matcap_on_device = None, None

    def _matcap(self, device):
        """The matcap texture on ``device``. A tensor (the given one or ``default_matcap``) is uploaded once and kept until
        ``matcap_path`` or the device changes; a path goes through ``matcap_sampler``'s own cache."""
        if self.matcap_path is not None and not torch.is_tensor(self.matcap_path):
            return matcap_sampler(self.matcap_path, device)
        held = self._matcap_on_device
        if held is None or self._matcap_source is not self.matcap_path or held.device != torch.device(device):
            source = default_matcap() if self.matcap_path is None else self.matcap_path
            self._matcap_source, self._matcap_on_device = self.matcap_path, source.to(device)
        return self._matcap_on_device

    def render_lookat(self, pipeline, f=[0, 0, 1], t=[0, 0, 0], fov=30.0, camera_proj=None, device=None, mm=None, lod_idx=None,
                      camera_clamp=[0, 5]):
        """The view from ``f`` towards ``t`` as a [height, width, C] ``RenderBuffer``. ``mm``: model rotation, applied to the rays
        (``rays @ mm``); camera_clamp: the near and far distances."""
        device = self.device if device is None else device
        ray_o, ray_d = look_at_rays(f, t, self.height, self.width, fov=fov,
                                    mode=self.camera_proj if camera_proj is None else camera_proj, device=device)
        if mm is not None:
            mm = mm.to(ray_o.device)
            ray_o, ray_d = torch.mm(ray_o, mm), torch.mm(ray_d, mm)
        rays = Rays(origins=ray_o, dirs=ray_d, dist_min=camera_clamp[0], dist_max=camera_clamp[1])
        return self.render(pipeline, rays, lod_idx=lod_idx).reshape(self.height, self.width, -1)

    def render(self, pipeline, rays, lod_idx=None):
        """Trace ``rays`` [n, 3] (in batches of ``render_batch``), shade, set the missed pixels' normal and colour to 1, then
        the shadows. Returns the flat ``RenderBuffer``."""
        if self.perf:
            _time = time.time()
        with torch.no_grad():
            if self.render_batch > 0:
                rb = RenderBuffer(xyz=None, hit=None, normal=None, shadow=None, ao=None, dirs=None)
                for ray_pack in rays.split(self.render_batch):
                    rb += pipeline.tracer(pipeline.nef, rays=ray_pack, lod_idx=lod_idx, **self.kwargs)
            else:
                rb = pipeline.tracer(pipeline.nef, rays=rays, lod_idx=lod_idx, **self.kwargs)
        if self.shading_mode == "rb" and rb.rgb is None:          # the tracer does not handle rgb
            rb.rgb = pipeline.nef.rgb(rb.xyz, rays.dirs)
        if self.perf:
            print("Time Elapsed:{:.4f}".format(time.time() - _time))
        if self.shading_mode != "rb" and rb.normal is None:
            raise RuntimeError(f"shading_mode {self.shading_mode!r} needs a tracer that fills the normal channel")

        if rays.origins.is_cuda:
            # shading and segmentation: one pass over the tracer's buffers, in place
            normal = None if rb.normal is None else rb.normal.detach().float().contiguous()
            hit = None if rb.hit is None else rb.hit.reshape(-1).contiguous()
            rb.rgb, _, _ = hip_ops.shade_view(
                self.shading_mode, normal=normal, hit=hit,
                dirs=rays.dirs.detach().float().contiguous() if self.shading_mode == "matcap" else None,
                rgb=rb.rgb.detach().float().contiguous() if self.shading_mode == "rb" else None,
                matcap=self._matcap(rays.origins.device) if self.shading_mode == "matcap" else None)
            rb.normal = normal
        else:
            if self.shading_mode == "matcap":
                rb = matcap_shader(rb, rays, self._matcap(rays.origins.device), mm=None)
            elif self.shading_mode == "normal":
                rb.rgb = (rb.normal + 1.0) / 2.0
            if rb.hit is not None:
                miss = ~rb.hit.reshape(-1)
                if rb.normal is not None:
                    rb.normal = rb.normal.clone()
                    rb.normal[miss] = 1.0
                rb.rgb = rb.rgb.clone()
                rb.rgb[miss] = 1.0

        if self.shadow:
            rb = pointlight_shadow_shader(rb, rays, pipeline, point_light=self.point_light, min_y=self.min_y, seed=self.seed,
                                          height=self.height, width=self.width, render_batch=self.render_batch)
        return rb

    def normal_slice(self, fn, dim=0, depth=0.0):
        """(normalised gradient of ``fn`` + 1) / 2 over a slice, [width, height, 3], where the field lives."""
        pts = normalized_slice(self.width, self.height, dim=dim, depth=depth, device=self.device).reshape(-1, 3)
        normal = (F.normalize(finitediff_gradient(pts, fn).detach()) + 1.0) / 2.0
        return normal.reshape(self.width, self.height, 3)

    def sdf_slice(self, fn, dim=0, depth=0):
        """The field ``fn`` over a slice as colours, fp32 [width, height, 3] where the field lives (call ``.cpu()`` to fetch it):
        orange inside, blue to yellow outside, grey isolines every 0.04, black at the surface."""
        pts = normalized_slice(self.width, self.height, dim=dim, depth=depth, device=self.device)
        with torch.no_grad():
            d = fn(pts.reshape(-1, 3))
        d = d.reshape(self.width, self.height).float().contiguous()
        return hip_ops.sdf_slice_colors(d) if d.is_cuda else sdf_slice_colors_torch(d)

    def shade_images(self, pipeline, f=[0, 0, 1], t=[0, 0, 0], fov=30.0, aa=1, mm=None, lod_idx=None, camera_clamp=[0, 10]):
        """``render_lookat`` (the mean of ``aa`` renders when aa > 1), on the host and transposed to [width, height, C]."""
        if mm is None:
            mm = torch.eye(3)
        if aa > 1:
            rb = RenderBuffer.mean(*[self.render_lookat(pipeline, f=f, t=t, fov=fov, mm=mm, lod_idx=lod_idx,
                                                        camera_clamp=camera_clamp) for _ in range(aa)])
        else:
            rb = self.render_lookat(pipeline, f=f, t=t, fov=fov, mm=mm, lod_idx=lod_idx, camera_clamp=camera_clamp)
        return rb.cpu().transpose()
