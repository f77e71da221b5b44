"""``PackedSDFTracer``: sphere tracing of a signed distance field through the grid's occupied cells (reference
wisp/tracers/packed_sdf_tracer.py). The ray / cell intersections come from ``grid.raytrace(with_exit=True)``; between two
evaluations of the field, everything the reference does with masked tensor operations -- the march, the hit test, the walk to
the next cell, the compaction of the live rays -- is ONE launch of the fused step kernel (shacira_amd/render.py
``SphereTrace``; contract in include/shacira_hip.h). The field is evaluated on the live rays only.

Two deliberate differences from the reference, both stated in the contract: pack ends are the packs' own (the reference's
``find_depth_bound`` can walk into the neighbouring ray's cells and never advances the last ray), and a ray's depth stops
changing when the ray retires (the reference keeps adding the last step to it).

Not capturable into a HIP graph: every round reads the survivor count back to size the next evaluation.
"""
import torch
import torch.nn.functional as F

from ... import render as spc_render
from ..core import RenderBuffer
from ..ops.differential import finitediff_gradient
from ..ops.geometric import pack_ends


class PackedSDFTracer:
    def __init__(self, num_steps=128, step_size=1.0, min_dis=0.0003):
        self.num_steps, self.step_size, self.min_dis = num_steps, step_size, min_dis

    def get_supported_channels(self):
        return {"depth", "normal", "xyz", "hit", "rgb", "alpha"}

    def get_required_nef_channels(self):
        return {"sdf"}

    def __call__(self, nef, rays, channels=("rgb",), extra_channels=(), lod_idx=None, **overrides):
        opts = dict(num_steps=self.num_steps, step_size=self.step_size, min_dis=self.min_dis)
        opts.update(overrides)
        return self.trace(nef, rays, set(channels), set(extra_channels), lod_idx=lod_idx, **opts)

    def trace(self, nef, rays, channels, extra_channels, lod_idx=None, num_steps=64, step_size=1.0, min_dis=1e-4):
        assert nef.grid is not None, "this tracer requires a grid"
        if not rays.origins.is_cuda:
            raise RuntimeError("PackedSDFTracer: rays must be on the MI355X (HIP) device; there is no CPU fallback")
        N, dev = rays.origins.shape[0], rays.origins.device
        if lod_idx is None:
            lod_idx = nef.grid.num_lods - 1
        xyz = torch.zeros(N, 3, device=dev)
        depth = torch.zeros(N, 1, device=dev)
        hit = torch.zeros(N, dtype=torch.bool, device=dev)
        normal = torch.zeros(N, 3, device=dev)
        rgb = torch.zeros(N, 3, device=dev)
        alpha = torch.zeros(N, 1, device=dev)

        traced = nef.grid.raytrace(rays, nef.grid.active_lods[lod_idx], with_exit=True)
        ridx, pidx, nuggets = traced.ridx, traced.pidx, traced.depth
        if ridx.shape[0] == 0:
            return RenderBuffer(xyz=xyz, depth=depth, hit=hit, normal=normal, rgb=rgb, alpha=alpha)
        nuggets[:, 0] += 1e-5
        first, pack_end = pack_ends(spc_render.mark_pack_boundaries(ridx))
        first_ridx = ridx.index_select(0, first.long()).long()
        state = spc_render.SphereTrace(rays.origins.index_select(0, first_ridx), rays.dirs.index_select(0, first_ridx),
                                       nuggets, first, pack_end, pidx=pidx, step_size=step_size, min_dis=min_dis,
                                       dist_max=rays.dist_max)
        with torch.no_grad():
            for _ in range(num_steps):
                if state.count == 0:
                    break
                # pidx: the cell of every live ray (int32, as the raytrace wrote it), for fields that index by cell
                sdf = nef(coords=state.coords[:state.count], lod_idx=lod_idx, pidx=state.pidx_active[:state.count],
                          channels="sdf")
                state.step(sdf)

        pack_hit = state.hit.bool()
        hit[first_ridx] = pack_hit
        xyz[first_ridx] = torch.where(pack_hit[:, None], state.x, torch.zeros_like(state.x))
        depth[first_ridx] = torch.where(pack_hit, state.t, torch.zeros_like(state.t))[:, None]
        alpha[first_ridx] = pack_hit[:, None].float()
        hit_rays = first_ridx[pack_hit]
        hit_points = state.x[pack_hit]

        extra_outputs = {}
        for channel in extra_channels:
            with torch.no_grad():
                feats = nef(coords=hit_points, lod_idx=lod_idx, channels=channel)
            buffer = torch.zeros(N, feats.shape[-1], device=dev)
            buffer[hit_rays] = feats.reshape(hit_points.shape[0], -1).to(buffer.dtype)
            extra_outputs[channel] = buffer

        if "rgb" in channels or "normal" in channels:
            with torch.no_grad():
                grad = finitediff_gradient(hit_points, nef.get_forward_function("sdf"))
            normal[hit_rays] = F.normalize(grad, p=2, dim=-1, eps=1e-5)
            rgb = (normal + 1.0) / 2.0
        return RenderBuffer(xyz=xyz, depth=depth, hit=hit, normal=normal, rgb=rgb, alpha=alpha, **extra_outputs)
