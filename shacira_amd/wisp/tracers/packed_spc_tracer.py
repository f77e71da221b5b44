"""``PackedSPCTracer``: rays against a structured point cloud, each ray taking the colour of the first cell it meets
(reference wisp/tracers/packed_spc_tracer.py). The reference -- and ``trace_composed`` here, kept as the oracle and the timing
baseline -- emits every ray / cell crossing, marks the first of each ray, looks the colours up and scatters four buffers. A
first hit needs none of the others: ``trace`` is ONE launch of ``shacira_spc_first_hit`` (spc.hip), a walk over the packed
occupancy words that stops at the first occupied cell and reads its colour by slot.

Deviation: ``lod_idx`` other than None or the finest level raises ``ValueError`` -- the reference indexes the finest level's
colours with a coarser level's point indices there."""
import torch

from ... import render as spc_render
from ..core import RenderBuffer


class PackedSPCTracer:
    def get_supported_channels(self):
        return {"depth", "hit", "rgb", "alpha"}

    def get_required_nef_channels(self):
        return {"rgb"}

    def __call__(self, nef, rays, channels=("rgb",), extra_channels=(), lod_idx=None):
        return self.trace(nef, rays, set(channels), set(extra_channels), lod_idx=lod_idx)

    @staticmethod
    def _level(nef, rays, lod_idx):
        max_level = nef.grid.blas.max_level
        if lod_idx is not None and int(lod_idx) != max_level:
            raise ValueError(f"PackedSPCTracer: an SPC field has colours for its finest level {max_level} only, got lod_idx "
                             f"{lod_idx}")
        if not rays.origins.is_cuda:
            raise RuntimeError("PackedSPCTracer: rays must be on the MI355X (HIP) device; there is no CPU fallback")
        return max_level

    def trace(self, nef, rays, channels, extra_channels, lod_idx=None):
        """RenderBuffer(depth [N, 1], hit bool [N], rgb [N, 3], alpha [N, 1]); a miss is 0 / False / 0 / 0."""
        level = self._level(nef, rays, lod_idx)
        spc = getattr(nef, "spc", None)
        if spc is not None and spc.colors is not None and spc.words.device == rays.origins.device:
            from ... import hip_ops
            depth, hit, _, rgb = hip_ops.spc_first_hit(rays.origins, rays.dirs, level, spc.words, spc.rank, spc.colors)
        else:       # an OctreeAS with features of its own: the same launch without colours, then one gather
            hit, pidx, depth = nef.grid.blas.first_hit(rays, level)
            rgb = torch.zeros((hit.shape[0], 3), device=hit.device)
            rows = torch.nonzero(hit).flatten()
            rgb[rows] = nef(ridx_hit=pidx[rows].long(), channels="rgb").squeeze(1).to(rgb.dtype)
        return RenderBuffer(depth=depth[:, None], hit=hit, rgb=rgb, alpha=hit[:, None].float())

    def trace_composed(self, nef, rays, channels, extra_channels, lod_idx=None):
        """The same buffer by the composed path: every crossing from ``raytrace``, the first of each ray by
        ``mark_pack_boundaries``, the colours from the field, four scatters."""
        level = self._level(nef, rays, lod_idx)
        N, dev = rays.origins.shape[0], rays.origins.device
        traced = nef.grid.blas.raytrace(rays, level, with_exit=False)
        first = spc_render.mark_pack_boundaries(traced.ridx)
        rows = traced.ridx[first].long()
        colors = nef(ridx_hit=traced.pidx[first].long(), channels="rgb").squeeze(1)
        depth = torch.zeros((N, 1), device=dev)
        hit = torch.zeros((N,), dtype=torch.bool, device=dev)
        rgb = torch.zeros((N, 3), device=dev)
        alpha = torch.zeros((N, 1), device=dev)
        depth[rows] = traced.depth[first]
        hit[rows] = True
        rgb[rows] = colors.to(rgb.dtype)
        alpha[rows] = 1.0
        return RenderBuffer(depth=depth, hit=hit, rgb=rgb, alpha=alpha)
