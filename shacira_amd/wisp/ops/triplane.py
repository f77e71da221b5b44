"""Triplane sampling for ``TriplanarGrid``: the autograd Function and the functional API over the HIP kernels of
``triplane.hip`` (contract: include/shacira_hip.h, shacira_triplane_forward).

The reference samples each LOD with three ``F.grid_sample(plane, ..., align_corners=True, padding_mode='reflection')``
calls (wisp/models/grids/triplanar_grid.py) and then stacks, permutes, concatenates and sums. Here one launch reads every
selected LOD and all three planes and writes the 'cat' or the summed 'sum' layout directly.

Kept from the reference's composition:
  * gradients reach every plane parameter, and the coordinates when they require one (fp32, from the coordinates the
    forward read);
  * first order only, as ``grid_sampler_2d_backward`` has no derivative: a backward with ``create_graph=True`` works, a
    second differentiation raises (``once_differentiable``);
  * autocast: ``grid_sample`` runs in the widest input type, so fp32 planes sample in fp32 and return fp32 even for fp16
    coordinates.
Planes or coordinates of other dtypes outside that rule (fp16 or fp64 modules) take the torch composition
(``triplane_torch``) after one ``hip_ops.warn_unfused`` warning; host tensors raise, as every ``hip_ops`` entry does.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from ... import hip_ops

_PLANE_AXES = ((1, 2), (0, 2), (0, 1))   # fmx reads (y, z), fmy (x, z), fmz (x, y): first component = width axis


class TriplaneInterpolate(torch.autograd.Function):
    """coords fp32 [N, 3], the 3 * len(lods) fp32 planes (fmx, fmy, fmz per LOD) -> [N, 3F] ('sum') or [N, len(lods) * 3F]."""

    @staticmethod
    def forward(ctx, coords, lods, multiscale_sum, *planes):
        feats = hip_ops.triplane_forward(coords, lods, planes, multiscale_sum)
        ctx.lods, ctx.multiscale_sum, ctx.fdim = tuple(lods), bool(multiscale_sum), planes[0].shape[1]
        if ctx.needs_input_grad[0]:   # the coordinate gradient reads the plane values; nothing else does
            ctx.save_for_backward(coords, *planes)
        else:
            ctx.save_for_backward(coords)
        return feats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        need_coords = ctx.needs_input_grad[0]
        need_planes = any(ctx.needs_input_grad[3:])
        saved = ctx.saved_tensors
        coords, planes = saved[0], (saved[1:] if need_coords else None)
        grads, grad_coords = hip_ops.triplane_backward(coords, ctx.lods, ctx.fdim, grad_output, ctx.multiscale_sum,
                                                       planes=planes, need_planes=need_planes, need_coords=need_coords)
        if grads is None:
            grads = [None] * (len(ctx.needs_input_grad) - 3)
        else:
            grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])]
        return (grad_coords, None, None, *grads)


def triplane_torch(coords, planes, num_lods, multiscale_sum):
    """The torch composition: per LOD and plane one ``grid_sample``, [x | y | z] per LOD, then 'cat' or a sum over LODs."""
    N = coords.shape[0]
    grid = coords.reshape(1, N, 1, 3)
    per_lod = []
    for l in range(num_lods):
        cols = []
        for p, (a, b) in enumerate(_PLANE_AXES):
            s = F.grid_sample(planes[3 * l + p], grid[..., [a, b]], mode="bilinear", align_corners=True,
                              padding_mode="reflection")
            cols.append(s[0, :, :, 0].transpose(0, 1))
        per_lod.append(torch.cat(cols, dim=-1))
    if multiscale_sum:
        return torch.stack(per_lod, dim=0).sum(0)
    return torch.cat(per_lod, dim=-1)


def triplane_interpolate(coords, lods, planes, multiscale_sum):
    """coords [N, 3] -> [N, 3F] (``multiscale_sum``) or [N, len(lods) * 3F], LODs in the order given.

    ``lods``: the LOD (plane side 2^lod + 1) of each level; ``planes``: fmx, fmy, fmz of each level, NCHW [1, F, S, S]."""
    planes = list(planes)
    hip_ops._need_gpu(coords, *planes)
    if coords.dim() != 2 or coords.shape[-1] != 3:
        raise RuntimeError(f"shacira_amd: coords must be [N, 3], got {tuple(coords.shape)}")
    pdt = {p.dtype for p in planes}
    cdt = coords.dtype
    if torch.is_autocast_enabled("cuda"):   # grid_sample: promote to the widest input type
        for d in pdt:
            cdt = torch.promote_types(cdt, d)
    if pdt == {torch.float32} and cdt == torch.float32:
        return TriplaneInterpolate.apply(coords.float().contiguous(), tuple(int(l) for l in lods), bool(multiscale_sum),
                                         *[p if p.is_contiguous() else p.contiguous() for p in planes])
    hip_ops.warn_unfused("triplane sampling", f"planes {sorted(str(d) for d in pdt)}, coordinates {coords.dtype}: the "
                         "kernels take fp32")
    return triplane_torch(coords, planes, len(planes) // 3, multiscale_sum)
