"""Mesh normalisation modes of the reference's ``wisp.ops.mesh.normalize``."""
import torch


def normalize(V: torch.Tensor, F: torch.Tensor, mode: str):
    """(vertices, faces) with the vertices rescaled; the input is not modified.

    'sphere': bounding-box centre to the origin, farthest vertex to distance 1. 'aabb': minimum corner to -1, the longest axis
    to [-1, 1]. 'planar': x and z stretched to [-1, 1] each, y scaled by the longest axis and resting on y = 0. 'none':
    unchanged."""
    if mode == "none":
        return V, F
    if mode == "sphere":
        centre = (V.max(dim=0).values + V.min(dim=0).values) / 2.0
        V = V - centre
        return V * (1.0 / torch.sqrt((V ** 2).sum(dim=-1).max())), F
    if mode == "aabb":
        V = V - V.min(dim=0).values
        return V * (1.0 / V.max()) * 2.0 - 1.0, F
    if mode == "planar":
        V = V - V.min(dim=0).values
        x = V[..., 0] * (1.0 / V[..., 0].max())
        z = V[..., 2] * (1.0 / V[..., 2].max())
        V = torch.stack([x, V[..., 1], z], dim=-1)
        y = V[..., 1] * (1.0 / V.max())
        V = torch.stack([x, y, z], dim=-1) * 2.0 - 1.0
        return torch.stack([V[..., 0], V[..., 1] - V[..., 1].min(), V[..., 2]], dim=-1), F
    raise ValueError(f"normalize: unknown mode {mode!r} (expected 'sphere', 'aabb', 'planar' or 'none')")
