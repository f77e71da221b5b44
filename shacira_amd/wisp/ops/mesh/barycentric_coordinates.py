"""``barycentric_coordinates`` of the reference (wisp/ops/mesh/barycentric_coordinates.py; the API of libigl's function of
that name), its clipping to [0, 1] included."""
import torch


def barycentric_coordinates(points: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor):
    """Barycentric weights [N, 3] (of ``A``, ``B``, ``C``) of ``points`` [N, 3] in the triangles with vertices ``A``, ``B``,
    ``C`` [N, 3] each. The weights of B and C are clipped to [0, 1] and so is 1 minus their sum, as in the reference: for
    a point outside its triangle the three no longer add up to one."""
    v0, v1, v2 = B - A, C - A, points - A
    d00 = (v0 * v0).sum(dim=-1)
    d01 = (v0 * v1).sum(dim=-1)
    d11 = (v1 * v1).sum(dim=-1)
    d20 = (v2 * v0).sum(dim=-1)
    d21 = (v2 * v1).sum(dim=-1)
    denom = d00 * d11 - d01 * d01
    l1 = torch.clip((d11 * d20 - d01 * d21) / denom, 0.0, 1.0)
    l2 = torch.clip((d00 * d21 - d01 * d20) / denom, 0.0, 1.0)
    l0 = torch.clip(1.0 - (l1 + l2), 0.0, 1.0)
    return torch.stack([l0, l1, l2], dim=-1).to(torch.float32)
