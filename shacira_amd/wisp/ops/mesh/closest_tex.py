"""``closest_tex`` of the reference (wisp/ops/mesh/closest_tex.py): the colour of the mesh at the closest surface point."""
import torch

from .barycentric_coordinates import barycentric_coordinates
from .closest_point import closest_point
from .sample_tex import sample_tex


def closest_tex(V: torch.Tensor, F: torch.Tensor, TV: torch.Tensor, TF: torch.Tensor, materials, points: torch.Tensor):
    """(rgb [N, 3], hit_pts [N, 3], dist [N, 1]) of ``points`` [N, 3]: the diffuse colour at, the position of and the signed
    distance to the closest point of the mesh ``V`` [#V, 3], ``F`` [#F, 3]. ``TV`` [#VT, 2] are the texture coordinates and
    ``TF`` [#F, 4] per face three indices into them plus the material id (``load_obj_materials``); the uv of a hit is the
    barycentric blend of its face's texture coordinates, or the first two barycentric weights when ``TV`` is empty. One
    pass over the (point, face) pairs; the results live where ``points`` lives."""
    if F.shape[0] == 0:
        raise ValueError("closest_tex: the mesh has no faces")
    dev = points.device
    V, F, TV, TF = V.to(dev), F.to(dev), TV.to(dev), TF.to(dev)
    dist, hit_pts, hit_tidx = closest_point(V, F, points)
    if bool((hit_tidx < 0).any()):
        raise ValueError("closest_tex: the mesh has no non-degenerate face")
    hit_V = V[F[hit_tidx]]
    BC = barycentric_coordinates(hit_pts, hit_V[:, 0], hit_V[:, 1], hit_V[:, 2])
    hit_TF = TF[hit_tidx]
    if TV.shape[0] > 0:
        hit_Tp = (TV[hit_TF[..., :3]] * BC.unsqueeze(-1)).sum(1)
    else:
        hit_Tp = BC[:, :2]
    rgb = sample_tex(hit_Tp, hit_TF[..., 3], materials)
    return rgb, hit_pts, dist
