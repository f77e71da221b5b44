"""``closest_point``: distance, closest point and face index of points against a mesh, in one pass over the (point, triangle)
pairs. Device tensors take the fused HIP kernel (``hip_ops.mesh_closest``); host tensors take ``mesh_closest_torch``, the same
fp32 operation sequence (include/shacira_hip.h, shacira_mesh_closest) in torch ops. The reference's own ``closest_point`` is
an ``assert False``; its signature is kept, plus ``signed``."""
import torch

from .... import hip_ops
from .compute_sdf import _cross, _dot, _edge_d2, _mesh_blocks, _root


def _hit_points(p, tri):
    """The contract's ``hit`` for points ``p`` [M, 3] against their winning triangles ``tri`` [M, 3, 3]."""
    one = torch.ones((), dtype=torch.float32, device=p.device)
    zero = torch.zeros((), dtype=torch.float32, device=p.device)
    p = [p[:, k] for k in range(3)]
    v = [[tri[:, i, k] for k in range(3)] for i in range(3)]
    a, b, c = v
    e = ([b[k] - a[k] for k in range(3)], [c[k] - b[k] for k in range(3)], [a[k] - c[k] for k in range(3)])
    n = _cross(e[0], e[2])
    m = [_cross(ei, n) for ei in e]
    r = [one / _dot(ei, ei) for ei in e]
    rn = one / _dot(n, n)
    pi = [[p[k] - v[i][k] for k in range(3)] for i in range(3)]
    s = (torch.copysign(one, _dot(m[0], pi[0])) + torch.copysign(one, _dot(m[1], pi[1]))) + torch.copysign(one, _dot(m[2], pi[2]))
    x = [torch.fmax(zero, torch.fmin(_dot(e[i], pi[i]) * r[i], one)) for i in range(3)]
    E = [_edge_d2(e[i], x[i], pi[i]) for i in range(3)]
    k = _dot(n, pi[0]) * rn
    first = (E[0] <= E[1]) & (E[0] <= E[2])
    second = E[1] <= E[2]
    out = []
    for j in range(3):
        on_edge = torch.where(first, a[j] + e[0][j] * x[0], torch.where(second, b[j] + e[1][j] * x[1], c[j] + e[2][j] * x[2]))
        out.append(torch.where(s >= 2, p[j] - n[j] * k, on_edge))
    return torch.stack(out, dim=1)


def mesh_closest_torch(points: torch.Tensor, triangles: torch.Tensor, signed: bool = True):
    """The contract of ``shacira_mesh_closest`` in fp32 torch ops, every operator rounding once, blocked over the points:
    (dist [N] fp32, hit [N, 3] fp32, tidx [N] int32) on the device of ``points``. Bit-equal to the kernel for finite inputs."""
    points = points.detach().to(torch.float32)
    tri = triangles.detach().to(device=points.device, dtype=torch.float32)
    N, T = points.shape[0], tri.shape[0]
    dist = torch.full((N,), float("inf"), dtype=torch.float32, device=points.device)
    hit = points.clone()
    tidx = torch.full((N,), -1, dtype=torch.int32, device=points.device)
    if N == 0 or T == 0:
        return dist, hit, tidx
    for start, stop, least, index, inside in _mesh_blocks(points, tri, signed=signed, winner=True):
        d = _root(least)
        dist[start:stop] = torch.where(inside, -d, d) if signed else d
        tidx[start:stop] = index.to(torch.int32)
        won = index >= 0
        hit[start:stop][won] = _hit_points(points[start:stop][won], tri[index[won]])
    return dist, hit, tidx


def closest_point(V: torch.Tensor, F: torch.Tensor, points: torch.Tensor, signed: bool = True):
    """(dist [N, 1] fp32, hit_pts [N, 3] fp32, hit_tidx [N] int64) of ``points`` [N, 3] against the mesh (``V`` [#V, 3]
    vertices, ``F`` [#F, 3] indices): the distance to the surface (negative inside when ``signed``: the bits of
    ``compute_sdf``), the closest surface point and the face it lies on (the lowest index among equally near faces; -1, with
    ``hit_pts = points`` and ``dist = +inf``, when the mesh has no non-degenerate face). The results live where ``points``
    lives: device tensors take the HIP kernel, host tensors ``mesh_closest_torch``."""
    triangles = V.to(points.device)[F.to(points.device)]
    run = hip_ops.mesh_closest if points.is_cuda else mesh_closest_torch
    dist, hit, tidx = run(points, triangles, signed=signed)
    return dist[..., None], hit, tidx.long()
