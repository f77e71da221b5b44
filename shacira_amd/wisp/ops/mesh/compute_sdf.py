"""``compute_sdf``: signed distance of points to a mesh. Device tensors take the fused HIP kernel (``hip_ops.mesh_sdf``); host
tensors take ``mesh_sdf_torch``, the same fp32 operation sequence (include/shacira_hip.h, shacira_mesh_sdf) in torch ops."""
import torch

from .... import hip_ops

_H, _K = 0.707106781, 0.577350269
_DIRECTIONS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0),
               (0.0, _H, _H), (_H, 0.0, _H), (_H, _H, 0.0),
               (0.0, _H, -_H), (_H, 0.0, -_H), (_H, -_H, 0.0),
               (_K, _K, _K), (-_K, _K, _K), (_K, -_K, _K), (_K, _K, -_K))
_BLOCK_PAIRS = 1 << 19    # (point, triangle) pairs per block of the host path: ~40 fp32 temporaries of that size


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross(x, y):
    return (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])


def _edge_d2(e, x, p):
    t = [e[k] * x - p[k] for k in range(3)]
    return (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]


def _mesh_blocks(points, tri, signed=True, winner=False):
    """The pair pass of the contract in fp32 torch ops, every operator rounding once (no fused multiply-add), blocked over
    the points. Yields per block ``(start, stop, least, index, inside)``: the least d2 over the candidate triangles (+inf if
    there are none), with ``winner`` the lowest index that attains it (-1 if none, int64), with ``signed`` the ray-stabbing
    verdict (else None). ``points`` [N, 3] and ``tri`` [T, 3, 3] are fp32 on one device, N > 0 and T > 0."""
    dev = points.device
    N, T = points.shape[0], tri.shape[0]
    one = torch.ones((), dtype=torch.float32, device=dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    # per triangle, [1, T]
    a, b, c = ([tri[None, :, v, k] for k in range(3)] for v in range(3))
    e0 = [b[k] - a[k] for k in range(3)]
    e1 = [c[k] - b[k] for k in range(3)]
    e2 = [a[k] - c[k] for k in range(3)]
    n = _cross(e0, e2)
    m = [_cross(e, n) for e in (e0, e1, e2)]
    r = [one / _dot(e, e) for e in (e0, e1, e2)]
    rn = one / _dot(n, n)
    valid = (n[0] != 0) | (n[1] != 0) | (n[2] != 0)
    g = [-e2[k] for k in range(3)]
    per_dir = []
    for d in _DIRECTIONS if signed else ():
        dv = [torch.full((), x, dtype=torch.float32, device=dev) for x in d]
        w = _cross(dv, g)
        det = _dot(e0, w)
        det64 = det.to(torch.float64)
        per_dir.append((dv, w, one / det, ~((det64 > -1e-8) & (det64 < 1e-8))))
    order = torch.arange(T, device=dev)[None] if winner else None
    block = max(1, _BLOCK_PAIRS // T)
    for start in range(0, N, block):
        p = [points[start:start + block, k, None] for k in range(3)]          # [B, 1]
        p0 = [p[k] - a[k] for k in range(3)]
        p1 = [p[k] - b[k] for k in range(3)]
        p2 = [p[k] - c[k] for k in range(3)]
        s = (torch.copysign(one, _dot(m[0], p0)) + torch.copysign(one, _dot(m[1], p1))) + torch.copysign(one, _dot(m[2], p2))
        edge = [_edge_d2(e, torch.fmax(zero, torch.fmin(_dot(e, pi) * ri, one)), pi)
                for e, pi, ri in ((e0, p0, r[0]), (e1, p1, r[1]), (e2, p2, r[2]))]
        h = _dot(n, p0)
        d2 = torch.where(s < 2, torch.fmin(edge[0], torch.fmin(edge[1], edge[2])), (h * h) * rn)
        d2 = torch.where(d2 < 0, zero, d2)
        least = torch.where(valid, d2, inf)
        # fminf ignores NaN operands: replace them with +inf before the (NaN-propagating) reduction
        least = torch.where(torch.isnan(least), inf, least)
        best = least.amin(dim=1)
        index = None
        if winner:   # "replace iff d2 < best" from +inf over ascending indices: the first index of the minimum, none at +inf
            index = torch.where((least == best[:, None]) & (least < inf), order, T).amin(dim=1)
            index = torch.where(index == T, -1, index)
        inside = None
        if signed:
            q = _cross(p0, e0)
            tau = _dot(g, q)
            inside = torch.ones(best.shape, dtype=torch.bool, device=dev)
            for dv, w, inv, live in per_dir:
                u = _dot(p0, w) * inv
                v = _dot(dv, q) * inv
                t = tau * inv
                hit = live & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1))
                inside &= (hit & (t >= 0)).any(dim=1) & (hit & ~(t >= 0)).any(dim=1)
        yield start, start + block, best, index, inside


def _root(d2):
    """sqrtf is correctly rounded; torch's vectorised host sqrt is not always. Through fp64 it is: the root of an fp32 value
    is at least 2^-50 (relative) away from an fp32 rounding boundary, further than the fp64 root's own error."""
    return d2.double().sqrt().float()


def mesh_sdf_torch(points: torch.Tensor, triangles: torch.Tensor):
    """The contract of ``shacira_mesh_sdf`` in fp32 torch ops, every operator rounding once (no fused multiply-add), blocked
    over the points: [N] fp32 on the device of ``points``. Bit-equal to the kernel for finite inputs."""
    points = points.detach().to(torch.float32)
    tri = triangles.detach().to(device=points.device, dtype=torch.float32)
    N, T = points.shape[0], tri.shape[0]
    out = torch.full((N,), float("inf"), dtype=torch.float32, device=points.device)
    if N == 0 or T == 0:
        return out
    for start, stop, least, _, inside in _mesh_blocks(points, tri):
        dist = _root(least)
        out[start:stop] = torch.where(inside, -dist, dist)
    return out


def compute_sdf(V: torch.Tensor, F: torch.Tensor, points: torch.Tensor, split_size: int = 10 ** 6):
    """Signed distance [N, 1] fp32 of ``points`` [N, 3] to the mesh (``V`` [#V, 3] vertices, ``F`` [#F, 3] indices), negative
    inside. The result lives where ``points`` lives (the reference moves everything to the GPU): device tensors take the HIP
    kernel, host tensors ``mesh_sdf_torch``. ``split_size`` is accepted for the reference's signature and has no effect:
    the kernel has no batch limit."""
    triangles = V.to(points.device)[F.to(points.device)]
    if points.is_cuda:
        return hip_ops.mesh_sdf(points, triangles)[..., None]
    return mesh_sdf_torch(points, triangles)[..., None]
