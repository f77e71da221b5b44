"""Helper, not a test: a numpy restatement of the closest-point contract (include/shacira_hip.h, shacira_mesh_closest) in
np.float32, one rounding per operator, on the helpers and meshes of mesh_sdf_ref.py; and the exact (fp64) closest point on a
triangle after Ericson, Real-Time Collision Detection 5.1.5; and the textured cube the closest_tex tests share."""
import numpy as np
import torch

import mesh_sdf_ref as ref
from mesh_sdf_ref import F32, ONE, Z, _cross, _dot, _edge_d2

INF = F32(np.inf)


def _triangle_terms(a, b, c):
    e = ([b[k] - a[k] for k in range(3)], [c[k] - b[k] for k in range(3)], [a[k] - c[k] for k in range(3)])
    n = _cross(e[0], e[2])
    m = [_cross(ei, n) for ei in e]
    r = [ONE / _dot(ei, ei) for ei in e]
    rn = ONE / _dot(n, n)
    return e, n, m, r, rn


def _pair_terms(p, v, e, m, r):
    pi = [[p[k] - v[i][k] for k in range(3)] for i in range(3)]
    s = (np.copysign(ONE, _dot(m[0], pi[0])) + np.copysign(ONE, _dot(m[1], pi[1]))) + np.copysign(ONE, _dot(m[2], pi[2]))
    x = [np.fmax(Z, np.fmin(_dot(e[i], pi[i]) * r[i], ONE)) for i in range(3)]
    E = [_edge_d2(e[i], x[i], pi[i]) for i in range(3)]
    return pi, s, x, E


def mesh_closest_ref(points, triangles, signed=True):
    """(dist [N] float32, hit [N, 3] float32, tidx [N] int32) of the contract."""
    points = np.ascontiguousarray(points, dtype=F32)
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    N, T = points.shape[0], tri.shape[0]
    dist = np.full((N,), np.inf, dtype=F32)
    hit = points.copy()
    tidx = np.full((N,), -1, dtype=np.int32)
    if N == 0 or T == 0:
        return dist, hit, tidx
    with np.errstate(all="ignore"):
        # the pair pass: d2 of every candidate, the winner by "replace iff d2 < best" over ascending indices
        v = [[tri[None, :, i, k] for k in range(3)] for i in range(3)]
        e, n, m, r, rn = _triangle_terms(*v)
        valid = (n[0] != 0) | (n[1] != 0) | (n[2] != 0)
        block = max(1, ref.BLOCK_PAIRS // T)
        for start in range(0, N, block):
            p = [points[start:start + block, k, None] for k in range(3)]
            pi, s, x, E = _pair_terms(p, v, e, m, r)
            h = _dot(n, pi[0])
            d2 = np.where(s < 2, np.fmin(E[0], np.fmin(E[1], E[2])), (h * h) * rn)
            d2 = np.where(d2 < 0, Z, d2)
            assert d2.dtype == F32
            cand = np.where(valid & ~np.isnan(d2), d2, INF)
            first = np.argmin(cand, axis=1)                      # the first index of the minimum
            least = cand[np.arange(cand.shape[0]), first]
            dist[start:start + block] = np.sqrt(least)
            tidx[start:start + block] = np.where(least < INF, first, -1)
        if signed:                                               # by exactly the existing rule
            dist = np.where(np.signbit(ref.mesh_sdf_ref(points, tri)), -dist, dist)
        # hit, once per point from the winning triangle
        won = tidx >= 0
        w = tri[tidx[won]]
        p = [points[won, k] for k in range(3)]
        v = [[w[:, i, k] for k in range(3)] for i in range(3)]
        e, n, m, r, rn = _triangle_terms(*v)
        pi, s, x, E = _pair_terms(p, v, e, m, r)
        k = _dot(n, pi[0]) * rn
        i0 = (E[0] <= E[1]) & (E[0] <= E[2])
        i1 = E[1] <= E[2]
        out = np.empty((int(won.sum()), 3), dtype=F32)
        for j in range(3):
            on_edge = np.where(i0, v[0][j] + e[0][j] * x[0], np.where(i1, v[1][j] + e[1][j] * x[1], v[2][j] + e[2][j] * x[2]))
            out[:, j] = np.where(s >= 2, p[j] - n[j] * k, on_edge)
            assert on_edge.dtype == F32
        hit[won] = out
    return dist, hit, tidx


def candidates(triangles):
    """bool [T]: the triangles with a non-zero fp32 normal, the only ones the contract measures."""
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    v = [[tri[:, i, k] for k in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        n = _triangle_terms(*v)[1]
    return (n[0] != 0) | (n[1] != 0) | (n[2] != 0)


def closest_on_triangle64(p, a, b, c):
    """Exact closest point of triangles (a, b, c) to points p in fp64, broadcasting over leading dimensions: [..., 3]."""
    p, a, b, c = (np.asarray(t, dtype=np.float64) for t in (p, a, b, c))
    dot = lambda x, y: (x * y).sum(axis=-1)    # noqa: E731
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = dot(ab, ap), dot(ac, ap)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        regions = [
            (d1 <= 0) & (d2 <= 0), a + 0 * p,
            (d3 >= 0) & (d4 <= d3), b + 0 * p,
            (vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None],
            (d6 >= 0) & (d5 <= d6), c + 0 * p,
            (vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None],
            (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None],
        ]
        inner = a + ab * (vb / (va + vb + vc))[..., None] + ac * (vc / (va + vb + vc))[..., None]
    out = inner
    for cond, value in reversed(list(zip(regions[0::2], regions[1::2]))):   # the first matching region wins
        out = np.where(cond[..., None], value, out)
    return out


def distance64(points, triangles):
    """[N, T] fp64: the exact distance of every point to every triangle."""
    tri = np.asarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    p = np.asarray(points, dtype=np.float64)[:, None, :]
    q = closest_on_triangle64(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    return np.linalg.norm(p - q, axis=-1)


# ---- the textured cube of the closest_tex tests ----------------------------------------------------------------------------
EPS = float(np.finfo(np.float32).eps)


def textured_cube():
    """The cube of mesh_sdf_ref: one material per face (material = face quad index), constant colours but for +x (quad 1),
    which carries a 4x4 texture with uv = (y + 0.5, z + 0.5)."""
    V, F = ref.cube(0.5)
    rng = np.random.default_rng(41)
    colours = rng.uniform(0, 1, (6, 3)).astype(np.float32)
    texture = rng.uniform(0, 1, (4, 4, 3)).astype(np.float32)
    TV = (V[:, 1:] + 0.5).astype(np.float32)                                       # per vertex (y, z) + 0.5
    TF = np.concatenate([F, (np.arange(12) // 2)[:, None]], axis=1).astype(np.int64)
    mats = {i: {"diffuse": torch.from_numpy(colours[i])} for i in range(6)}
    mats[1]["diffuse_texname"] = torch.from_numpy(texture)
    return V, F, TV, TF, mats, colours, texture


def face_points(per_face=40, seed=42):
    """Points 0.3 outside each face of the cube, above its inner part: (points [6 * per_face, 3], face quad index)."""
    rng = np.random.default_rng(seed)
    points, quad = [], []
    for q, (axis, sign) in enumerate([(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]):   # the quads of ref.cube
        p = rng.uniform(-0.3, 0.3, (per_face, 3))
        p[:, axis] = sign * 0.8
        points.append(p)
        quad += [q] * per_face
    return np.concatenate(points).astype(np.float32), np.asarray(quad)


def bilinear64(texture, u, v):
    """fp64 bilinear sample of texture [H, W, 3] at uv in [0, 1]^2: grid (u * 2 - 1, -(v * 2 - 1)), align_corners."""
    H, W = texture.shape[:2]
    x = u.astype(np.float64) * (W - 1)
    y = (1.0 - v.astype(np.float64)) * (H - 1)
    x0, y0 = np.clip(np.floor(x).astype(int), 0, W - 2), np.clip(np.floor(y).astype(int), 0, H - 2)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    t = texture.astype(np.float64)
    return (t[y0, x0] * (1 - fx) + t[y0, x0 + 1] * fx) * (1 - fy) + (t[y0 + 1, x0] * (1 - fx) + t[y0 + 1, x0 + 1] * fx) * fy


def check_closest_tex(rgb, hit, dist, points, quad, colours, texture):
    flat = quad != 1
    assert np.array_equal(rgb[flat], colours[quad[flat]])                              # that face's colour, exactly
    want = bilinear64(texture, hit[~flat, 1] + 0.5, hit[~flat, 2] + 0.5)
    err = float(np.abs(rgb[~flat] - want).max())
    print(f"closest_tex: max |rgb - bilinear texel| on +x = {err / EPS:.2f} eps (bound 16 eps)")
    assert err <= 16 * EPS
    assert np.abs(dist[:, 0] - 0.3).max() <= 4 * EPS
    expect = points.copy()
    expect[np.arange(points.shape[0]), quad // 2] = np.where(quad % 2 == 1, 0.5, -0.5)
    assert np.abs(hit - expect).max() <= 4 * EPS
