"""Helper, not a test: a numpy restatement of the mesh-to-SDF contract (include/shacira_hip.h, shacira_mesh_sdf) in
np.float32, one rounding per operator, vectorised over (points, triangles) in blocks; and the meshes, the point batch and the
bit view that the mesh tests share."""
import numpy as np

F32 = np.float32
H, K = F32(0.707106781), F32(0.577350269)
Z, ONE = F32(0.0), F32(1.0)
DIRECTIONS = ((ONE, Z, Z), (Z, ONE, Z), (Z, Z, ONE),
              (Z, H, H), (H, Z, H), (H, H, Z),
              (Z, H, -H), (H, Z, -H), (H, -H, Z),
              (K, K, K), (-K, K, K), (K, -K, K), (K, K, -K))
BLOCK_PAIRS = 1 << 19


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross(x, y):
    return (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])


def _edge_d2(e, x, p):
    t0, t1, t2 = e[0] * x - p[0], e[1] * x - p[1], e[2] * x - p[2]
    return (t0 * t0 + t1 * t1) + t2 * t2


def mesh_sdf_ref(points, triangles, unsigned=False):
    """sdf [N] float32 of the contract; ``unsigned``: the distance without the ray-stabbing sign."""
    points = np.ascontiguousarray(points, dtype=F32)
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    N, T = points.shape[0], tri.shape[0]
    out = np.full((N,), np.inf, dtype=F32)
    if N == 0 or T == 0:
        return out
    with np.errstate(all="ignore"):
        a, b, c = ([tri[None, :, v, k] for k in range(3)] for v in range(3))
        e0 = [b[k] - a[k] for k in range(3)]
        e1 = [c[k] - b[k] for k in range(3)]
        e2 = [a[k] - c[k] for k in range(3)]
        n = _cross(e0, e2)
        m = [_cross(e, n) for e in (e0, e1, e2)]
        r = [ONE / _dot(e, e) for e in (e0, e1, e2)]
        rn = ONE / _dot(n, n)
        valid = (n[0] != 0) | (n[1] != 0) | (n[2] != 0)
        g = [-e2[k] for k in range(3)]
        per_dir = []
        for d in DIRECTIONS:
            w = _cross(d, g)
            det = _dot(e0, w)
            det64 = det.astype(np.float64)
            per_dir.append((d, w, ONE / det, ~((det64 > -1e-8) & (det64 < 1e-8))))
        block = max(1, BLOCK_PAIRS // T)
        for start in range(0, N, block):
            p = [points[start:start + block, k, None] for k in range(3)]
            p0 = [p[k] - a[k] for k in range(3)]
            p1 = [p[k] - b[k] for k in range(3)]
            p2 = [p[k] - c[k] for k in range(3)]
            s = (np.copysign(ONE, _dot(m[0], p0)) + np.copysign(ONE, _dot(m[1], p1))) + np.copysign(ONE, _dot(m[2], p2))
            edge = [_edge_d2(e, np.fmax(Z, np.fmin(_dot(e, pi) * ri, ONE)), pi)
                    for e, pi, ri in ((e0, p0, r[0]), (e1, p1, r[1]), (e2, p2, r[2]))]
            h = _dot(n, p0)
            d2 = np.where(s < 2, np.fmin(edge[0], np.fmin(edge[1], edge[2])), (h * h) * rn)
            d2 = np.where(d2 < 0, Z, d2)
            least = np.fmin.reduce(np.where(valid, d2, F32(np.inf)), axis=1, initial=F32(np.inf))
            dist = np.sqrt(least.astype(F32))
            assert dist.dtype == F32 and d2.dtype == F32
            if unsigned:
                out[start:start + block] = dist
                continue
            q = _cross(p0, e0)
            tau = _dot(g, q)
            inside = np.ones(dist.shape, dtype=bool)
            for d, w, inv, live in per_dir:
                u = _dot(p0, w) * inv
                v = _dot(d, q) * inv
                t = tau * inv
                assert u.dtype == F32 and v.dtype == F32 and t.dtype == F32
                hit = live & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1))
                inside &= (hit & (t >= 0)).any(axis=1) & (hit & ~(t >= 0)).any(axis=1)
            out[start:start + block] = np.where(inside, -dist, dist)
    return out


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def icosphere(level, radius=1.0):
    """(V float32 [10 * 4^level + 2, 3], F int64 [20 * 4^level, 3]): an icosahedron subdivided ``level`` times, vertices
    pushed to ``radius`` (in fp64, then rounded), outward-facing."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    V = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[key] = len(V) - 1
            return mid[key]
        for i, j, k in F:
            ij, jk, ki = midpoint(i, j), midpoint(j, k), midpoint(k, i)
            out += [(i, ij, ki), (j, jk, ij), (k, ki, jk), (ij, jk, ki)]
        F = out
    return (np.asarray(V) * radius).astype(F32), np.asarray(F, dtype=np.int64)


def cube(half=0.5):
    """(V [8, 3], F [12, 3]): the axis-aligned cube [-half, half]^3, two triangles per face, outward-facing."""
    V = np.asarray([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    F = [tri for q in quads for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return V, np.asarray(F, dtype=np.int64)


def soup(num_triangles=37, seed=0, scale=0.5):
    """float32 [T, 3, 3]: random triangles in [-1, 1]^3 of edge ~``scale``; triangle 1 has two equal vertices and triangle 2
    three (both degenerate: n == 0)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, size=(num_triangles, 1, 3))
    tri = (centre + rng.uniform(-scale, scale, size=(num_triangles, 3, 3))).astype(F32)
    if num_triangles > 2:
        tri[1, 1] = tri[1, 0]
        tri[2, 1] = tri[2, 0]
        tri[2, 2] = tri[2, 0]
    return tri


def lattice(n=9):
    """The n^3 lattice of [-1, 1]^3, float32 [n^3, 3] (n = 9: points exactly on the cube's faces, edges and planes)."""
    ax = np.linspace(-1.0, 1.0, n).astype(F32)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)


def box_sdf(points, half=0.5):
    """Exact signed distance to the cube [-half, half]^3 in fp64."""
    q = np.abs(np.asarray(points, dtype=np.float64)) - half
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)


# ---- what the mesh tests share ----------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 4099)
_POINTS = np.random.default_rng(21).uniform(-1, 1, (SIZES[-1], 3)).astype(F32)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def _triangles(name):
    if name == "one":
        return np.asarray([[[-0.4, -0.3, 0.1], [0.5, -0.2, -0.1], [0.1, 0.6, 0.2]]], dtype=F32)
    if name == "cube":
        V, F = cube(0.5)
        return V[F]
    if name == "cube x6":
        V, F = cube(0.5)
        return np.tile(V[F], (6, 1, 1))
    if name == "soup":
        return soup(37, seed=3)
    level, radius = {"ico2": (2, 0.7), "ico4": (4, 0.7), "ico5+1": (5, 0.7)}[name]
    V, F = icosphere(level, radius)
    tri = V[F]
    if name == "ico5+1":      # one more (degenerate: a point) than a multiple of the chunk granule, across two passes
        tri = np.concatenate([tri, np.full((1, 3, 3), 0.25, dtype=F32)])
    return tri
