"""numpy restatement of the shacira_mesh_voxelize contract (include/shacira_hip.h): the same fp32 operation sequence, one
rounding per operator, so the cell set is reproduced EXACTLY: dense (``mesh_voxelize_ref``) and, by the same formulas, as
sorted keys (``mesh_voxelize_keys``) for the levels whose G^3 cells do not fit. Also the meshes and an fp64 separating-axis
test the tests share. Written from the contract alone."""
import numpy as np

from mesh_sdf_ref import cube, icosphere  # noqa: F401  (the shared meshes)

F32 = np.float32


def _cross(x, y):
    return (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])


def _boxes(triangles, level, margin):
    """Per valid triangle with a non-empty clipped bounding box: (lo int64 [3], hi int64 [3], bool [hi - lo + 1]: the cells of
    the box that the contract sets), in the order of the triangles."""
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    G = 1 << level
    half = F32(0.5) * F32(G)
    H = F32(0.5) + F32(margin)
    with np.errstate(all="ignore"):
        for t in tri:
            a, b, c = t
            n = _cross(b - a, a - c)
            if not (n[0] != 0 or n[1] != 0 or n[2] != 0):
                continue
            P = (t + F32(1.0)) * half                     # [vertex, component]
            if not np.isfinite(P).all():
                continue
            E = (P[1] - P[0], P[2] - P[1], P[0] - P[2])
            N = _cross(E[0], E[1])
            rN = H * ((abs(N[0]) + abs(N[1])) + abs(N[2]))
            lo = np.maximum(np.ceil((P.min(axis=0) - H) - F32(0.5)), F32(0.0))
            hi = np.minimum(np.floor((P.max(axis=0) + H) - F32(0.5)), F32(G - 1))
            if not (lo <= hi).all():
                continue
            lo, hi = lo.astype(np.int64), hi.astype(np.int64)
            p = [(np.arange(lo[k], hi[k] + 1).astype(F32) + F32(0.5)) for k in range(3)]
            p = [p[0][:, None, None], p[1][None, :, None], p[2][None, None, :]]
            s = (N[0] * (p[0] - P[0, 0]) + N[1] * (p[1] - P[0, 1])) + N[2] * (p[2] - P[0, 2])
            ok = (s >= -rN) & (s <= rN)
            for k in range(3):
                u, v = (k + 1) % 3, (k + 2) % 3
                sigma = F32(1.0) if N[k] >= 0 else F32(-1.0)
                for i in range(3):
                    mu, mv = -sigma * E[i][v], sigma * E[i][u]
                    r = H * (abs(mu) + abs(mv))
                    f = (mu * (p[u] - P[i, u]) + mv * (p[v] - P[i, v])) + r
                    ok = ok & (f >= 0)
            yield lo, hi, ok


def mesh_voxelize_ref(triangles, level, margin):
    """bool [G, G, G], indexed [x][y][z]: the cells the contract sets."""
    G = 1 << level
    grid = np.zeros((G, G, G), dtype=bool)
    for lo, hi, ok in _boxes(triangles, level, margin):
        grid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] |= ok
    return grid


def mesh_voxelize_keys(triangles, level, margin):
    """int64, sorted and unique: the keys (x * G + y) * G + z of the cells the contract sets -- ``mesh_voxelize_ref`` by the
    same formulas without the G^3 cells, so that the deepest levels have a reference."""
    G = 1 << level
    keys = [np.zeros(0, dtype=np.int64)]
    for lo, hi, ok in _boxes(triangles, level, margin):
        x, y, z = np.nonzero(ok)
        keys.append(((x + lo[0]) * G + (y + lo[1])) * G + (z + lo[2]))
    return np.unique(np.concatenate(keys))


def words_of_keys(keys):
    """(word index int64 [W] ascending, uint32 [W]): the non-zero words of ``pack_words`` from sorted unique keys."""
    word, inverse = np.unique(keys >> 5, return_inverse=True)
    bits = np.zeros(word.shape[0], dtype=np.uint32)
    np.bitwise_or.at(bits, inverse, np.uint32(1) << (keys & 31).astype(np.uint32))
    return word, bits


def unit_counts(triangles, level, margin):
    """int64 [T]: the column words of every triangle -- the (x, y) columns of its clipped bounding box times the 32-bit words
    its z range touches -- 0 for an invalid triangle or an empty box. The box does not depend on the overlap test."""
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    G = 1 << level
    half = F32(0.5) * F32(G)
    H = F32(0.5) + F32(margin)
    out = np.zeros(tri.shape[0], dtype=np.int64)
    with np.errstate(all="ignore"):
        for j, t in enumerate(tri):
            n = _cross(t[1] - t[0], t[0] - t[2])
            P = (t + F32(1.0)) * half
            if not (n[0] != 0 or n[1] != 0 or n[2] != 0) or not np.isfinite(P).all():
                continue
            lo = np.maximum(np.ceil((P.min(axis=0) - H) - F32(0.5)), F32(0.0))
            hi = np.minimum(np.floor((P.max(axis=0) + H) - F32(0.5)), F32(G - 1))
            if (lo <= hi).all():
                lo, hi = lo.astype(np.int64), hi.astype(np.int64)
                out[j] = (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * ((hi[2] >> 5) - (lo[2] >> 5) + 1)
    return out


def pack_words(grid):
    """uint32 [ceil(G^3 / 32)]: bit key & 31 of word key >> 5, key = (x * G + y) * G + z."""
    flat = grid.reshape(-1)
    words = (flat.size + 31) // 32
    bits = np.zeros(words * 32, dtype=np.uint64)
    bits[:flat.size] = flat
    return (bits.reshape(words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def sat_f64(triangles, level, half_extent):
    """bool [G, G, G]: the 13-axis separating-axis test in fp64, in its textbook form (projection intervals of the triangle
    and of the cube on every axis, closed), for cubes of ``half_extent`` cells around the cell centres, clipped to the grid.
    Degenerate and non-finite triangles mark nothing."""
    tri = np.asarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    G = 1 << level
    grid = np.zeros((G, G, G), dtype=bool)
    centres = np.stack(np.meshgrid(*([np.arange(G) + 0.5] * 3), indexing="ij"), axis=-1).reshape(-1, 3)
    eye = np.eye(3)
    h = float(half_extent)
    for t in tri:
        if not np.isfinite(t).all():
            continue
        P = (t + 1.0) * (G / 2)
        E = np.stack([P[1] - P[0], P[2] - P[1], P[0] - P[2]])
        N = np.cross(E[0], E[1])
        if not N.any():
            continue
        axes = [eye[0], eye[1], eye[2], N] + [np.cross(E[i], eye[k]) for i in range(3) for k in range(3)]
        ok = np.ones(centres.shape[0], dtype=bool)
        for ax in axes:
            proj = P @ ax
            c = centres @ ax
            r = h * np.abs(ax).sum()
            ok &= (proj.min() <= c + r) & (proj.max() >= c - r)
        grid |= ok.reshape(G, G, G)
    return grid


def generic_rotation():
    """A fixed rotation with no axis-aligned direction: Rz(0.37) Ry(0.51) Rx(0.23)."""
    def rot(axis, angle):
        c, s = np.cos(angle), np.sin(angle)
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    return rot(2, 0.37) @ rot(1, 0.51) @ rot(0, 0.23)


def rotated_icosphere(level, radius=0.7):
    """float32 [T, 3, 3]: ``icosphere(level, radius)`` turned by ``generic_rotation``."""
    V, Fc = icosphere(level, radius)
    V = (V.astype(np.float64) @ generic_rotation().T).astype(F32)
    return V[Fc]


def random_triangles(count=64, seed=5, extent=1.2):
    """float32 [count, 3, 3] with vertices uniform in [-extent, extent]^3: some reach outside the cube."""
    return np.random.default_rng(seed).uniform(-extent, extent, (count, 3, 3)).astype(F32)
