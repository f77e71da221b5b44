"""Helper, not a test: a numpy restatement of the mesh point-sampling contract (include/shacira_hip.h, shacira_mesh_sample):
Philox4x32-10 in uint64 arithmetic, the integer CDF of the face areas and its search rule, the point formulas in np.float32 one
operator at a time, the Gaussian displacement in fp64 from the same words, and the narrowband keep rule."""
import numpy as np

F32 = np.float32
SURFACE, NEAR, CUBE, CELLS = 0, 1, 2, 3
BLOCK = 256
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
KNOWN_ANSWERS = (          # (counter, key, output): the known-answer vectors of Random123's Philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays: ten rounds on the counter (c0..c3) under the key (k0, k1); operands broadcast."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2           # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def sample_words(n, seed, segment=0, index_base=0):
    """uint32 [n, 8]: the eight words of samples 0 .. n - 1 (draw 0, then draw 1)."""
    idx = np.uint64(index_base) + np.arange(n, dtype=np.uint64)
    lo, hi = idx & MASK, idx >> np.uint64(32)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    return np.stack(philox4x32_10(lo, hi, 0, segment, k0, k1) + philox4x32_10(lo, hi, 1, segment, k0, k1), axis=1)


def unit(w):
    """U(w) in [0, 1), float32 (exact)."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def unit1(w):
    """U1(w) in (0, 1], float32 (exact)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)) + np.uint32(1)).astype(F32) * F32(2.0 ** -24)


def face_normals(triangles):
    """cross(a - b, b - c) in float32, one rounding per operator: [T, 3]."""
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    x, y = tri[:, 0] - tri[:, 1], tri[:, 1] - tri[:, 2]
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                     x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)


def face_areas64(triangles):
    """Twice the face areas in fp64 from the fp32 edge differences (the products of fp32 values are exact in fp64)."""
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    x, y = (tri[:, 0] - tri[:, 1]).astype(np.float64), (tri[:, 1] - tri[:, 2]).astype(np.float64)
    nx, ny, nz = x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]
    return np.sqrt((nx * nx + ny * ny) + nz * nz)


def face_cdf(triangles):
    """uint32 [T]: cdf[t] = min(floor(sum[t] / sum[T - 1] * 2^32), 2^32 - 1), the running sum in fp64 in index order. None
    when the total area is zero (or not finite)."""
    run = np.cumsum(face_areas64(triangles))
    if run.shape[0] == 0 or not (run[-1] > 0) or not np.isfinite(run[-1]):
        return None
    return np.minimum(np.floor(run / run[-1] * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)


def face_of(cdf, w):
    """The face of every word: the first t with cdf[t] > min(w, cdf[T - 1] - 1)."""
    cdf = np.asarray(cdf, dtype=np.uint32).astype(np.int64)
    w = np.minimum(np.asarray(w, dtype=np.uint32).astype(np.int64), (cdf[-1] - 1) & 0xFFFFFFFF)
    return np.minimum(np.searchsorted(cdf, w, side="right"), cdf.shape[0] - 1).astype(np.int32)


def face_word_counts(cdf):
    """How many of the 2^32 words each face owns under the rule of ``face_of`` (python ints)."""
    c = [int(v) for v in cdf]
    counts = [c[t] - (c[t - 1] if t else 0) for t in range(len(c))]
    last = max(t for t in range(len(c)) if counts[t] > 0)
    counts[last] += (1 << 32) - c[-1]
    return counts


def gaussians64(words):
    """fp64 [n, 3]: the Box-Muller normals of words 4..7 of every row, from the same fp32 uniforms as the kernel."""
    g = np.asarray(words, dtype=np.uint32)[:, 4:8]
    r0 = np.sqrt(-2.0 * np.log(unit1(g[:, 0]).astype(np.float64)))
    r1 = np.sqrt(-2.0 * np.log(unit1(g[:, 2]).astype(np.float64)))
    a0, a1 = 2.0 * np.pi * unit(g[:, 1]).astype(np.float64), 2.0 * np.pi * unit(g[:, 3]).astype(np.float64)
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=1)


def keep_mask(points, occupancy_words, level):
    """bool [n]: OctreeAS.query's pidx > -1 against the packed words of ``level``."""
    G = 1 << level
    p = np.asarray(points, dtype=F32)
    with np.errstate(invalid="ignore"):
        cell = np.floor((F32(G) * (p + F32(1.0))) / F32(2.0))
        inside = ((cell >= 0) & (cell < G)).all(axis=1)
    q = np.where(inside[:, None], np.nan_to_num(cell, nan=0.0), 0).astype(np.int64)
    key = (q[:, 0] * G + q[:, 1]) * G + q[:, 2]
    words = np.asarray(occupancy_words).view(np.uint32)
    return inside & (((words[key >> 5] >> (key & 31).astype(np.uint32)) & 1) != 0)


def pack_occupancy(grid):
    """uint32 words of a bool [G, G, G] grid indexed [x][y][z]: bit (key & 31) of word (key >> 5)."""
    bits = np.asarray(grid, dtype=bool).reshape(-1)
    padded = np.zeros(((bits.shape[0] + 31) // 32) * 32, dtype=np.uint64)
    padded[:bits.shape[0]] = bits
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def make_samples(mode, n, seed=0, segment=0, index_base=0, words=None, triangles=None, cdf=None, sigma=0.0, corners=None,
                 samples_per_cell=1, cell_level=0):
    """dict(points float32 [n, 3], normals float32 [n, 3], face int32 [n], words uint32 [n, 8], points64): sample i of the
    contract for every i. NEAR: ``points`` adds the fp64 Gaussian rounded to float32 (compare with a tolerance) and
    ``points64`` keeps the fp64 sum."""
    w = sample_words(n, seed, segment, index_base) if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    assert w.shape == (n, 8)
    out = dict(words=w, normals=np.zeros((n, 3), dtype=F32), face=np.full((n,), -1, dtype=np.int32), points64=None)
    if mode == CUBE:
        out["points"] = unit(w[:, :3]) * F32(2.0) - F32(1.0)
    elif mode == CELLS:
        c = np.asarray(corners, dtype=np.int16)[np.arange(n) // samples_per_cell, :3].astype(F32)
        width = F32(2.0) / F32(1 << cell_level)
        out["points"] = (c * width - F32(1.0)) + unit(w[:, :3]) * width
    else:
        tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
        t = face_of(face_cdf(tri) if cdf is None else cdf, w[:, 0])
        a, b, c = tri[t, 0], tri[t, 1], tri[t, 2]
        u, v = np.sqrt(unit(w[:, 1]))[:, None], unit(w[:, 2])[:, None]
        assert u.dtype == F32 and v.dtype == F32
        p = ((F32(1.0) - u) * a + (u * (F32(1.0) - v)) * b) + (u * v) * c
        assert p.dtype == F32
        out["face"], out["normals"] = t, face_normals(tri)[t]
        if mode == NEAR:
            out["points64"] = p.astype(np.float64) + float(F32(sigma)) * gaussians64(w)
            p = out["points64"].astype(F32)
        out["points"] = p
    assert out["points"].dtype == F32
    return out
