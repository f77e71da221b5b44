"""Deterministic edge coordinates for the triplane and octree operators, shared by the CPU restatement tests and the GPU
edge suites (tests/test_gpu_triplane_edges.py, tests/test_gpu_octree_edges.py). Everything is built from the LODs / levels
of a call and a seed; nothing here touches a device.

Triplane families (one value per sample and axis, mixed within a sample):
  lattice    c = -1 + 2 k / R for a LOD of the call (R = 2^lod) with k in [-3 R, 4 R] (exact in fp32 for R <= 1024), and
             np.nextafter of it to either side
  unit       +-1, +-(1 - 2^-24), +-0.0, +-1e-40
  far        +-{3, 5, 7, 7.5, 1000.25, 65537, 1e6} and uniform draws in +-8
  inside     uniform draws in +-1
  nonfinite  NaN, +-inf, and 3e38 where every LOD of the call has R >= 4 (the unnormalised index overflows to inf there;
             at R < 4 it stays finite with floor(index / span) >= 2^24, where the parity of the kernel's (int) cast is
             not defined: left out, as every such magnitude is)
"""
import numpy as np

import octree_ref as oref
import triplane_ref as tr

TRIPLANE_FAR = (3.0, 5.0, 7.0, 7.5, 1000.25, 65537.0, 1e6)
TRIPLANE_UNIT = (1.0, 1.0 - 2.0 ** -24, 0.0, 1e-40)
MIN_BATCH = 1537          # the batch the preconditions are asserted on; a smaller N takes its first rows

# (F, lods, batch sizes): tests/test_gpu_triplane_edges.py
TRIPLANE_CASES = [
    (1, (0,), (1, 511, 512, 513, 1537)),          # nbins == 1, N around the sort's chunk
    (4, (5, 6, 7, 8), ((1 << 14) + 3,)),          # production shape
    (3, (8, 3), (5003,)),                         # runtime F, descending LODs
    (5, (7, 3, 7), (5003,)),                      # repeated LOD
    (8, (3, 9), (20011,)),                        # 32 768 bins: global-counter path, windows with R < nb
    (16, (10,), (20011,)),                        # nb == 64 exactly
    (20, (6, 10), (20011,)),                      # nb capped, finest window does not fit
    (32, (4, 6), (3001,)),                        # widest F
]


def _signed(rng, values, n):
    v = np.asarray(values, dtype=np.float32)[rng.integers(0, len(values), n)]
    return np.where(rng.integers(0, 2, n) == 1, -v, v).astype(np.float32)


def triplane_values(lods, n, rng, nonfinite=True):
    """n fp32 values, one family each."""
    fam = rng.choice(6, n, p=[0.30, 0.10, 0.12, 0.25, 0.19, 0.04])
    out = np.empty(n, dtype=np.float32)
    # lattice
    R = (1 << np.asarray(lods, dtype=np.int64))[rng.integers(0, len(lods), n)]
    k = np.floor(rng.uniform(0, 1, n) * (7 * R + 1)).astype(np.int64) - 3 * R
    lat = (-1.0 + 2.0 * k / R).astype(np.float32)
    assert np.all(lat.astype(np.float64) == -1.0 + 2.0 * k / R)              # exact in fp32
    side = rng.integers(0, 3, n)
    lat = np.where(side == 1, np.nextafter(lat, np.float32(np.inf)), np.where(side == 2, np.nextafter(lat, np.float32(
        -np.inf)), lat))
    pools = [lat, _signed(rng, TRIPLANE_UNIT, n), _signed(rng, TRIPLANE_FAR, n),
             rng.uniform(-8, 8, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)]
    for f, pool in enumerate(pools):
        out[fam == f] = pool[fam == f]
    nf = [np.nan, np.inf, -np.inf] + ([3e38, -3e38] if min(lods) >= 2 else [])
    sel = fam == 5
    out[sel] = np.asarray(nf, dtype=np.float32)[rng.integers(0, len(nf), n)][sel] if nonfinite else pools[4][sel]
    return out


def triplane_coords(lods, n, seed, nonfinite=True):
    """fp32 [n, 3]: the first n rows of a batch of at least MIN_BATCH samples (the one ``triplane_reach`` counts on)."""
    rng = np.random.default_rng(seed)
    full = max(int(n), MIN_BATCH)
    return triplane_values(lods, 3 * full, rng, nonfinite).reshape(full, 3)


def triplane_reach(coords, lods):
    """Samples (any axis, any LOD of the call) that reach each branch, from the restatement alone:
    {'flips>=2', 'negative and odd flip', 'zero weight', 'on a border', 'largest finite flips'}."""
    coords = np.asarray(coords, dtype=np.float32)
    n = coords.shape[0]
    many, negodd, zero, border = (np.zeros(n, dtype=bool) for _ in range(4))
    top = 0.0
    for lod in lods:
        S = (1 << lod) + 1
        flips, neg, refl = tr.reflect_info(coords, S, np.float32)
        fin = np.isfinite(flips)
        top = max(top, float(flips[fin].max()) if fin.any() else 0.0)
        with np.errstate(invalid="ignore"):
            many |= (fin & (flips >= 2)).any(1)
            negodd |= (fin & neg & (np.fmod(flips, 2) == 1)).any(1)
            border |= (fin & ((refl == 0) | (refl == S - 1))).any(1)
        for a, b in tr.PLANE_AXES:
            ix, _ = tr._index(coords[:, a], S, np.float32, True)
            iy, _ = tr._index(coords[:, b], S, np.float32, True)
            xs, ys, ws = tr._corners(ix, iy, np.float32)
            for x, y, w in zip(xs, ys, ws):
                zero |= (x >= 0) & (x < S) & (y >= 0) & (y < S) & (w == 0)
    return {"flips>=2": int(many.sum()), "negative and odd flip": int(negodd.sum()), "zero weight": int(zero.sum()),
            "on a border": int(border.sum()), "largest finite flips": top}


def assert_triplane_reach(coords, lods, n=None):
    """The preconditions of the edge suite on a batch of at least MIN_BATCH samples. ``n``: the rows that are sent when the
    batch is cut short; from 511 rows on, the head itself holds the same minima scaled by n / MIN_BATCH."""
    reach = triplane_reach(coords, lods)
    assert coords.shape[0] >= MIN_BATCH
    assert reach["flips>=2"] >= 100 and reach["negative and odd flip"] >= 100 and reach["zero weight"] >= 100, reach
    assert reach["on a border"] >= 32, reach
    assert reach["largest finite flips"] < 2.0 ** 24, reach        # the parity of the (int) cast is defined
    if n is not None and 511 <= n < coords.shape[0]:
        head = triplane_reach(coords[:n], lods)
        most, few = (100 * n) // MIN_BATCH, (32 * n) // MIN_BATCH
        assert min(head["flips>=2"], head["negative and odd flip"], head["zero weight"]) >= most, (n, head)
        assert head["on a border"] >= few, (n, head)
    return reach


# ---- octree ------------------------------------------------------------------------------------------------------------------
# -1 - 2^-24 is no fp32 number (it rounds to -1): the first fp32 value below -1 stands for "just outside".
OCTREE_BELOW = np.nextafter(np.float32(-1), np.float32(-2))
OCTREE_TOP = np.float32(1.0 - 2.0 ** -24)            # c + 1 rounds to 2: outside


def octree_face_values(level):
    """c = -1 + 2 k / G, k = 0..G (exact in fp32)."""
    G = 1 << level
    return (-1.0 + 2.0 * np.arange(G + 1) / G).astype(np.float32)


def octree_pool(levels):
    """Every special value of the octree edge suite as one fp32 array: cell faces of every level with their neighbours,
    the cube's borders, zeros, denormals, outside and non-finite values."""
    vals = []
    for level in sorted(set(levels)):
        f = octree_face_values(level)
        vals += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    vals.append(np.asarray([-1.0, OCTREE_BELOW, OCTREE_TOP, 0.0, -0.0, 1e-40, -1e-40, 1.3, -1.3, 3e38, np.nan, np.inf,
                            -np.inf], dtype=np.float32))
    return np.concatenate(vals)


def assert_octree_landing(levels):
    """Each special value lands where the suite says, from ``octree_ref.locate`` alone."""
    def loc(v, level):
        c = np.zeros((np.size(v), 3), dtype=np.float32)
        c[:, 0] = v
        inside, cell, t = oref.locate(c, level)
        return inside, cell[:, 0], t[:, 0]

    for level in levels:
        G = 1 << level
        inside, cell, t = loc(octree_face_values(level), level)
        assert inside[:G].all() and not inside[G]                        # the face k = G is c = 1: outside
        assert np.array_equal(cell[:G], np.arange(G)) and np.all(t[:G] == 0)
        inside, cell, t = loc(np.float32(-1), level)
        assert inside[0] and cell[0] == 0 and t[0] == 0
        assert not loc(OCTREE_BELOW, level)[0][0] and not loc(OCTREE_TOP, level)[0][0]
        for v in (0.0, -0.0, 1e-40, -1e-40):
            inside, cell, t = loc(np.float32(v), level)
            assert inside[0] and cell[0] == G // 2 and t[0] == (0.0 if level else 0.5)
        for v in (1.3, -1.3, 3e38, np.nan, np.inf, -np.inf):
            assert not loc(np.float32(v), level)[0][0]


# (levels, F, occupancies of the finest level): tests/test_gpu_octree_edges.py. dense only at level <= 5; "far" = the single
# cell (G-1, G-1, G-1), whose corners end in the last, partial word of the corner bit grid; "first" = the cell (0, 0, 0)
OCTREE_CASES = [
    ((0,), 4, ("dense",)),
    ((0, 1), 2, ("dense", "far", "first")),
    ((6, 2), 4, ("shell", "far", "first")),
    ((5, 5), 1, ("dense", "shell", "far", "first")),
    ((3, 7), 3, ("shell", "far", "first")),            # runtime F, windows in the backward
    ((5, 6, 7, 8), 5, ("shell", "far", "first")),
]


def _pool_rows(pool, cells, fine, coarse, rng):
    """Rows that hold every pool value once. A value that some occupied cell holds on an axis -- at the finest level, or
    else at the coarsest level of the call -- gets a row of its own: the value on that axis (the axes take turns), the other
    two inside such a cell, so that the sample can hit. The values no occupied cell holds on the axis (most of them, when a
    single cell is occupied) cannot hit wherever the other axes are: they go three to a row, one per axis."""
    cells = np.asarray(cells)
    G, sh = 1 << fine, fine - coarse
    m = pool.shape[0]
    axis = np.arange(m) % 3
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.floor((pool.astype(np.float64) + 1.0) * (G / 2))
    k = np.where(np.isfinite(k) & (k >= 0) & (k < G), k, -(1 << 20)).astype(np.int64)
    pick = np.zeros(m, dtype=np.int64)
    can = np.zeros(m, dtype=bool)
    for shift in (sh, 0):                                   # the coarsest level first, a cell of the finest level wins
        for a in range(3):
            order = np.argsort(cells[:, a] >> shift, kind="stable")
            along = cells[order, a] >> shift
            lo, hi = np.searchsorted(along, k >> shift, "left"), np.searchsorted(along, k >> shift, "right")
            has = (axis == a) & (hi > lo)
            pick[has] = order[lo[has] + rng.integers(0, np.maximum(hi - lo, 1))[has]]
            can |= has
    own = (-1.0 + 2.0 * (cells[pick[can]] + rng.uniform(0.05, 0.95, (int(can.sum()), 3))) / G).astype(np.float32)
    own[np.arange(own.shape[0]), axis[can]] = pool[can]
    rest = pool[~can]
    rest = np.concatenate([rest, np.repeat(rest[-1:], (-rest.shape[0]) % 3)]) if rest.shape[0] else rest
    return np.concatenate([own, rest.reshape(-1, 3)])


def octree_coords(levels, cells, n, seed):
    """fp32 [n, 3]. ``cells``: occupied cells of the finest level, int [C, 3]. A batch of MIN_BATCH samples or more holds the
    whole pool of special values (``octree_pool``, placed by ``_pool_rows``; ``assert_octree_pool_present`` proves it on the
    batch); a shorter one holds an evenly spaced part of those rows, a third of the batch at most. They sit at rows spread
    over the batch by a fixed permutation. Of the rows left, a third lies inside an occupied cell with a face of that cell,
    or a neighbour value, on some axes; a third mixes the pool's values per axis with draws inside the cube; the rest is
    uniform in +-1.1."""
    rng = np.random.default_rng(seed)
    fine = max(levels)
    G = 1 << fine
    pool = octree_pool(levels)
    out = rng.uniform(-1.1, 1.1, (n, 3)).astype(np.float32)
    kind = rng.integers(0, 3, n)
    mixed = np.where(rng.integers(0, 2, (n, 3)) == 1, pool[rng.integers(0, pool.shape[0], (n, 3))],
                     rng.uniform(-1, 1, (n, 3)).astype(np.float32))
    out[kind == 1] = mixed[kind == 1]
    pick = np.asarray(cells)[rng.integers(0, len(cells), n)].astype(np.float64)
    u = rng.uniform(0, 1, (n, 3))
    how = rng.integers(0, 6, (n, 3))
    u = np.where(how == 0, 0.0, np.where(how == 1, 1.0, u))              # the cell's own faces (the upper one: next cell)
    inside = (-1.0 + 2.0 * (pick + u) / G).astype(np.float32)
    inside = np.where(how == 2, np.nextafter(inside, np.float32(np.inf)), np.where(how == 3, np.nextafter(
        inside, np.float32(-np.inf)), inside))
    out[kind == 2] = inside[kind == 2]
    rows = _pool_rows(pool, cells, fine, min(levels), rng)
    if n < MIN_BATCH:
        rows = rows[np.linspace(0, rows.shape[0] - 1, min(rows.shape[0], n // 3)).astype(np.int64)]
    assert rows.shape[0] <= n
    out[rng.permutation(n)[:rows.shape[0]]] = rows
    return out


def assert_octree_pool_present(coords, levels):
    """Every value of ``octree_pool(levels)`` is a coordinate of the batch: every face of every level with both fp32
    neighbours, the borders, both zeros, both denormals, the outside values, NaN and both infinities."""
    pool = octree_pool(levels)
    coords = np.asarray(coords, dtype=np.float32)
    assert coords.shape[0] >= MIN_BATCH
    finite = pool[np.isfinite(pool)]
    missing = finite[~np.isin(finite, coords)]
    assert missing.size == 0, missing
    assert np.isnan(coords).any() and (coords == np.inf).any() and (coords == -np.inf).any()
    zero = coords == 0
    assert (zero & np.signbit(coords)).any() and (zero & ~np.signbit(coords)).any()      # isin cannot tell -0.0 from 0.0
    tiny = np.float32(1e-40)
    assert tiny != 0 and (coords == tiny).any() and (coords == -tiny).any()
    return pool.shape[0]
