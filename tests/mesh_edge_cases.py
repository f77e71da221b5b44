"""Helper, not a test: the deterministic inputs that tests/test_mesh_edges_cpu.py, tests/test_gpu_mesh_edges.py and
tests/test_gpu_mesh_voxelize_edges.py share. The distance, closest-point and voxelise kernels decide on exact comparisons
(the sign of a zero, s == 2, E0 == E1, u == 0, u + v == 1, t == 0, d2 == 0, f == 0, s == rN); uniform random inputs never
land on one. These builders put the inputs there, and on the edges of the kernels' partitions (include/shacira_hip.h:
passes of SHACIRA_MESH_SDF_PASS_TRIANGLES, chunks of SHACIRA_MESH_SDF_CHUNK_GRANULE; mesh_sdf.hip: 512 points per workgroup;
mesh_voxelize.hip: 32 counts per scan thread, 2^30 units per pair launch). The CPU file proves that each case is what it
claims; the GPU files hold the kernels to the restatements on them."""
import numpy as np

import mesh_closest_ref as cref
import mesh_sdf_ref as ref
from mesh_sdf_ref import F32, _POINTS
from shacira_amd import _lib

PASS = _lib.MESH_SDF_PASS_TRIANGLES
SOUP_SIZES = (31, 32, 33, 64, 65)          # around the chunk granule: T <= 32 is always one chunk
BLOCK_SIZES = (256, 257, 511, 512, 513)    # around the 256 lanes and the 512 points of a workgroup
ONE_CHUNK_N = 2047 * 512 + 1               # the smallest N whose point blocks alone fill the chip: one chunk per pass


# ---- distance and closest point -------------------------------------------------------------------------------------------
def special_base(mesh):
    """float32 [B, 3]: for "cube" (and "cube x6") lattice(9), points exactly on the faces, edges, vertices and diagonal planes
    of the cube; for "ico2" its 162 vertices, the midpoint of edge a-b of every face and every centroid (802 points)."""
    if mesh.startswith("cube"):
        return ref.lattice(9)
    V, F = ref.icosphere(2, 0.7)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return np.concatenate([V, (a + b) * F32(0.5), ((a + b) + c) / F32(3.0)]).astype(F32)


def special_points(mesh):
    """float32 [7 B, 3]: ``special_base`` and, per coordinate, a copy with that coordinate one ulp up and one with it one ulp
    down, so that every sign plane the base points lie on is straddled (around 0 the neighbours are denormals)."""
    base = special_base(mesh)
    out = [base]
    for k in range(3):
        for towards in (np.inf, -np.inf):
            moved = base.copy()
            moved[:, k] = np.nextafter(base[:, k], F32(towards))
            out.append(moved)
    return np.concatenate(out)


def pair_d2(points, triangles):
    """(d2 float32 [N, T] of the contract, +inf where the triangle is no candidate or d2 is a NaN)."""
    points = np.ascontiguousarray(points, dtype=F32)
    tri = np.ascontiguousarray(triangles, dtype=F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        v = [[tri[None, :, i, k] for k in range(3)] for i in range(3)]
        e, n, m, r, rn = cref._triangle_terms(*v)
        p = [points[:, k, None] for k in range(3)]
        pi, s, x, E = cref._pair_terms(p, v, e, m, r)
        h = ref._dot(n, pi[0])
        d2 = np.where(s < 2, np.fmin(E[0], np.fmin(E[1], E[2])), (h * h) * rn)
        d2 = np.where(d2 < 0, ref.Z, d2)
        valid = (n[0] != 0) | (n[1] != 0) | (n[2] != 0)
        return np.where(valid & ~np.isnan(d2), d2, cref.INF)


def soup_of(T):
    assert T in SOUP_SIZES
    return ref.soup(T, seed=3)


_ICO5 = []


def pass_mesh(extra):
    """The first PASS + ``extra`` triangles of the icosphere of level 5 (an open cap of it): extra = 0 fills one pass exactly,
    extra = 1 leaves the last triangle alone in the second."""
    if not _ICO5:
        V, F = ref.icosphere(5, 0.7)
        _ICO5.append(V[F])
    assert _ICO5[0].shape[0] > PASS + extra
    return _ICO5[0][:PASS + extra]


def pass_points(n=65):
    """``_POINTS[:n]`` with the last row aimed at the centroid of triangle PASS of ``pass_mesh(1)``, which then wins it."""
    last = pass_mesh(1)[PASS]
    points = _POINTS[:n].copy()
    points[n - 1] = ((last[0] + last[1]) + last[2]) / F32(3.0)
    return points


def one_chunk_points():
    """float32 [ONE_CHUNK_N, 3] uniform in the cube, the last row aimed as in ``pass_points``; and the 512 rows the
    restatement is evaluated on: 0, N - 2, N - 1 and 509 others."""
    points = np.random.default_rng(24).uniform(-1, 1, (ONE_CHUNK_N, 3)).astype(F32)
    points[-1] = pass_points()[-1]
    subset = np.random.default_rng(25).choice(ONE_CHUNK_N - 3, 512, replace=False) + 1
    subset[:3] = (0, ONE_CHUNK_N - 2, ONE_CHUNK_N - 1)
    return points, subset


SLIVERS = ("needle 1e-20", "needle 1e-12", "near-collinear", "collinear")


def slivers():
    """name -> float32 [3, 3]. The needles sit at the origin with two edges of the given length along x and y: n = (0, 0,
    -len^2) is a denormal (1e-40) or tiny (1e-24), dot(n, n) underflows to 0 and r_n = +inf, the m_i underflow to zeros whose
    signs sgn() reads; both are valid. The near-collinear triangle has n ~ 3e-8. The collinear one has three distinct vertices
    on a line through the origin and n == 0 exactly (every product is exact): no candidate."""
    def needle(length):
        return np.asarray([[0, 0, 0], [length, 0, 0], [0, length, 0]], dtype=F32)
    near = np.asarray([[0.1, 0.2, 0.3], [0.4, 0.2, 0.3], [0.25, 0.2 + 1e-7, 0.3]], dtype=F32)
    line = np.asarray([[0.125, 0.25, 0.5], [0.25, 0.5, 1.0], [0.375, 0.75, 1.5]], dtype=F32) * F32(0.5)
    return dict(zip(SLIVERS, (needle(1e-20), needle(1e-12), near, line)))


def sliver_mesh():
    """(soup(37, seed=3) with the slivers mixed in [T = 41, 3, 3], name -> index). The 1e-20 needle comes first of the two, so
    that among equal d2 it is the one that wins."""
    soup, s = ref.soup(37, seed=3), slivers()
    order = [(4, "collinear"), (9, "needle 1e-20"), (20, "near-collinear"), (30, "needle 1e-12")]
    parts, index, at = [], {}, 0
    for before, name in order:
        parts += [soup[at:before], s[name][None]]
        index[name] = before + len(index)
        at = before
    tri = np.concatenate(parts + [soup[at:]])
    assert tri.shape[0] == 41 and all(np.array_equal(tri[i], s[name]) for name, i in index.items())
    return tri, index


def sliver_points():
    """float32 [94, 3]: ``_POINTS[:65]``, of which one lies nearer the origin than the soup; 26 points around the origin, one
    per sign pattern (zeros included: dot(e, p) == 0 meets r_i = +inf), so that each needle wins some; and three points
    on, above and beside the near-collinear triangle."""
    signs = np.asarray([s for s in np.ndindex(3, 3, 3) if s != (1, 1, 1)], dtype=F32) - F32(1.0)
    near = np.asarray([[0.2, 0.2, 0.3], [0.25, 0.2, 0.35], [0.25, 0.1, 0.3]], dtype=F32)
    return np.concatenate([_POINTS[:65], signs * np.asarray([0.03125, 0.04, 0.05], dtype=F32), near])


NON_FINITE_ROWS = (7, 20, 41)


def non_finite():
    """(points [65, 3], finite triangles [37, 3, 3], all triangles [39, 3, 3], bool [65]: the finite rows). The points are
    ``_POINTS[:65]`` with one NaN coordinate (row 7), one +inf coordinate (row 20) and one row of 3e38, whose every d2
    overflows. The triangles are soup(37, seed=3), then one all-NaN triangle (n is a NaN, which is != 0: a candidate whose d2
    is a NaN) and one with vertices at 1e30."""
    points = _POINTS[:65].copy()
    points[7, 1] = np.nan
    points[20, 0] = np.inf
    points[41] = 3e38
    finite = np.ones(65, dtype=bool)
    finite[list(NON_FINITE_ROWS)] = False
    soup = ref.soup(37, seed=3)
    far = np.asarray([[1e30, 0, 0], [0, 1e30, 0], [0, 0, 1e30]], dtype=F32)
    return points, soup, np.concatenate([soup, np.full((1, 3, 3), np.nan, dtype=F32), far[None]]), finite


# ---- voxelise ---------------------------------------------------------------------------------------------------------------
DYADIC_LEVELS = (1, 3, 5)
DYADIC_MARGINS = (0.0, 0.25, 0.5, 1.0)


def _from_grid_units(g, level):
    """Grid units (multiples of 0.5 up to G) to cube coordinates, exactly; the kernel's (v + 1) * (G / 2) gives g back."""
    return (np.asarray(g, dtype=np.float64) * (2.0 / (1 << level)) - 1.0).astype(F32)


def dyadic_triangles(level):
    """float32 [5, 3, 3], axis-aligned, every grid-unit coordinate a multiple of 0.5, so that every operation of the contract
    is exact and the touching cases (f == 0, s == +-rN, i + 0.5 == max + H) are hit exactly: in the cell-face plane x = G / 2
    with vertices on grid lines; in the plane x = G / 2 + 0.5 through cell centres; in the boundary planes x = +1 and x = -1
    (grid units G and 0); and one in z = 0.5 with a vertex on the cell centre (0.5, 0.5, 0.5)."""
    G = 1 << level
    h = G / 2

    def in_x(x):
        return [[x, 0, 0], [x, G, h], [x, h, G]]
    centre = [[0.5, 0.5, 0.5], [G - 0.5, 1, 0.5], [1, G - 0.5, 0.5]]
    return _from_grid_units([in_x(h), in_x(h + 0.5), in_x(G), in_x(0), centre], level)


def beyond_the_boundary(level):
    """The x = +1 triangle of ``dyadic_triangles`` with x = nextafter(1, 2): v + 1 rounds to 2, so in grid units the plane IS
    the boundary and the restatement marks the last layer of cells, where fp64 (g > G) marks none at margin 0. The contract's
    rounding, not a bug: a restatement-only case."""
    tri = dyadic_triangles(level)[2:3].copy()
    tri[:, :, 0] = np.nextafter(F32(1.0), F32(2.0))
    return tri


def tiny(count, seed, size=0.01):
    """``count`` triangles of extent ``size`` (a cell of level 5 is 0.0625 wide) at uniform places in the cube: the ``_tiny``
    of test_gpu_mesh_voxelize.py."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.98, 0.98, (count, 1, 3))
    return (centre + rng.uniform(-size, size, (count, 3, 3))).astype(F32)


EMPTIES_SIZES = (1, 31, 32, 33, 1025)


def _invalid(t, kind):
    t = t.copy()
    if kind == 0:
        t[1] = t[0]                    # degenerate
    elif kind == 1:
        t[2, 0] = np.nan               # a NaN vertex
    else:
        t += F32(2.5)                  # wholly outside
    return t


def empties(T, padded):
    """(float32 [T (+ 80), 3, 3], bool: which are invalid): T tiny triangles, every third one invalid, in turn degenerate,
    with a NaN vertex, wholly outside the cube; ``padded``: 40 more invalid ones in front and 40 behind. A scan thread owns 32
    counts, so thread 0 then owns only empties, and so does the thread that owns the tail."""
    assert T in EMPTIES_SIZES
    tri = tiny(T, 30 + T)
    bad = np.zeros(T, dtype=bool)
    for i in range(2, T, 3):
        tri[i] = _invalid(tri[i], (i // 3) % 3)
        bad[i] = True
    if padded:
        pad = np.stack([_invalid(t, i % 3) for i, t in enumerate(tiny(80, 29))])
        tri = np.concatenate([pad[:40], tri, pad[40:]])
        bad = np.concatenate([np.ones(40, dtype=bool), bad, np.ones(40, dtype=bool)])
    return tri, bad


FULL_GRID_COUNT, FULL_GRID_SPLIT = 33, 17


def full_grid_triangles():
    """float32 [33, 3, 3]: large tilted triangles that reach beyond the cube on every axis, so that the clipped bounding box of
    each is the whole grid: G^2 columns of G / 32 words, 2^25 units at level 10."""
    rng = np.random.default_rng(31)
    base = np.asarray([[-3.0, -2.0, -2.5], [3.0, -1.5, 2.5], [0.25, 3.0, 0.25]])
    tri = base[None] + rng.uniform(-0.2, 0.2, (FULL_GRID_COUNT, 3, 3))
    tri[:, :, 2] += np.linspace(-0.5, 0.5, FULL_GRID_COUNT)[:, None]
    return tri.astype(F32)


def level10_triangles():
    """float32 [2001, 3, 3]: 2000 tiny triangles (about ten cells of level 10 across) and one of about 0.3 extent."""
    return np.concatenate([tiny(2000, 32), tiny(1, 33, size=0.15)])
