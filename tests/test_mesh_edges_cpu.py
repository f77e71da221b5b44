"""The inputs of the mesh edge suites (tests/mesh_edge_cases.py), held on the CPU: every case is what it claims to be -- the
special positions do produce zeros, ties and negative values, the slivers are candidates or not as stated, the non-finite rows
come out of the restatement as the contract states, every empty triangle has no work unit -- and the references the GPU files
compare with are sound on their own: the sparse voxel restatement equals the dense one, and on dyadic axis-aligned triangles,
where every fp32 operation is exact, the restatement equals the fp64 separating-axis test cell for cell."""
import numpy as np
import pytest

import mesh_closest_ref as cref
import mesh_edge_cases as me
import mesh_sdf_ref as ref
import mesh_voxelize_ref as vref
from mesh_sdf_ref import _POINTS, _bits, _triangles
from test_gpu_mesh_voxelize import _CASES, MARGINS, _tiny


# ---- distance and closest point -------------------------------------------------------------------------------------------
def test_the_lattice_against_the_cube_has_zeros_ties_and_inside_points():
    points, tri = me.special_base("cube"), _triangles("cube")
    assert points.shape == (729, 3)
    sdf = ref.mesh_sdf_ref(points, tri)
    d2 = me.pair_d2(points, tri)
    tied = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2
    assert int((sdf == 0).sum()) == 98 and int((sdf < 0).sum()) == 27 and int(tied.sum()) == 621
    assert np.array_equal(np.sqrt(d2.min(axis=1)), np.abs(sdf))
    moved = me.special_points("cube")
    assert moved.shape == (7 * 729, 3) and np.array_equal(moved[:729], points)
    assert int((moved != np.tile(points, (7, 1))).sum()) == 6 * 729           # one coordinate each, by one ulp
    assert np.abs(moved.astype(np.float64) - np.tile(points, (7, 1))).max() == 2.0 ** -23       # the ulp above 1
    assert (np.abs(moved[moved != 0]) < 1e-44).any()                          # the neighbours of 0 are denormals
    assert np.array_equal(me.special_points("cube x6"), moved)


def test_the_icosphere_points_lie_on_the_icosphere():
    points, tri = me.special_base("ico2"), _triangles("ico2")
    assert points.shape == (802, 3) and tri.shape[0] == 320
    sdf = ref.mesh_sdf_ref(points, tri)
    assert int((sdf == 0).sum()) == 190 and bool((sdf[:162] == 0).all())
    assert float(np.abs(sdf).max()) <= 1e-7
    moved = ref.mesh_sdf_ref(me.special_points("ico2"), tri)
    assert (moved < 0).any() and (moved > 0).any() and (moved == 0).any()


def test_slivers_are_candidates_or_not_as_stated():
    s = me.slivers()
    tri, index = me.sliver_mesh()
    valid = cref.candidates(tri)
    assert [bool(valid[index[name]]) for name in me.SLIVERS] == [True, True, True, False]
    with np.errstate(all="ignore"):
        for name, n2 in (("needle 1e-20", 1e-40), ("needle 1e-12", 1e-24)):
            t = s[name]
            n = np.asarray(ref._cross(t[1] - t[0], t[0] - t[2]))
            assert n[0] == 0 and n[1] == 0 and abs(float(n[2]) + n2) <= 1e-3 * n2
            assert ref._dot(n, n) == 0 and np.isposinf(ref.ONE / ref._dot(n, n))
        assert 0 < abs(float(s["needle 1e-20"][1, 0]) ** 2) < float(np.finfo(np.float32).tiny)      # n is a denormal
        t = s["near-collinear"]
        n = np.asarray(ref._cross(t[1] - t[0], t[0] - t[2]))
        assert 1e-8 < float(np.abs(n).max()) < 1e-7
    line = s["collinear"]
    assert len({tuple(v) for v in line.tolist()}) == 3
    points = me.sliver_points()
    for signed in (True, False):
        dist, hit, tidx = cref.mesh_closest_ref(points, tri, signed=signed)
        wins = {name: int((tidx == i).sum()) for name, i in index.items()}
        assert wins["needle 1e-20"] >= 1 and wins["needle 1e-12"] >= 1 and wins["near-collinear"] >= 1, wins
        assert wins["collinear"] == 0 and int(tidx.min()) >= 0
    d2 = me.pair_d2(points, tri)
    assert np.isinf(d2[:, index["collinear"]]).all()
    assert np.isinf(d2[:, index["needle 1e-20"]]).any()                        # 0 * inf over the face: a NaN never wins


def test_non_finite_rows_come_out_as_the_contract_states():
    points, soup, tri, finite = me.non_finite()
    assert tuple(np.nonzero(~finite)[0]) == me.NON_FINITE_ROWS and tri.shape[0] == 39
    assert np.isnan(points[7]).sum() == 1 and np.isposinf(points[20]).sum() == 1 and (points[41] == np.float32(3e38)).all()
    assert cref.candidates(tri)[37] and cref.candidates(tri)[38]               # NaN != 0 and inf != 0
    plain = cref.mesh_closest_ref(points, soup, signed=False)
    for dist, hit, tidx in (plain, cref.mesh_closest_ref(points, tri, signed=False)):
        assert np.isposinf(dist[~finite]).all() and (tidx[~finite] == -1).all()
        assert np.array_equal(hit[~finite], points[~finite], equal_nan=True)
        assert np.isfinite(dist[finite]).all() and (tidx[finite] >= 0).all() and (tidx < 37).all()
        # the NaN and 1e30 triangles change no bit of the other 62 rows
        assert np.array_equal(_bits(dist[finite]), _bits(plain[0][finite])) and np.array_equal(tidx[finite], plain[2][finite])
        assert np.array_equal(_bits(hit[finite]), _bits(plain[1][finite]))


def test_the_last_triangle_of_the_pass_edge_mesh_wins_its_point():
    assert me.pass_mesh(0).shape[0] == me.PASS and me.pass_mesh(1).shape[0] == me.PASS + 1
    points = me.pass_points()
    assert points.shape == (65, 3) and np.array_equal(points[:64], _POINTS[:64])
    tidx = cref.mesh_closest_ref(points, me.pass_mesh(1), signed=False)[2]
    assert tidx[64] == me.PASS and (tidx[:64] < me.PASS).all()
    big, subset = me.one_chunk_points()
    assert big.shape == (2047 * 512 + 1, 3) and np.array_equal(big[-1], points[64])
    assert len(set(subset.tolist())) == 512 and {0, big.shape[0] - 2, big.shape[0] - 1} <= set(subset.tolist())


@pytest.mark.parametrize("T", me.SOUP_SIZES)
def test_the_small_soups_keep_their_degenerate_triangles(T):
    valid = cref.candidates(me.soup_of(T))
    assert valid.shape == (T,) and not valid[1] and not valid[2] and int(valid.sum()) == T - 2


# ---- voxelise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("name", sorted(_CASES))
def test_sparse_restatement_equals_the_dense_one(name, margin):
    tri, level = _CASES[name]()
    dense = vref.mesh_voxelize_ref(tri, level, margin)
    keys = vref.mesh_voxelize_keys(tri, level, margin)
    assert keys.dtype == np.int64 and np.array_equal(keys, np.nonzero(dense.reshape(-1))[0])
    word, bits = vref.words_of_keys(keys)
    want = vref.pack_words(dense)
    assert np.array_equal(word, np.nonzero(want)[0]) and np.array_equal(bits, want[word])


@pytest.mark.parametrize("margin", me.DYADIC_MARGINS)
@pytest.mark.parametrize("level", me.DYADIC_LEVELS)
def test_on_dyadic_triangles_the_restatement_is_the_fp64_test(level, margin):
    """Grid-unit coordinates are multiples of 0.5 up to 32, H of 0.25: every product and sum of the contract fits 24 bits, so
    nothing rounds and the touching cells are decided exactly. Equality, not the band of test_mesh_voxelize_cpu.py."""
    tri = me.dyadic_triangles(level)
    G = 1 << level
    g = (tri.astype(np.float64) + 1.0) * (G / 2)
    assert np.array_equal(g * 2, np.round(g * 2)) and g.min() == 0 and g.max() == G
    assert (g[0, :, 0] == G / 2).all() and (g[1, :, 0] == G / 2 + 0.5).all() and (g[2, :, 0] == G).all()
    assert (g[3, :, 0] == 0).all() and (g[4, 0] == 0.5).all()
    for part in (tri, *(tri[i:i + 1] for i in range(5))):
        got = vref.mesh_voxelize_ref(part, level, margin)
        assert got.any() and np.array_equal(got, vref.sat_f64(part, level, 0.5 + margin))
    # the boundary planes mark the outermost layer of cells and, at margin 0, nothing else
    if margin == 0.0:
        for i, layer in ((2, G - 1), (3, 0)):
            got = vref.mesh_voxelize_ref(tri[i:i + 1], level, margin)
            assert got[layer].any() and not np.delete(got, layer, axis=0).any()


def test_a_plane_one_ulp_beyond_the_boundary_rounds_onto_it():
    """Restatement only: v + 1 rounds 2 + 2^-23 to 2, so the contract sees the plane x = G and marks the last layer; fp64
    sees it outside every closed cell. The contract's rounding, stated here so that nobody extends the equality above."""
    tri = me.beyond_the_boundary(3)
    assert (tri[:, :, 0] > 1).all()
    got = vref.mesh_voxelize_ref(tri, 3, 0.0)
    assert int(got.sum()) == 43 and int(got[7].sum()) == 43
    assert not vref.sat_f64(tri, 3, 0.5).any()
    assert np.array_equal(got, vref.mesh_voxelize_ref(me.dyadic_triangles(3)[2:3], 3, 0.0))


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("T", me.EMPTIES_SIZES)
def test_every_invalid_triangle_of_the_empties_has_no_unit(T, padded):
    tri, bad = me.empties(T, padded)
    assert tri.shape[0] == T + (80 if padded else 0) and int(bad.sum()) == T // 3 + (80 if padded else 0)
    units = vref.unit_counts(tri, 5, 0.5)
    assert np.array_equal(units == 0, bad)
    if padded:
        assert bad[:40].all() and bad[-40:].all() and not units[:32].any() and not units[-32:].any()
        inner = me.empties(T, False)[0]
        assert np.array_equal(vref.mesh_voxelize_ref(tri, 5, 0.5), vref.mesh_voxelize_ref(inner, 5, 0.5))
    assert vref.mesh_voxelize_ref(tri, 5, 0.5).any()


def test_tiny_is_the_tiny_of_the_voxelise_suite():
    assert np.array_equal(me.tiny(50, 10), _tiny(50, 10))
    assert np.array_equal(me.tiny(5, 13, size=0.05), _tiny(5, 13, size=0.05))


def test_unit_counts_and_the_full_grid_triangles():
    tri = me.full_grid_triangles()
    assert tri.shape == (me.FULL_GRID_COUNT, 3, 3)
    units = vref.unit_counts(tri, 10, 0.0)
    assert (units == 1 << 25).all()
    split = me.FULL_GRID_SPLIT
    assert int(units[:split].sum()) < 1 << 30 and int(units[split:].sum()) < 1 << 30 < int(units.sum())
    # the counts against the boxes of the restatement on a small level, where every box can be looked at
    for lo, hi, ok in vref._boxes(tri[:3], 5, 0.0):
        assert (lo == 0).all() and (hi == 31).all() and ok.any() and not ok.all()
    some = np.concatenate([vref.random_triangles(), me.empties(33, False)[0]])
    boxes = list(vref._boxes(some, 6, 0.5))
    counts = vref.unit_counts(some, 6, 0.5)
    assert len(boxes) == int((counts > 0).sum())
    for (lo, hi, ok), c in zip(boxes, counts[counts > 0]):
        assert c == ok.shape[0] * ok.shape[1] * len({z >> 5 for z in range(lo[2], hi[2] + 1)})


def test_the_level_10_case_reaches_the_top_of_the_key_range():
    tri = me.level10_triangles()
    assert tri.shape == (2001, 3, 3)
    keys = vref.mesh_voxelize_keys(tri, 10, 0.5)
    assert keys.shape[0] > 100_000 and int(keys.max()) >= 1 << 29 and int(keys.max()) < 1 << 30
    assert (np.diff(keys) > 0).all()
    assert int(vref.unit_counts(tri, 10, 0.5).max()) > 10_000                  # the large one: many columns of several words
