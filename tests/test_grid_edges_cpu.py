"""The yardsticks of the triplane and octree edge suites, held on the CPU: the error scales ``backward_scale`` of
tests/triplane_ref.py and tests/octree_ref.py (count and A = sum |w g| per texel / table entry), the reflection helper, the
fp32-index restatement against torch's fp32 CPU grid_sample on far and lattice coordinates, and the preconditions of every
batch of tests/grid_edge_cases.py that the GPU suites run."""
import numpy as np
import pytest
import torch

import grid_edge_cases as ge
import octree_ref as oref
import triplane_ref as tr
from shacira_amd.wisp.accelstructs import OctreeAS
from shacira_amd.wisp.ops import octree as octree_ops
from test_triplane_cpu import _torch_triplane

EPS = float(np.finfo(np.float32).eps)


# ---- triplane --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdim,lods", [(2, (0,)), (3, (4, 2)), (1, (3, 1, 3)), (4, (5, 6))])
@pytest.mark.parametrize("summed", [True, False])
def test_triplane_abs_sum_is_the_backward_of_absolute_values(fdim, lods, summed):
    rng = np.random.default_rng(fdim + len(lods))
    coords = ge.triplane_coords(lods, 700, 3)[:700]
    sides = [(1 << l) + 1 for l in lods]
    planes = [[rng.standard_normal((fdim, S, S)).astype(np.float32) for _ in range(3)] for S in sides]
    go = rng.standard_normal((700, 3 * fdim * (1 if summed else len(lods)))).astype(np.float32)
    scale = tr.backward_scale(coords, sides, fdim, go, summed, index_dtype=np.float32)
    gabs, _, _ = tr.backward(coords, planes, np.abs(go), summed, index_dtype=np.float32)   # the weights are >= 0
    gref, _, _ = tr.backward(coords, planes, go, summed, index_dtype=np.float32)
    for l in range(len(lods)):
        for p in range(3):
            count, asum = scale[l][p]
            np.testing.assert_allclose(asum, gabs[l][p], rtol=1e-13, atol=0)
            assert np.all(np.abs(gref[l][p]) <= asum * (1 + 1e-12))
            assert np.all(asum[:, count == 0] == 0) and count.shape == (sides[l], sides[l])


def test_triplane_count_equals_a_brute_force_loop():
    lods, fdim = (3, 1), 2
    coords = ge.triplane_coords(lods, 64, 9)[:64]
    go = np.ones((64, 3 * fdim), dtype=np.float32)
    scale = tr.backward_scale(coords, [9, 3], fdim, go, True, index_dtype=np.float32)
    touched = 0
    for l, S in enumerate([9, 3]):
        for p, (a, b) in enumerate(tr.PLANE_AXES):
            want = np.zeros((S, S), dtype=np.int64)
            wsum = np.zeros((S, S))
            for i in range(64):
                ix, _ = tr._index(coords[i:i + 1, a], S, np.float32, True)
                iy, _ = tr._index(coords[i:i + 1, b], S, np.float32, True)
                x0, y0 = int(np.floor(ix[0])), int(np.floor(iy[0]))
                for dy in (0, 1):
                    for dx in (0, 1):
                        if 0 <= x0 + dx < S and 0 <= y0 + dy < S:
                            want[y0 + dy, x0 + dx] += 1
                            fx = np.float32(ix[0] - np.float32(x0)) if dx else np.float32(np.float32(x0 + 1) - ix[0])
                            fy = np.float32(iy[0] - np.float32(y0)) if dy else np.float32(np.float32(y0 + 1) - iy[0])
                            wsum[y0 + dy, x0 + dx] += float(np.float32(fx * fy))
            count, asum = scale[l][p]
            assert np.array_equal(count, want)
            np.testing.assert_allclose(asum[0], wsum, rtol=1e-13, atol=0)      # g = 1: A is the sum of the fp32 weights
            touched += int(want.sum())
    assert touched > 300


def test_reflect_info_names_the_branches():
    S = 9                                                  # R = 8: x = (c + 1) * 4
    c = np.asarray([0.25, 3.0, -3.0, -4.0, 5.5, 1.0, -1.0, np.nan, np.inf], dtype=np.float32)
    flips, neg, refl = tr.reflect_info(c, S)
    assert np.array_equal(flips[:7], [0, 2, 1, 1, 3, 1, 0]) and not np.isfinite(flips[7:]).any()
    assert np.array_equal(neg, [False, False, True, True, False, False, False, False, False])
    assert np.array_equal(refl[:7], [5, 0, 8, 4, 6, 8, 0])  # before the clip; x = 8 is one flip that lands on the far border
    mult = tr.coord_mult(c, S)
    assert np.array_equal(mult[:7], [4, 0, 0, 4, -4, 0, 0])
    idx, _ = tr._index(c[:7], S, np.float32, False)         # the forward's clipped index is the same point
    assert np.array_equal(idx, [5, 0, 8, 4, 6, 8, 0])


@pytest.mark.parametrize("lod", [0, 3, 6, 10])
def test_fp32_index_restatement_matches_torch_fp32_on_far_and_lattice_coordinates(lod):
    """The GPU suites' reference on their own inputs (finite ones: torch's CPU kernel is not the contract for NaN / inf):
    lattice points out to k in [-3R, 4R] with their neighbours, magnitudes up to 1e6, uniform draws in +-8."""
    rng = np.random.default_rng(lod)
    coords = ge.triplane_coords((lod,), 3000, 20 + lod, nonfinite=False)
    reach = ge.assert_triplane_reach(coords, (lod,))
    assert float(np.abs(coords).max()) == 1e6 and reach["largest finite flips"] >= 5e5 - 1
    S = (1 << lod) + 1
    planes = [[rng.standard_normal((2, S, S)).astype(np.float32) for _ in range(3)]]
    out = _torch_triplane(torch.tensor(coords), [[torch.tensor(p[None]) for p in planes[0]]], True).numpy()
    ref = tr.forward(coords, planes, True, index_dtype=np.float32)
    scale = tr.abs_forward(coords, planes, True, index_dtype=np.float32)
    assert np.all(np.abs(out - ref) <= 4 * EPS * scale + 1e-30)


@pytest.mark.parametrize("fdim,lods,sizes", ge.TRIPLANE_CASES)
def test_every_triplane_edge_batch_reaches_its_branches(fdim, lods, sizes):
    for n in sizes:
        coords = ge.triplane_coords(lods, n, 1000 + n)
        reach = ge.assert_triplane_reach(coords, lods, n)
        assert np.isnan(coords).any() and np.isinf(coords).any(), reach


# ---- octree ----------------------------------------------------------------------------------------------------------------
def _octree_problem(levels, fdim, n, seed, summed):
    rng = np.random.default_rng(seed)
    cells = oref.shell_cells(max(levels))
    index = octree_ops.build_octree_index(OctreeAS.from_quantized_points(torch.from_numpy(cells), max(levels)), levels)
    lp = [index[l].level_points.numpy() for l in levels]
    trk = [index[l].trinkets.numpy() for l in levels]
    tables = [rng.standard_normal((index[l].rows + 1, fdim)).astype(np.float32) for l in levels]
    coords = ge.octree_coords(levels, cells, n, seed)
    go = rng.standard_normal((n, fdim * (1 if summed else len(levels)))).astype(np.float32)
    return lp, trk, tables, coords, go


@pytest.mark.parametrize("summed", [True, False])
def test_octree_abs_sum_is_the_backward_of_absolute_values(summed):
    levels = [4, 2]
    lp, trk, tables, coords, go = _octree_problem(levels, 3, 900, 4, summed)
    rows = [t.shape[0] for t in tables]
    scale = oref.backward_scale(coords, levels, lp, trk, rows, go, summed)
    gabs, _, _ = oref.backward(coords, levels, lp, trk, tables, np.abs(go), summed, weight_dtype=np.float32)
    gref, _, _ = oref.backward(coords, levels, lp, trk, tables, go, summed, weight_dtype=np.float32)
    for l in range(len(levels)):
        count, asum = scale[l]
        np.testing.assert_allclose(asum, gabs[l], rtol=1e-13, atol=0)         # the weights are >= 0
        assert np.all(np.abs(gref[l]) <= asum * (1 + 1e-12))
        assert count[-1] == 0 and np.all(asum[-1] == 0) and np.all(asum[count == 0] == 0)
        assert int(count.sum()) % 8 == 0 and int(count.sum()) > 800


def test_octree_count_equals_a_brute_force_loop():
    levels = [3]
    lp, trk, tables, coords, go = _octree_problem(levels, 1, 64, 7, True)
    count, asum = oref.backward_scale(coords, levels, lp, trk, [tables[0].shape[0]], np.ones((64, 1), np.float32), True)[0]
    want = np.zeros(tables[0].shape[0], dtype=np.int64)
    wsum = np.zeros(tables[0].shape[0])
    cellrow = {tuple(c): i for i, c in enumerate(lp[0].tolist())}
    for i in range(64):
        c = coords[i]
        if not np.all(np.isfinite(c)):
            continue
        with np.errstate(over="ignore"):
            p = (c + np.float32(1)) * np.float32(4)
        fl = np.floor(p)
        if np.any(fl < 0) or np.any(fl >= 8) or tuple(int(v) for v in fl) not in cellrow:
            continue
        t = p - fl                                                            # fp32
        for k in range(8):
            w = np.float32(1)
            for a in range(3):
                w = np.float32(w * (t[a] if oref.CORNERS[k, a] else np.float32(1) - t[a]))
            row = trk[0][cellrow[tuple(int(v) for v in fl)], k]
            want[row] += 1
            wsum[row] += float(w)
    assert np.array_equal(count, want) and want.sum() >= 8 * 16
    np.testing.assert_allclose(asum[:, 0], wsum, rtol=1e-13, atol=0)


def test_octree_fp32_weights_are_the_fp64_weights_to_rounding():
    t = np.random.default_rng(1).uniform(0, 1, (500, 3)).astype(np.float32).astype(np.float64)
    t[:3] = [[0, 0, 0], [0, 0.5, 1 - 2.0 ** -24], [2.0 ** -24, 2.0 ** -30, 0.75]]
    w64, w32 = oref.weights(t), oref.weights(t, np.float32)
    assert np.all(np.abs(w32 - w64) <= 6 * 2.0 ** -24 * w64)                  # 1 - t once per axis, two products
    assert np.array_equal(w32, w32.astype(np.float32).astype(np.float64))


def test_octree_special_values_land_where_the_suite_says():
    ge.assert_octree_landing(range(0, 9))
    pool = ge.octree_pool([0, 3])
    assert np.isnan(pool).any() and np.isinf(pool).any() and np.signbit(pool[pool == 0]).any()


@pytest.mark.parametrize("levels,fdim,occupancies", ge.OCTREE_CASES)
def test_every_octree_edge_batch_holds_every_special_value(levels, fdim, occupancies):
    """The N = 1537 batch of every case carries the whole pool -- every face of every level with both neighbours, the
    borders, zeros, denormals, outside and non-finite values -- and enough of its rows lie in occupied cells."""
    G = 1 << max(levels)
    for occ in occupancies:
        cells = (oref._all_cells(max(levels)) if occ == "dense" else oref.shell_cells(max(levels)) if occ == "shell"
                 else np.full((1, 3), G - 1 if occ == "far" else 0, dtype=np.int64))
        coords = ge.octree_coords(levels, cells, 1537, 104)
        assert ge.assert_octree_pool_present(coords, levels) == sum(3 * ((1 << l) + 1) for l in set(levels)) + 13
        inside, cell, _ = oref.locate(coords, max(levels))
        assert int((oref.cell_rank(cells, max(levels), cell, inside) >= 0).sum()) >= 1537 // 8
        for n, seed in ((511, 101), (512, 102), (513, 103)):
            short = ge.octree_coords(levels, cells, n, seed)
            inside, cell, _ = oref.locate(short, max(levels))
            assert int((oref.cell_rank(cells, max(levels), cell, inside) >= 0).sum()) >= n // 8
