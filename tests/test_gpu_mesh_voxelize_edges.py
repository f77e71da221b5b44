"""Mesh voxelisation on the MI355X at its edges: ``hip_ops.mesh_voxelize`` (mesh_voxelize.hip) against the numpy restatement
(tests/mesh_voxelize_ref.py) on the inputs of tests/mesh_edge_cases.py. Words and grid are compared exactly, as in
test_gpu_mesh_voxelize.py's test_kernel_equals_the_restatement. What each case is is tests/test_mesh_edges_cpu.py's subject;
wall times are in profiles/mesh_edges.md.

  dyadic triangles   axis-aligned, in cell-face, cell-centre and boundary planes: f == 0, s == +-rN and i + 0.5 == max + H are
                     met exactly, and the restatement there IS the fp64 separating-axis test
  empties in a pass  triangles without work units at the front, in the middle and at the tail of the scan
  levels 7 to 10     keys up to 2^30; the deepest level against the sparse form of the restatement
  2^30 units         the second pair launch of a pass (unit_base > 0)
"""
import numpy as np
import pytest
import torch

import mesh_edge_cases as me
import mesh_voxelize_ref as vref
from test_gpu_mesh_voxelize import _CASES, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _check(tri, level, margin, dev, want=None):
    want = vref.mesh_voxelize_ref(tri, level, margin) if want is None else want
    words, grid = _run(tri, level, margin, dev)
    assert np.array_equal(grid, want)
    assert np.array_equal(words, vref.pack_words(want))
    return want


@pytest.mark.parametrize("margin", me.DYADIC_MARGINS)
@pytest.mark.parametrize("level", me.DYADIC_LEVELS)
def test_dyadic_triangles(dev, level, margin):
    tri = me.dyadic_triangles(level)
    assert _check(tri, level, margin, dev).any()
    for i in range(tri.shape[0]):                                # each alone, too: the OR of five hides a missing cell
        assert _check(tri[i:i + 1], level, margin, dev).any()


@pytest.mark.parametrize("margin", me.DYADIC_MARGINS)
def test_a_plane_one_ulp_beyond_the_boundary(dev, margin):
    tri = me.beyond_the_boundary(3)
    want = _check(tri, 3, margin, dev)
    assert int(want[7].sum()) == 43 if margin == 0.0 else want[7].any()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("T", me.EMPTIES_SIZES)
def test_empties_in_a_pass(dev, T, padded):
    tri, bad = me.empties(T, padded)
    assert bad[:40].all() and bad[-40:].all() if padded else not bad[0]
    assert _check(tri, 5, 0.5, dev).any()


_SPANNING = _CASES["spanning@6"]()[0]


@pytest.mark.parametrize("level", [7, 8])
@pytest.mark.parametrize("name", ["ico2", "spanning"])
def test_levels_7_and_8(dev, name, level):
    tri = vref.rotated_icosphere(2) if name == "ico2" else _SPANNING
    assert _check(tri, level, 0.5, dev).any()


def _expected_words(keys, level, dev):
    """int32 [G^3 / 32] on the device from sorted unique keys."""
    word, bits = vref.words_of_keys(keys)
    out = torch.zeros(((1 << (3 * level)) // 32,), dtype=torch.int32, device=dev)
    out[torch.from_numpy(word).to(dev)] = torch.from_numpy(bits.view(np.int32)).to(dev)
    return out


def test_level_10_against_the_sparse_restatement(dev):
    from shacira_amd import hip_ops
    tri = me.level10_triangles()
    keys = vref.mesh_voxelize_keys(tri, 10, 0.5)
    assert int(keys.max()) >= 1 << 29
    words, grid = hip_ops.mesh_voxelize(torch.from_numpy(tri).to(dev), 10, 0.5, with_grid=False)
    assert grid is None and words.dtype == torch.int32 and tuple(words.shape) == (1 << 25,)
    assert torch.equal(words, _expected_words(keys, 10, dev))


def test_more_than_2_to_the_30_units_in_a_pass(dev):
    """33 triangles of 2^25 column words each: the pass has 33 * 2^25 > 2^30 units and takes a second pair launch with
    unit_base = 2^30, which starts in the middle of triangle 32's units. The halves [0, 17) and [17, 33) stay below 2^30
    on the single-launch path that the cases above pin; the OR of their words is the whole."""
    from shacira_amd import hip_ops
    tri = me.full_grid_triangles()
    split = me.FULL_GRID_SPLIT
    units = vref.unit_counts(tri, 10, 0.0)
    assert (units == 1 << 25).all() and tri.shape[0] == 33
    assert split << 25 < 1 << 30 < 33 << 25 and (33 - split) << 25 < 1 << 30
    assert int(units[:split].sum()) == split << 25 and int(units.sum()) == 33 << 25
    t = torch.from_numpy(tri).to(dev)
    whole = hip_ops.mesh_voxelize(t, 10, 0.0, with_grid=False)[0]
    first = hip_ops.mesh_voxelize(t[:split], 10, 0.0, with_grid=False)[0]
    second = hip_ops.mesh_voxelize(t[split:], 10, 0.0, with_grid=False)[0]
    assert bool((second & ~first).any()) and bool((first & ~second).any())
    assert torch.equal(whole, first | second)
    # the last triangle, whose units the second launch finishes, marks cells that no other triangle does
    last = hip_ops.mesh_voxelize(t[32:], 10, 0.0, with_grid=False)[0]
    rest = hip_ops.mesh_voxelize(t[:32], 10, 0.0, with_grid=False)[0]
    assert bool((last & ~rest).any()) and torch.equal(whole, rest | last)
