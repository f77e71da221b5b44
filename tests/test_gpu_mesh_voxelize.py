"""Mesh voxelisation on the MI355X: the HIP kernels of shacira_mesh_voxelize (mesh_voxelize.hip) against the numpy
restatement of the contract (tests/mesh_voxelize_ref.py). Equality is exact, on both outputs: the contract fixes the fp32
operation sequence of the overlap test, and the predicate belongs to one (cell, triangle) pair under an OR, so no split of the
work over passes, column words and lanes may change a bit. How the restatement stands against exact geometry is
test_mesh_voxelize_cpu.py's subject. Then properties that do not go through the restatement: completeness against surface
samples, a cross-check against ``closest_point``, and the structures built on the result."""
import math

import numpy as np
import pytest
import torch

import mesh_voxelize_ref as vref
from test_build_resources import _kernels

gpu = pytest.mark.gpu
MARGINS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_ONE = np.asarray([[[-0.4, -0.3, 0.1], [0.5, -0.2, -0.1], [0.1, 0.6, 0.2]]], dtype=np.float32)


def _tiny(count, seed, size=0.01):
    """``count`` triangles of extent ``size`` (a cell of level 5 is 0.0625 wide) at uniform places in the cube."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.98, 0.98, (count, 1, 3))
    return (centre + rng.uniform(-size, size, (count, 3, 3))).astype(np.float32)


def _mixed():
    """valid, degenerate, valid, NaN vertex, wholly outside, valid"""
    a, b, c = _tiny(3, 11, size=0.2)
    degenerate = np.stack([a[0], a[0], a[2]])
    nan = b.copy()
    nan[2, 0] = np.nan
    return np.stack([a, degenerate, b, nan, c + np.float32(2.5), c])


def _two_passes():
    """Five triangles more than one pass holds: 127 tiny triangles repeated to fill the first pass exactly (an OR does not
    count repeats), then 5 others, which only the second pass sees. (all triangles, the distinct ones, the repeated 127)"""
    from shacira_amd import _lib
    P = _lib.MESH_VOXELIZE_PASS_TRIANGLES
    base, extra = _tiny(127, 12), _tiny(5, 13, size=0.05)
    first = np.tile(base, (P // 127 + 1, 1, 1))[:P]
    return np.concatenate([first, extra]), np.concatenate([base, extra]), base


# name -> (triangles, level)
_CASES = {
    "ico2@0": lambda: (vref.rotated_icosphere(2), 0),
    "ico2@1": lambda: (vref.rotated_icosphere(2), 1),
    "ico2@2": lambda: (vref.rotated_icosphere(2), 2),
    "ico2@5": lambda: (vref.rotated_icosphere(2), 5),
    "ico2@6": lambda: (vref.rotated_icosphere(2), 6),
    "none@3": lambda: (np.zeros((0, 3, 3), np.float32), 3),
    "one@3": lambda: (_ONE, 3),
    "spanning@6": lambda: (np.asarray([[[-1.5, -1.4, -0.9], [1.6, -1.2, 0.1], [0.1, 1.7, 0.8]]], dtype=np.float32), 6),
    "tiny2000@5": lambda: (_tiny(2000, 10), 5),
    "outside@4": lambda: (_ONE + np.float32(3.0), 4),
    "mixed@4": lambda: (_mixed(), 4),
    "cube@3": lambda: ((lambda V, F: V[F])(*vref.cube(0.5)), 3),
    "random64@4": lambda: (vref.random_triangles(), 4),
}


def _run(tri, level, margin, dev, with_grid=True):
    from shacira_amd import hip_ops
    G = 1 << level
    words, grid = hip_ops.mesh_voxelize(torch.from_numpy(tri).to(dev), level, margin, with_grid=with_grid)
    assert words.dtype == torch.int32 and tuple(words.shape) == ((G ** 3 + 31) // 32,) and words.device == dev
    if with_grid:
        assert grid.dtype == torch.bool and tuple(grid.shape) == (G, G, G) and grid.device == dev
        assert int(grid.view(torch.uint8).max()) <= 1
    return words.cpu().numpy().view(np.uint32), (grid.cpu().numpy() if with_grid else None)


@gpu
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("name", sorted(_CASES))
def test_kernel_equals_the_restatement(dev, name, margin):
    tri, level = _CASES[name]()
    want = vref.mesh_voxelize_ref(tri, level, margin)
    words, grid = _run(tri, level, margin, dev)
    assert np.array_equal(grid, want)
    assert np.array_equal(words, vref.pack_words(want))
    if name in ("none@3", "outside@4"):
        assert not want.any()
    else:
        assert want.any()
    again, _ = _run(tri, level, margin, dev, with_grid=False)        # the same bits twice, and without the byte grid
    assert np.array_equal(again, words)


@gpu
def test_more_triangles_than_one_pass_holds(dev):
    from shacira_amd import _lib
    tri, distinct, base = _two_passes()
    assert tri.shape[0] == _lib.MESH_VOXELIZE_PASS_TRIANGLES + 5
    want = vref.mesh_voxelize_ref(distinct, 5, 0.5)
    assert (want & ~vref.mesh_voxelize_ref(base, 5, 0.5)).any()      # cells that only the second pass marks
    words, grid = _run(tri, 5, 0.5, dev)
    assert np.array_equal(grid, want) and np.array_equal(words, vref.pack_words(want))


# ---- completeness, cross-check, integration: one sphere shared by the tests below ---------------------------------------------
_SPHERE = {}


def _sphere(dev):
    """(V, F) of the turned icosphere of level 3, radius 0.7, on the device."""
    if "mesh" not in _SPHERE:
        V, F = vref.icosphere(3, 0.7)
        V = (V.astype(np.float64) @ vref.generic_rotation().T).astype(np.float32)
        _SPHERE["mesh"] = (torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev))
    return _SPHERE["mesh"]


@gpu
def test_every_surface_sample_falls_in_an_occupied_cell(dev):
    """A point within 0.45 cell (per axis) of a surface point lies in a cell whose centre is within 0.95 cell of that surface
    point, inside the closed cube of half-extent 1: the margins leave a band of 0.05 cell, far wider than fp32 rounding."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.ops.mesh import sample_surface
    V, F = _sphere(dev)
    level, cell = 5, 2.0 / 32
    torch.manual_seed(3)
    pts = sample_surface(V, F, 200_000)[0]
    blas = OctreeAS.from_triangles(V, F, level, margin=0.5)
    assert blas.extent["vertices"] is V and blas.extent["faces"] is F
    jitter = (torch.rand_like(pts) * 2.0 - 1.0) * (0.45 * cell)
    assert (blas.query(pts + jitter).pidx >= 0).all()
    tight = OctreeAS.from_triangles(V, F, level, margin=0.05)
    assert (tight.query(pts).pidx >= 0).all()
    assert 0 < tight.points.shape[0] < blas.points.shape[0] < 32 ** 3 // 4


@gpu
def test_cells_against_the_distance_to_the_mesh(dev):
    """At margin 0 an occupied cell touches the mesh, so its centre is within half a cell diagonal of it; and a centre closer
    than half a cell has the mesh inside its cell."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.ops.mesh import closest_point
    V, F = _sphere(dev)
    level, G = 5, 32
    cell = 2.0 / G
    occ = OctreeAS.from_triangles(V, F, level, margin=0.0).occupancy_grid.reshape(-1)
    idx = torch.stack(torch.meshgrid(*[torch.arange(G, device=dev)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = (idx.float() + 0.5) * cell - 1.0
    dist = closest_point(V, F, centres, signed=False)[0][:, 0]
    assert occ.any() and (dist[occ] <= math.sqrt(3.0) / 2.0 * cell * (1.0 + 1e-3)).all()
    assert occ[dist < 0.5 * cell * (1.0 - 1e-3)].all()


@gpu
def test_octree_index_raytrace_and_grid_on_the_result(dev):
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from shacira_amd.wisp.ops.octree import build_octree_index
    from shacira_amd.wisp.ops.spc import mesh_to_octree
    V, F = _sphere(dev)
    level = 5
    blas = mesh_to_octree(V, F, level, num_samples=123)
    assert isinstance(blas, OctreeAS) and blas.packed_occupancy(level) is not None and blas.packed_occupancy(4) is None
    other = OctreeAS.from_quantized_points(blas.points.long(), level)
    assert other.packed_occupancy(level) is None and torch.equal(other.points, blas.points)
    mine, theirs = build_octree_index(blas, [3, level]), build_octree_index(other, [3, level])
    for l in (3, level):
        for field in ("level_points", "points_dual", "occupancy", "corner_index"):
            assert torch.equal(getattr(mine[l], field), getattr(theirs[l], field)), (l, field)
    # 256 rays from a sphere of radius 3 towards the centre hit the surface at depth 3 - 0.7 (the faces sag 0.002 below the
    # sphere, a thirtieth of a cell): that depth lies inside an occupied cell, between the first entry and the last exit
    g = torch.Generator().manual_seed(6)
    o = torch.nn.functional.normalize(torch.randn(256, 3, generator=g), dim=-1).to(dev) * 3.0
    hits = blas.raytrace(Rays(o, -o / 3.0, 0.0, 10.0), with_exit=True)
    ridx = hits.ridx.long()
    first = torch.full((256,), float("inf"), device=dev).scatter_reduce(0, ridx, hits.depth[:, 0], "amin")
    last = torch.full((256,), -float("inf"), device=dev).scatter_reduce(0, ridx, hits.depth[:, 1], "amax")
    assert (first <= 2.3).all() and (last >= 2.3).all() and (first > 2.0).all() and (last < 4.0).all()
    pts = V[F].mean(1)
    for cls, kw in ((OctreeGrid, {}), (CodebookOctreeGrid, {})):
        grid = cls.from_triangles(V, F, feature_dim=4, base_lod=3, num_lods=3, feature_std=0.1, **kw).to(dev)
        assert grid.blas.max_level == level and torch.equal(grid.blas.points, blas.points)
        feats = grid.interpolate(pts, 2)
        assert feats.shape[0] == pts.shape[0] and torch.isfinite(feats).all() and (feats != 0).any()


def test_voxelize_kernels_have_no_private_segment():
    ks = {k: v for k, v in _kernels().items() if "vox_" in k}
    for must in ("vox_prologue_kernel", "vox_scan_kernel", "vox_pair_kernel", "vox_finish_kernel"):
        assert any(must in k for k in ks), f"{must} not found in the code objects"
    bad = {k: v for k, v in ks.items() if v[0] > 0}
    assert not bad, f"kernels with a private segment (bytes, vgprs): {bad}"
