"""Mesh voxelisation without a GPU: the numpy restatement of the shacira_mesh_voxelize contract (tests/mesh_voxelize_ref.py)
against an fp64 separating-axis test in its textbook form, the pure-torch helpers of ``wisp.ops.spc`` against their
definitions, and the guards of the Python surface.

Restatement against fp64, with a tolerance EPS in cells: A = the cells overlapped at half-extent h - EPS, B = those at
h + EPS, and A <= restatement <= B is required. Measured: on every input below the restatement EQUALS the fp64 set, so the
inclusion holds at every power of ten tried, down to 1e-12 -- the search for the smallest one finds no floor. The floor is then
the number format's: a grid coordinate at level 5 is rounded by up to ulp(32) / 2 = 1.9e-6 cells and the edge functions multiply
two of them, so 1e-5 is the smallest power of ten the fp32 formulas can be held to; EPS is ten times that. At EPS, B \\ A is
at most 2 cells of 4 670 (0.04 %), far inside the 2 % condition, which is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_voxelize_ref as vref

EPS = 1e-4
MARGINS = (0.0, 0.5, 1.0)
_INPUTS = {
    "ico2@3": lambda: (vref.rotated_icosphere(2), 3),
    "ico2@5": lambda: (vref.rotated_icosphere(2), 5),
    "random64@4": lambda: (vref.random_triangles(), 4),
}


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("name", sorted(_INPUTS))
def test_restatement_lies_between_the_fp64_sets(name, margin):
    tri, level = _INPUTS[name]()
    h = 0.5 + margin
    A, B = vref.sat_f64(tri, level, h - EPS), vref.sat_f64(tri, level, h + EPS)
    band, outer = int((B & ~A).sum()), int(B.sum())
    print(f"{name} margin {margin}: |A| {int(A.sum())} |B| {outer} |B - A| {band}")
    assert outer > 0 and band <= 0.02 * outer          # the condition on the inputs, on the fp64 test alone
    got = vref.mesh_voxelize_ref(tri, level, margin)
    assert not (A & ~got).any() and not (got & ~B).any()
    if name == "random64@4":                           # some triangles reach outside: the border cells are not a dumping ground
        assert (np.abs(tri) > 1.0).any()


def test_axis_aligned_cube_marks_both_sides_of_its_faces():
    """The cube [-0.5, 0.5]^3 at level 3 has its faces on the cell boundaries x, y, z = 2 and 6 (grid units). At margin 0 a
    closed cell touches the surface iff all its indices are in 1..6 and one of them is 1, 2, 5 or 6: 6^3 - 2^3 cells."""
    V, F = vref.cube(0.5)
    got = vref.mesh_voxelize_ref(V[F], 3, 0.0)
    idx = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1)
    want = ((idx >= 1) & (idx <= 6)).all(-1) & ~((idx >= 3) & (idx <= 4)).all(-1)
    assert want.sum() == 6 ** 3 - 2 ** 3
    assert np.array_equal(got, want)
    assert got[1, 3, 3] and got[2, 3, 3] and got[5, 3, 3] and got[6, 3, 3] and not got[0, 3, 3] and not got[3, 3, 3]
    # margin 1: the cube of half-extent 1.5 around every centre of the 8^3 grid touches the surface, the corner cells
    # (centre 0.5, reaching to 2) and the innermost ones (centre 3.5, reaching down to 2) only in a point or a face: closed
    assert vref.mesh_voxelize_ref(V[F], 3, 1.0).all()


def test_invalid_triangles_and_geometry_outside_mark_nothing():
    one = np.asarray([[-0.4, -0.3, 0.1], [0.5, -0.2, -0.1], [0.1, 0.6, 0.2]], dtype=np.float32)
    degenerate = np.stack([one[0], one[0], one[2]])
    nan = one.copy()
    nan[1, 1] = np.nan
    outside = one + np.float32(3.0)
    base = vref.mesh_voxelize_ref(one[None], 4, 0.5)
    assert base.any()
    for bad in (degenerate, nan, outside):
        assert not vref.mesh_voxelize_ref(bad[None], 4, 0.5).any()
        assert np.array_equal(vref.mesh_voxelize_ref(np.stack([bad, one, bad]), 4, 0.5), base)
    assert not vref.mesh_voxelize_ref(np.zeros((0, 3, 3), np.float32), 4, 0.5).any()
    words = vref.pack_words(base)
    assert words.shape == (128,) and sum(bin(int(w)).count("1") for w in words) == int(base.sum())


# ---- wisp.ops.spc ------------------------------------------------------------------------------------------------------------
def _morton(cells, level):
    code = np.zeros(cells.shape[0], dtype=np.int64)
    for b in range(level):
        code |= (((cells[:, 0] >> b) & 1) << (3 * b + 2)) | (((cells[:, 1] >> b) & 1) << (3 * b + 1)) | (
            ((cells[:, 2] >> b) & 1) << (3 * b))
    return code


def test_dilate_points_is_the_clipped_26_neighbourhood():
    from shacira_amd.wisp.ops.spc import dilate_points
    level, G = 3, 8
    cells = np.asarray([[0, 0, 0], [7, 3, 7], [4, 4, 4], [4, 5, 4], [4, 4, 4]], dtype=np.int64)
    want = set()
    for c in cells:
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    want.add(tuple(np.clip(c + (dx, dy, dz), 0, G - 1)))
    got = dilate_points(torch.from_numpy(cells).short(), level)
    assert got.dtype == torch.int16
    got = got.long().numpy()
    assert len(got) == len(want) and set(map(tuple, got)) == want
    assert (np.diff(_morton(got, level)) > 0).all()


def test_sample_spc_samples_fall_in_their_cells():
    from shacira_amd.wisp.ops.spc import sample_spc
    torch.manual_seed(0)
    level, k = 4, 9
    cells = torch.tensor([[0, 0, 0], [15, 15, 15], [3, 9, 12]])
    s = sample_spc(cells, level, k)
    assert tuple(s.shape) == (3 * k, 3) and s.dtype == torch.float32
    cell = torch.floor((s.double() + 1.0) * 8.0).long().reshape(3, k, 3)
    assert (cell == cells[:, None, :]).all()


def test_pointcloud_to_octree_averages_attributes_per_cell():
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.ops.spc import pointcloud_to_octree
    rng = np.random.default_rng(2)
    level, G = 3, 8
    pts = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    pts[5] = np.nan
    att = rng.normal(size=(400, 2)).astype(np.float32)
    blas, mean = pointcloud_to_octree(torch.from_numpy(pts), level, torch.from_numpy(att))
    assert isinstance(blas, OctreeAS) and blas.max_level == level
    keep = np.isfinite(pts).all(-1)
    cell = np.clip(np.floor(G * (pts[keep] + 1.0) / 2.0), 0, G - 1).astype(np.int64)
    uniq = np.unique(cell, axis=0)
    uniq = uniq[np.argsort(_morton(uniq, level))]
    assert np.array_equal(blas.points.long().numpy(), uniq)
    want = np.stack([att[keep][(cell == u).all(-1)].astype(np.float64).mean(0) for u in uniq])
    assert np.allclose(mean.numpy(), want, atol=1e-5)
    grown = pointcloud_to_octree(torch.from_numpy(pts), level, dilate=1)
    assert grown.points.shape[0] > blas.points.shape[0]
    assert (grown.occupancy_grid | ~blas.occupancy_grid).all()


def test_depth_interval_samples_and_expanded_boundaries():
    from shacira_amd.wisp.ops.spc import expand_pack_boundary, sample_from_depth_intervals
    torch.manual_seed(1)
    iv = torch.tensor([[1.0, 2.0], [0.5, 0.75]])
    s = sample_from_depth_intervals(iv, 8)
    assert tuple(s.shape) == (2, 8)
    lo = iv[:, 0:1] + (iv[:, 1:2] - iv[:, 0:1]) * torch.arange(8)[None] / 8
    assert (s >= lo).all() and (s <= lo + (iv[:, 1:2] - iv[:, 0:1]) / 8 + 1e-6).all()
    big = expand_pack_boundary(torch.tensor([True, False, False, True]), 3)
    assert big.dtype == torch.int32 and big.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]


# ---- the surface's guards -----------------------------------------------------------------------------------------------------
def test_host_tensors_raise_and_from_mesh_still_raises():
    from shacira_amd import hip_ops
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from shacira_amd.wisp.ops.spc import mesh_to_octree
    V, F = vref.cube(0.5)
    V, F = torch.from_numpy(V), torch.from_numpy(F)
    for call in (lambda: OctreeAS.from_triangles(V, F, 3), lambda: mesh_to_octree(V, F, 3, num_samples=10),
                 lambda: OctreeGrid.from_triangles(V, F, 2, 2, 2), lambda: hip_ops.mesh_voxelize(V[F], 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for fn in (OctreeAS.from_mesh, OctreeGrid.from_mesh, CodebookOctreeGrid.from_mesh):
        with pytest.raises(NotImplementedError, match="from_triangles"):
            fn("mesh.obj", 4)


def test_spc_is_installed_with_the_other_mirrored_packages():
    import shacira_amd.wisp as mirror
    assert "ops.spc" in mirror._ALIASES


def test_entry_point_validates_before_any_launch():
    from shacira_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: validation fails first
    vox = L.shacira_mesh_voxelize
    assert vox(-1, one, 3, 0.5, one, None, one, 1 << 30, None) == _lib.EINVAL             # count
    assert vox(1 << 31, one, 3, 0.5, one, None, one, 1 << 30, None) == _lib.EINVAL
    assert vox(4, one, -1, 0.5, one, None, one, 1 << 30, None) == _lib.EINVAL             # level
    assert vox(4, one, _lib.OCTREE_MAX_LEVEL + 1, 0.5, one, None, one, 1 << 30, None) == _lib.EINVAL
    for margin in (-0.5, float("nan"), float("inf")):
        assert vox(4, one, 3, margin, one, None, one, 1 << 30, None) == _lib.EINVAL
    assert vox(4, None, 3, 0.5, one, None, one, 1 << 30, None) == _lib.EINVAL             # null operands
    assert vox(4, one, 3, 0.5, None, None, one, 1 << 30, None) == _lib.EINVAL
    assert vox(4, one, 3, 0.5, one, ctypes.c_void_p(24), one, 1 << 30, None) == _lib.EINVAL   # grid not 16-byte aligned
    assert vox(4, one, 3, 0.5, one, None, None, 0, None) == _lib.EWORKSPACE
    assert vox(4, one, 3, 0.5, one, None, one, 8, None) == _lib.EWORKSPACE
    size = L.shacira_mesh_voxelize_workspace_bytes
    assert size(0, 3) == 0 and size(-1, 3) == 0 and size(4, 11) == 0
    assert size(4, 3) == 4 * 192 + 5 * 8
    P = _lib.MESH_VOXELIZE_PASS_TRIANGLES
    assert size(10 * P, 10) == size(P, 0) == P * 192 + (P + 1) * 8
