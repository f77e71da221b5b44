"""The mesh-sampling contract on the host (no GPU): Philox's known answers, the entry points' validation codes (which precede
any HIP call), the statistics of the numpy restatement (tests/mesh_sample_ref.py; the GPU test ties the kernel to it bit for
bit), the CDF rule at every boundary word, and the host-side pieces of the SDF pipeline: ``SDFBatch``, ``compute_sdf_iou``, the
dataset's path validation and the seeded samplers' refusal of host tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_sample_ref as R
from conftest import ROOT
from mesh_sdf_ref import soup
from shacira_amd import _lib, hip_ops

# the 1 - 1e-6 quantiles of chi-square: 36 degrees of freedom (37 faces), and 34 (soup(37) has two zero-area faces, which
# are dropped: 35 faces). The test asserts the smaller, which implies the other.
CHI2_36, CHI2_34 = 91.50239105659848, 88.38328239675273


def test_philox_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(*counter, *key)
        assert tuple(int(x) for x in got) == want
    # vectorised over counters, and the index's high word is the second counter word
    w = R.sample_words(3, seed=(0x299F31D0 << 32) | 0xA4093822, segment=0x03707344, index_base=(0x85A308D3 << 32) | 0x243F6A88)
    assert w.shape == (3, 8) and w.dtype == np.uint32
    assert tuple(int(x) for x in R.philox4x32_10(0x243F6A88, 0x85A308D3, 0, 0x03707344, 0xA4093822, 0x299F31D0)) == tuple(w[0, :4])
    assert tuple(int(x) for x in R.philox4x32_10(0x243F6A89, 0x85A308D3, 1, 0x03707344, 0xA4093822, 0x299F31D0)) == tuple(w[1, 4:])
    # the counter's high word turns over
    w = R.sample_words(2, seed=5, index_base=(1 << 32) - 1)
    assert tuple(w[1, :4]) == tuple(int(x) for x in R.philox4x32_10(0, 1, 0, 0, 5, 0))


def test_symbols_are_declared_bound_and_exported():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "shacira_hip.h")).read()
    for name in ("shacira_mesh_sample", "shacira_mesh_sample_count"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert name in header
    assert L.shacira_abi_version() == 11                     # additive entry points do not move the ABI
    assert (_lib.MESH_SAMPLE_SURFACE, _lib.MESH_SAMPLE_NEAR, _lib.MESH_SAMPLE_CUBE, _lib.MESH_SAMPLE_CELLS) == (0, 1, 2, 3)
    assert _lib.MESH_SAMPLE_BLOCK == R.BLOCK == 256


def test_entry_points_validate_their_arguments():
    """SHACIRA_EINVAL before anything is launched: the pointers here are never dereferenced."""
    L = _lib.lib()
    one = ctypes.c_void_p(64)
    E = _lib.EINVAL

    def sample(mode=R.CUBE, n=1, base=0, words=None, T=0, tri=None, cdf=None, C=0, corners=None, spc=0, clevel=0, occ=None,
               olevel=0, offsets=None, points=one, normals=None, face=None, source=None):
        return L.shacira_mesh_sample(mode, n, base, 7, 0, words, T, tri, cdf, 0.0, C, corners, spc, clevel, occ, olevel, offsets,
                                     points, normals, face, source, None)

    def count(mode=R.CUBE, n=1, base=0, T=0, tri=None, cdf=None, C=0, corners=None, spc=0, clevel=0, occ=one, olevel=0,
              counts=one):
        return L.shacira_mesh_sample_count(mode, n, base, 7, 0, None, T, tri, cdf, 0.0, C, corners, spc, clevel, occ, olevel,
                                           counts, None)

    assert sample(mode=4) == E and sample(mode=-1) == E and count(mode=9) == E               # a bad mode
    assert sample(n=-1) == E and count(n=-1) == E and sample(n=1 << 31) == E                 # negative or too many
    assert sample(base=-1) == E and sample(base=(1 << 63) - 1, n=2) == E                     # the counter leaves int64
    assert sample(points=None) == E                                                          # a NULL output
    assert count(counts=None) == E and count(occ=None) == E
    assert sample(mode=R.SURFACE, T=1, tri=None, cdf=one) == E                               # NULL operands of the mode
    assert sample(mode=R.SURFACE, T=1, tri=one, cdf=None) == E
    assert sample(mode=R.NEAR, T=0, tri=one, cdf=one) == E                                   # no triangle to choose
    assert sample(mode=R.SURFACE, T=1 << 31, tri=one, cdf=one) == E
    assert sample(mode=R.CELLS, n=6, C=2, corners=None, spc=3) == E
    assert sample(mode=R.CELLS, n=7, C=2, corners=one, spc=3) == E                           # n != C * samples_per_cell
    assert sample(mode=R.CELLS, n=6, C=2, corners=one, spc=0) == E
    assert sample(mode=R.CELLS, n=6, C=2, corners=one, spc=3, clevel=_lib.OCTREE_MAX_LEVEL + 1) == E   # a level out of range
    assert sample(mode=R.CELLS, n=6, C=2, corners=one, spc=3, clevel=-1) == E
    assert sample(occ=one, olevel=_lib.OCTREE_MAX_LEVEL + 1, offsets=one) == E
    assert count(olevel=-1) == E and count(olevel=11) == E
    assert sample(occ=one, offsets=None) == E and sample(occ=None, offsets=one) == E         # the filter needs both
    # n == 0: nothing is launched, whatever the pointers
    assert sample(n=0, points=None) == 0 and count(n=0, counts=None, occ=None) == 0
    assert sample(mode=R.SURFACE, n=0) == 0 and sample(mode=R.CELLS, n=0, C=0, spc=4) == 0
    assert sample(mode=R.CELLS, n=0, C=1, spc=4) == E                                        # ... but the shape must still agree


def _live_soup():
    tri = soup(37)
    return tri[R.face_areas64(tri) > 0]


def test_face_counts_follow_the_area_shares():
    tri = _live_soup()
    assert tri.shape[0] == 35                                   # soup(37) has two zero-area faces: dropped
    n = 200000
    s = R.make_samples(R.SURFACE, n, seed=11, triangles=tri)
    share = R.face_areas64(tri) / R.face_areas64(tri).sum()
    counts = np.bincount(s["face"], minlength=tri.shape[0])
    chi2 = (((counts - n * share) ** 2) / (n * share)).sum()
    print("chi-square", chi2, "thresholds", CHI2_34, CHI2_36)
    assert chi2 < CHI2_34 < CHI2_36


def test_surface_samples_are_uniform_on_a_triangle():
    tri = np.asarray([[[-0.4, -0.3, 0.1], [0.5, -0.2, -0.1], [0.1, 0.6, 0.2]]], dtype=np.float32)
    n = 100000
    p = R.make_samples(R.SURFACE, n, seed=3, triangles=tri)["points"].astype(np.float64)
    centroid = tri[0].astype(np.float64).mean(axis=0)
    err = np.abs(p.mean(axis=0) - centroid)
    sem = p.std(axis=0) / np.sqrt(n)
    print("mean - centroid", err, "standard error", sem)
    assert (err < 5 * sem).all()
    # every sample lies in the triangle's plane (up to rounding) and inside it
    nrm = np.cross(tri[0, 1] - tri[0, 0], tri[0, 2] - tri[0, 0]).astype(np.float64)
    assert np.abs((p - tri[0, 0]) @ nrm).max() < 1e-6


def test_gaussian_variates_have_zero_mean_and_unit_variance():
    n = 200000
    g = R.gaussians64(R.sample_words(n, seed=5, segment=2)).reshape(-1)
    m = g.shape[0]
    print("mean", g.mean(), "variance", g.var())
    assert abs(g.mean()) < 5 / np.sqrt(m)                        # standard error of the mean: 1 / sqrt(m)
    assert abs(g.var() - 1.0) < 5 * np.sqrt(2.0 / m)             # standard error of the variance: sqrt(2 / m)
    assert np.abs(g).max() <= np.sqrt(-2 * np.log(2.0 ** -24)) + 1e-12       # the largest possible radius, 5.77


def _boundary_words(cdf):
    c = cdf.astype(np.int64)
    w = np.concatenate([[0, 0xFFFFFFFF], c - 1, c, c + 1])
    return np.unique(w[(w >= 0) & (w <= 0xFFFFFFFF)]).astype(np.uint32)


@pytest.mark.parametrize("where", ["first", "middle", "last", "first and last", "all but one"])
def test_zero_area_faces_are_never_chosen(where):
    base = _live_soup()[:9].copy()
    dead = {"first": [0], "middle": [4], "last": [8], "first and last": [0, 1, 7, 8], "all but one": [0, 1, 2, 3, 5, 6, 7, 8]}[where]
    for t in dead:
        base[t, 1] = base[t, 0]                                  # two equal vertices: no area
    cdf = R.face_cdf(base)
    assert cdf[-1] == 0xFFFFFFFF and (np.diff(cdf.astype(np.int64)) >= 0).all()
    words = _boundary_words(cdf)
    faces = R.face_of(cdf, words)
    assert ((faces >= 0) & (faces < 9)).all()                    # every word maps to a face
    assert not np.isin(faces, dead).any(), (where, faces)
    assert (np.diff(faces) >= 0).all()                           # ... monotonically
    # the wrapper's builder is the restated one
    assert np.array_equal(hip_ops.mesh_face_cdf(torch.from_numpy(base)).numpy().view(np.uint32), cdf)


def test_word_shares_equal_area_shares():
    tri = soup(37)                                               # the two zero-area faces stay in: their share is exactly 0
    cdf = R.face_cdf(tri)
    owned = R.face_word_counts(cdf)
    assert sum(owned) == 1 << 32                                 # every word has exactly one face
    area = R.face_areas64(tri)
    share = area / area.sum()
    worst = max(abs(owned[t] / 2.0 ** 32 - share[t]) for t in range(37))
    print("largest share difference", worst, "bound", 2 * 2.0 ** -32)
    assert worst <= 2 * 2.0 ** -32
    assert owned[1] == 0 and owned[2] == 0
    # face_word_counts restates face_of: at every boundary word the two agree
    words = _boundary_words(cdf)
    faces = R.face_of(cdf, words)
    starts = np.concatenate([[0], np.cumsum(owned)[:-1]])
    for w, t in zip(words.tolist(), faces.tolist()):
        assert starts[t] <= w < starts[t] + owned[t]


def test_a_mesh_without_area_is_refused():
    flat = np.zeros((3, 3, 3), dtype=np.float32)
    assert R.face_cdf(flat) is None
    with pytest.raises(RuntimeError, match="code -1"):           # SHACIRA_EINVAL
        hip_ops.mesh_face_cdf(torch.from_numpy(flat))


def test_keep_rule_restates_the_octree_query():
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.datasets.sdf_dataset import pack_occupancy
    level = 3
    grid = torch.rand(8, 8, 8, generator=torch.Generator().manual_seed(0)) < 0.4
    blas = OctreeAS(level, grid)
    pts = (torch.rand(4000, 3, generator=torch.Generator().manual_seed(1)) * 2.4 - 1.2)
    pts[:8] = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 0.0, 0.0], [0.999999, 0.0, 0.0], [float("nan"), 0.0, 0.0],
                            [0.0, float("inf"), 0.0], [-1.0000001, 0.0, 0.0], [0.75, 0.75, 0.75], [0.0, 0.0, -0.0]])
    words = pack_occupancy(grid)
    assert np.array_equal(words.numpy().view(np.uint32), R.pack_occupancy(grid.numpy()))
    assert np.array_equal(R.keep_mask(pts.numpy(), words.numpy(), level), (blas.query(pts).pidx > -1).numpy())


def test_sdf_batch_fields_and_none_entries():
    from shacira_amd.wisp.datasets import Batch, SDFBatch
    coords, sdf = torch.zeros(4, 3), torch.ones(4, 1)
    b = SDFBatch(coords=coords, sdf=sdf)
    assert isinstance(b, Batch) and isinstance(b, dict)
    assert b.fields == ["coords", "sdf", "rgb", "normals"]
    assert b["rgb"] is None and b.normals is None and b.coords is coords and b["sdf"] is sdf
    assert list(b.coord_values()) == ["sdf"]
    b = SDFBatch(coords, sdf, normals=coords)
    assert list(b.coord_values()) == ["sdf", "normals"]
    b.extra = 3
    assert b["extra"] == 3 and "extra" in b.fields
    with pytest.raises(AttributeError):
        b.missing


def test_compute_sdf_iou():
    from shacira_amd.wisp.ops.sdf import compute_sdf_iou
    gts = torch.tensor([[-1.0], [-0.5], [0.5], [1.0]])
    assert compute_sdf_iou(gts, gts) == 100.0
    assert compute_sdf_iou(torch.tensor([[-1.0], [0.5], [-0.5], [1.0]]), gts) == pytest.approx(100.0 / 3)
    assert compute_sdf_iou(-gts, gts) == 0.0
    assert compute_sdf_iou(torch.ones(4, 1), torch.ones(4, 1)) == 100.0         # the empty union
    assert compute_sdf_iou(torch.zeros(0, 1), torch.zeros(0, 1)) == 100.0


def test_mesh_dataset_validates_its_path(tmp_path):
    from shacira_amd.wisp.datasets import MeshSampledSDFDataset
    with pytest.raises(FileNotFoundError, match="does not exist"):
        MeshSampledSDFDataset(str(tmp_path / "nothing.obj"), "train")
    other = tmp_path / "mesh.ply"
    other.write_text("ply\n")
    with pytest.raises(FileNotFoundError, match="does not support the mesh format"):
        MeshSampledSDFDataset(str(other), "train")
    assert MeshSampledSDFDataset.is_root_of_dataset("a/b/bunny.obj", []) and not MeshSampledSDFDataset.is_root_of_dataset("a/b", [])


def test_seeded_samplers_refuse_host_tensors():
    from shacira_amd.wisp.ops import mesh, spc
    V, F = torch.rand(3, 3), torch.tensor([[0, 1, 2]])
    for call in (lambda: mesh.sample_surface(V, F, 4, seed=1), lambda: mesh.sample_near_surface(V, F, 4, seed=1),
                 lambda: mesh.sample_uniform(4, seed=1, device="cpu"), lambda: mesh.point_sample(V, F, ["rand", "trace"], 4, seed=1),
                 lambda: spc.sample_spc(torch.zeros(1, 3, dtype=torch.int16), 2, 3, seed=1),
                 lambda: hip_ops.mesh_sample("surface", 4, triangles=V[F])):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    # without a seed they are the torch code they were
    assert mesh.sample_surface(V, F, 4)[0].shape == (4, 3) and mesh.sample_uniform(5).shape == (5, 3)
    assert mesh.point_sample(V, F, ["rand", "near", "trace"], 4).shape == (12, 3)
    assert spc.sample_spc(torch.zeros(2, 3, dtype=torch.int16), 2, 3).shape == (6, 3)
