"""The SDF datasets on the device: ``MeshSampledSDFDataset`` from an OBJ on disk and ``OctreeSampledSDFDataset`` from a voxelised
mesh -- shapes, residency, distances equal to the kernel's, reproducible resampling, the pool's narrowband -- and one end-to-end
``fit_sdf`` scored against the same fit fed by the unseeded torch sampler."""
import numpy as np
import pytest
import torch

import mesh_sample_ref as R
from mesh_sdf_ref import _bits, icosphere
from shacira_amd import harness, hip_ops
from shacira_amd.wisp.accelstructs import OctreeAS
from shacira_amd.wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset, SDFBatch, SDFDataset
from shacira_amd.wisp.ops import mesh as mesh_ops

pytestmark = pytest.mark.gpu

MODES = ["rand", "rand", "near", "near", "trace"]
# volumetric IoU (percent) of fit_sdf fed by point_sample(seed=None) + compute_sdf over torch seeds 0..4, measured on the MI355X
# (profiles/mesh_sample.md); the margin is twice their spread
PARENT_IOUS = (70.685, 70.321, 70.453, 69.742, 70.489)
MARGIN = 2 * (max(PARENT_IOUS) - min(PARENT_IOUS))


def dev():
    return torch.device("cuda")


def write_obj(path, V, F):
    with open(path, "w") as fh:
        for v in V:
            fh.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in v))
        for f in F:
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in f))
    return str(path)


@pytest.fixture(scope="module")
def obj_path(tmp_path_factory):
    V, F = icosphere(2)
    return write_obj(tmp_path_factory.mktemp("mesh") / "icosphere.obj", V, F)


def test_mesh_dataset(obj_path):
    ds = MeshSampledSDFDataset(obj_path, "train", num_samples=1000, seed=3)
    assert ds.sample_mode == MODES and len(ds) == 5000
    coords, sdf = ds.data["coords"], ds.data["sdf"]
    assert coords.shape == (5000, 3) and sdf.shape == (5000, 1) and coords.is_cuda and sdf.is_cuda
    assert coords.dtype == torch.float32 and sdf.dtype == torch.float32 and ds.coordinates is coords
    assert ds.verts.is_cuda and ds.faces.is_cuda
    tri = ds.verts[ds.faces]
    assert torch.equal(sdf.view(torch.int32), hip_ops.mesh_sdf(coords, tri)[:, None].view(torch.int32))
    trace = sdf[4000:].abs().max().item()
    print("largest |sdf| on the 'trace' segment", trace)
    assert trace < 1e-5
    assert (coords[:2000].abs() <= 1).all() and 0.001 < sdf[2000:4000].abs().mean().item() < 0.02
    # the set is the restated one: segment = the technique's position, key high word = the number of the resample
    cdf = ds.face_cdf.cpu().numpy().view(np.uint32)
    want = R.make_samples(R.SURFACE, 1000, seed=3, segment=4, triangles=tri.cpu().numpy(), cdf=cdf)
    assert np.array_equal(_bits(coords[4000:].cpu().numpy()), _bits(want["points"]))
    batch = ds[torch.arange(10, device=dev())]
    assert isinstance(batch, SDFBatch) and batch.rgb is None and batch.normals is None
    assert torch.equal(batch.coords, coords[:10]) and torch.equal(batch["sdf"], sdf[:10])
    first = {k: v.clone() for k, v in ds.data.items()}
    ds.resample()
    assert len(ds) == 5000 and not torch.equal(ds.data["coords"], first["coords"])
    want = R.make_samples(R.CUBE, 1000, seed=(1 << 32) | 3, segment=1)
    assert np.array_equal(_bits(ds.data["coords"][1000:2000].cpu().numpy()), _bits(want["points"]))
    again = MeshSampledSDFDataset(obj_path, "train", num_samples=1000, seed=3)
    for k in first:
        assert torch.equal(again.data[k], first[k])
    again.resample()
    for k in first:
        assert torch.equal(again.data[k], ds.data[k])
    other = MeshSampledSDFDataset(obj_path, "train", num_samples=1000, seed=4)
    assert not torch.equal(other.data["coords"], first["coords"])


def test_mesh_dataset_normals_and_transform(obj_path):
    def double(batch):
        return SDFBatch(coords=batch.coords * 2, sdf=batch.sdf, normals=batch.normals)

    ds = MeshSampledSDFDataset(obj_path, "val", transform=double, sample_mode=["trace", "rand"], num_samples=700,
                               get_normals=True, seed=9)
    assert len(ds) == 1400 and ds.data["normals"].shape == (1400, 3) and ds.data["normals"].is_cuda
    tri = ds.verts[ds.faces].cpu().numpy()
    want = R.make_samples(R.SURFACE, 1400, seed=9, triangles=tri, cdf=ds.face_cdf.cpu().numpy().view(np.uint32))
    assert np.array_equal(_bits(ds.data["normals"].cpu().numpy()), _bits(want["normals"]))
    assert np.array_equal(_bits(ds.data["normals"].cpu().numpy()), _bits(R.face_normals(tri)[want["face"]]))
    assert np.array_equal(_bits(ds.data["coords"].cpu().numpy()), _bits(want["points"]))
    assert ds.data["sdf"].abs().max().item() < 1e-5
    rows = torch.tensor([5, 0, 1399], device=dev())
    batch = ds[rows]
    assert torch.equal(batch.coords, ds.data["coords"][rows] * 2) and torch.equal(batch.normals, ds.data["normals"][rows])
    assert batch.fields == ["coords", "sdf", "rgb", "normals"] and batch.rgb is None


@pytest.fixture(scope="module")
def blas():
    V, F = icosphere(2, 0.6)
    return OctreeAS.from_triangles(torch.from_numpy(V).to(dev()), torch.from_numpy(F).to(dev()), 4)


def test_octree_dataset(blas):
    ds = OctreeSampledSDFDataset(blas, "train", num_samples=2000, samples_per_voxel=4, seed=5)
    pool, sdf = ds.data_pool["coords"], ds.data_pool["sdf"]
    cells = blas.points.shape[0]
    assert pool.is_cuda and sdf.shape == (ds.pool_size, 1)
    assert (blas.query(pool).pidx > -1).all()                       # the whole pool lies in the narrowband
    assert len(ds.segment_counts) == 5 and sum(ds.segment_counts) == ds.pool_size
    # 'rand' fills every occupied cell and the surface lies in the cells it was voxelised into; 'near' loses some
    n = cells * 4
    assert ds.segment_counts[0] == n and ds.segment_counts[1] == n and ds.segment_counts[4] == n
    assert 0 < ds.segment_counts[2] <= n and 0 < ds.segment_counts[3] <= n
    print("cells", cells, "pool", ds.pool_size, "segments", ds.segment_counts)
    assert torch.equal(sdf.view(torch.int32),
                       hip_ops.mesh_sdf(pool, blas.extent["vertices"][blas.extent["faces"]])[:, None].view(torch.int32))
    # the reference's pool order: both 'rand' segments (segments 0 and 1 of the key) first
    want = R.make_samples(R.CELLS, n, seed=5, segment=1, corners=blas.points.cpu().numpy(), samples_per_cell=4, cell_level=4)
    assert np.array_equal(_bits(pool[n:2 * n].cpu().numpy()), _bits(want["points"]))
    assert len(ds) == 2000 and ds.coordinates.shape == (2000, 3) and ds.data["sdf"].shape == (2000, 1)
    rows = {r.tobytes() for r in torch.cat([pool, sdf], dim=1)[:-1].cpu().numpy()}
    assert len(rows) == ds.pool_size - 1
    for _ in range(2):
        work = torch.cat([ds.data["coords"], ds.data["sdf"]], dim=1).cpu().numpy()
        assert len({r.tobytes() for r in work}) == 2000 and all(r.tobytes() in rows for r in work)
        before = ds.data["coords"].clone()
        ds.resample()
        assert not torch.equal(before, ds.data["coords"])
    again = OctreeSampledSDFDataset(blas, "train", num_samples=2000, samples_per_voxel=4, seed=5)
    assert torch.equal(again.data_pool["coords"], pool)
    again.resample()
    again.resample()
    assert torch.equal(again.data["coords"], ds.data["coords"]) and torch.equal(again.data["sdf"], ds.data["sdf"])
    batch = ds[torch.arange(7, device=dev())]
    assert isinstance(batch, SDFBatch) and batch.rgb is None and batch.normals is None and batch.coords.shape == (7, 3)


def test_octree_dataset_edges(blas):
    # more samples asked than the pool holds: the whole permutation (the reference's: of pool_size - 1 rows)
    ds = OctreeSampledSDFDataset(blas, "train", num_samples=10 ** 7, samples_per_voxel=4, sample_mode=["rand"], seed=1)
    assert ds.pool_size == blas.points.shape[0] * 4 and len(ds) == ds.pool_size - 1
    # no 'rand' entry: the reference indexes the first 'rand' segment and fails; here the segment size is known
    ds = OctreeSampledSDFDataset(blas, "train", num_samples=500, samples_per_voxel=4, sample_mode=["near", "trace"], seed=1)
    assert ds.pool_size > blas.points.shape[0] * 4 and len(ds) == 500 and (blas.query(ds.coordinates).pidx > -1).all()
    # packed words made from the bool grid when the structure does not hold them
    bare = OctreeAS(4, blas.occupancy_grid.clone())
    bare.extent.update(blas.extent)
    assert bare.packed_occupancy(4) is None
    other = OctreeSampledSDFDataset(bare, "train", num_samples=500, samples_per_voxel=4, sample_mode=["near", "trace"], seed=1)
    assert torch.equal(other.data_pool["coords"], ds.data_pool["coords"]) and torch.equal(other.data["sdf"], ds.data["sdf"])
    with pytest.raises(RuntimeError, match="was not initialized from a mesh"):
        OctreeSampledSDFDataset(OctreeAS.make_dense(3), "train")
    with pytest.raises(RuntimeError, match="texv"):
        OctreeSampledSDFDataset(blas, "train", sample_tex=True, samples_per_voxel=1)
    with pytest.raises(Exception, match="not implemented"):
        OctreeSampledSDFDataset(blas, "train", sample_mode=["spray"], samples_per_voxel=1)
    assert OctreeSampledSDFDataset.supports_blas(blas) and not OctreeSampledSDFDataset.supports_blas(OctreeAS.make_dense(2))


class ParentPathSDF(SDFDataset):
    """The working set as the code before the fused sampler made it: ``point_sample(seed=None)`` + ``compute_sdf``."""

    def __init__(self, V, F, num_samples, seed):
        super().__init__()
        torch.manual_seed(seed)
        pts = mesh_ops.point_sample(V, F, MODES, num_samples)
        self.data = dict(coords=pts, sdf=mesh_ops.compute_sdf(V, F, pts))


def fit_and_score(dataset):
    fit = harness.fit_sdf(dataset, dev(), steps=300, batch=4096, seed=0)
    return fit, harness.validate_sdf(fit["nef"], dataset)


def mesh_for_fit():
    V, F = icosphere(2, 0.6)
    return torch.from_numpy(V).to(dev()), torch.from_numpy(F).to(dev())


def test_fit_sdf_on_the_fused_dataset(tmp_path):
    V, F = mesh_for_fit()
    path = write_obj(tmp_path / "small.obj", V.cpu().numpy(), F.cpu().numpy())
    ds = MeshSampledSDFDataset(path, "train", num_samples=1000, mode_norm="none", seed=0)
    fit, score = fit_and_score(ds)
    assert list(score) == ["volumetric_iou"]
    _, parent = fit_and_score(ParentPathSDF(V, F, 1000, seed=0))
    assert list(parent) == ["iou"]
    first, last = float(np.mean(fit["losses"][:20])), float(np.mean(fit["losses"][-20:]))
    print("volumetric_iou", score["volumetric_iou"], "parent path", parent["iou"], "margin", MARGIN, "loss", first, "->", last)
    assert score["volumetric_iou"] >= parent["iou"] - MARGIN
    assert last < first and len(fit["losses"]) == 300


def test_validate_sdf_names_the_metric_by_dataset(blas):
    ds = OctreeSampledSDFDataset(blas, "train", num_samples=1000, samples_per_voxel=4, seed=2)
    fit = harness.fit_sdf(ds, dev(), steps=20, batch=512, seed=0, resample_every=8)
    score = harness.validate_sdf(fit["nef"], ds)
    assert list(score) == ["narrowband_iou"] and 0.0 <= score["narrowband_iou"] <= 100.0
    assert ds.resample_count == 3                                   # the load's, and steps 8 and 16
