"""The RGB-D path without a GPU: the restatement tests/spc_ref.py against hand-computed cases, the torch restatements of
wisp.ops.pointcloud, the camera moves, ``RTMVDataset(device='cpu')`` on the analytic scene of ``harness.write_analytic_rtmv``,
the host path of ``StructuredPointCloud``, ``SPCField`` and the tracer's ``lod_idx`` rule."""
import math

import numpy as np
import pytest
import torch

import spc_ref as S
from shacira_amd import harness
from shacira_amd.wisp.core import Camera, Rays
from shacira_amd.wisp.ops.pointcloud import create_pointcloud_from_images, normalize_pointcloud
from shacira_amd.wisp.ops.spc import StructuredPointCloud, pointcloud_to_octree

U = 2.0 ** -24
VIEWS, H, W = 30, 16, 24


# ---- the restatement against hand-computed cases -----------------------------------------------------------------------------
def test_cells_by_hand():
    pts = np.array([[1.0, -1.0, 0.0], [3.0, -7.0, 0.24], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [-0.5, 0.5, 0.999]], np.float32)
    keys, keep = S.cells_ref(pts, 2)                  # G = 4: cells of width 0.5
    assert keep.tolist() == [True, True, False, False, True]
    # (3, 0, 2): x = 1 falls into the last cell, x = -1 into the first; outside is clamped; (1, 3, 3)
    assert keys.tolist() == [(3 * 4 + 0) * 4 + 2, (3 * 4 + 0) * 4 + 2, (1 * 4 + 3) * 4 + 3]


def test_words_rank_slots_by_hand():
    keys = np.array([0, 31, 32, 63, 63, 0])
    words = S.words_ref(keys, 2)                      # 64 cells: two words
    assert words.tolist() == [0x80000001, 0x80000001]
    rank, cells = S.rank_ref(words)
    assert rank.tolist() == [0, 2] and cells == 4
    assert S.slots_ref(np.array([0, 31, 32, 63]), words, rank).tolist() == [0, 1, 2, 3]
    assert S.num_words(1) == 1 and S.num_words(2) == 2 and S.num_words(5) == 1024
    assert S.words_ref(np.array([7]), 1).tolist() == [0x80]          # level 1: 8 cells in one word


def test_colour_means_by_hand():
    keys = np.array([5, 5, 9, 9, 9])
    cols = np.array([[0, 1, 255], [1, 2, 255], [10, 0, 1], [10, 0, 1], [11, 1, 1]], np.uint8)
    words = S.words_ref(keys, 2)
    rank, cells = S.rank_ref(words)
    sums, colors = S.colors_ref(keys, cols, words, rank, cells)
    assert sums.tolist() == [[1, 3, 510, 2], [31, 1, 3, 3]]
    # 0.5 is a tie and rounds up: (2 * 1 + 2) // 4 = 1; 1.5 -> 2; 31 / 3 = 10.33 -> 10; 1 / 3 -> 0
    assert colors.tolist() == [[1, 2, 255, 255], [10, 0, 1, 255]]


def test_colour_bytes_by_hand():
    px = np.array([[255, 0, 128, 255], [255, 0, 128, 0], [10, 20, 30, 128]], np.uint8)
    white = S.colour_bytes_ref(px, False)
    assert white[0].tolist() == [255, 0, 128] and white[1].tolist() == [255, 255, 255]
    assert S.colour_bytes_ref(px, True)[1].tolist() == [0, 0, 0]
    a = 128 / 255
    assert white[2].tolist() == [round(255 * (c / 255 * a + 1 - a)) for c in (10, 20, 30)]
    assert S.colour_bytes_ref(px[:, :3], False).tolist() == px[:, :3].tolist()
    assert S.colour_bytes_ref(np.array([[4 * 255, 0, 2 * 255, 4 * 255]]), False, mip=1).tolist() == [[255, 0, 128]]


def test_first_hit_by_hand():
    occ = np.zeros((2, 2, 2), bool)
    occ[0, 0, 0] = True
    o = np.array([[-2, -0.5, -0.5], [2, -0.5, -0.5], [-0.5, -0.5, -0.5], [-2, 0.5, 0.5], [-2, -0.5, -0.5], [np.nan, 0, 0],
                  [0.5, 0.5, 0.5]], np.float32)
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    depth, hit, pidx = S.first_hit_ref(o, d, occ, 1)
    # from outside: enters the cube at 1; through the empty cell (1, 0, 0) first, from 1 to 2; from inside the cell: 0; a row of
    # empty cells; pointing away; not finite; a zero direction inside an empty cell
    assert hit.tolist() == [True, True, True, False, False, False, False]
    assert depth.tolist() == [1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert pidx.tolist() == [0, 0, 0, -1, -1, -1, -1]
    occ[:] = False
    occ[1, 1, 1] = True
    depth, hit, pidx = S.first_hit_ref(np.array([[2, 0.5, 0.5]], np.float32), np.array([[-1, 0, 0]], np.float32), occ, 1)
    assert (depth[0], hit[0], pidx[0]) == (1.0, True, 7)


def test_walk_restatement_equals_the_recorded_kernels():
    """tests/golden/grid_walk.npz holds what the dense-grid walk computed on an MI355X (tests/golden/make_grid_walk.py):
    ``walk_ref`` and ``first_hit_ref`` reproduce it on the recorded inputs -- counts, ray ids and Morton indices exactly, every
    depth bit for bit. The recording is the authority; tests/test_gpu_grid_walk.py holds the kernels to the same file."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_walk.npz"))
    dense = sorted({tuple(k.split(".")[1:3]) for k in gold.files if k.startswith("dense.")})
    assert len(dense) == 6
    for N, level in dense:
        g = lambda name: gold[f"dense.{N}.{level}.{name}"]
        level = int(level)
        occ = S.occupancy_from_bits(g("bits"), level)
        ridx, cells, depth = S.walk_ref(g("origins"), g("dirs"), occ, level, finite_gate=False)
        assert np.array_equal(np.bincount(ridx, minlength=int(N)), g("counts")) and np.array_equal(ridx, g("ridx"))
        assert np.array_equal([S.morton(int(x), int(y), int(z), level) for x, y, z in cells], g("pidx"))
        assert np.array_equal(depth.view(np.int32), g("depth").view(np.int32))
    hits = sorted({tuple(k.split(".")[1:4]) for k in gold.files if k.startswith("hit.") and k.endswith(".origins")})
    assert len(hits) == 3 * 5 * 5
    for level, kind, N in hits:
        g = lambda name: gold[f"hit.{level}.{kind}.{N}.{name}"]
        occ = S.occupancy_from_bits(gold[f"hit.{level}.{kind}.bits"], int(level))
        depth, hit, pidx = S.first_hit_ref(g("origins"), g("dirs"), occ, int(level))
        assert np.array_equal(hit, g("hit")) and np.array_equal(pidx, g("pidx")), (level, kind, N)
        assert np.array_equal(depth.view(np.int32), g("depth").view(np.int32)), (level, kind, N)


# ---- wisp.ops.pointcloud and the camera moves --------------------------------------------------------------------------------
def test_create_pointcloud_from_images_literal():
    rgb = torch.arange(2 * 2 * 4, dtype=torch.float32).reshape(2, 2, 4)
    mask = torch.tensor([[1.0, 0.0], [0.0, 1.0]]).reshape(2, 2, 1)
    rays = Rays(torch.ones(2, 2, 3), torch.tensor([0.0, 0.0, 2.0]).expand(2, 2, 3))
    depth = torch.tensor([[1.0, 5.0], [5.0, 3.0]]).reshape(2, 2, 1)
    coords, colors = create_pointcloud_from_images([rgb, rgb], [mask, mask], [rays, rays], [depth, depth])
    assert coords.tolist() == [[1, 1, 3], [1, 1, 7]] * 2
    assert colors.tolist() == [[0, 1, 2], [12, 13, 14]] * 2


def test_normalize_pointcloud_literal():
    pts = torch.tensor([[0.0, 0.0, 0.0], [4.0, 2.0, 1.0], [2.0, 1.0, -1.0]])
    out, center, scale = normalize_pointcloud(pts.clone(), return_scale=True)
    assert center.tolist() == [2.0, 1.0, 0.0] and float(scale) == 0.5
    assert out.tolist() == [[-1.0, -0.5, 0.0], [1.0, 0.5, 0.5], [0.0, 0.0, -0.5]]
    assert torch.equal(normalize_pointcloud(pts.clone()), out)


def test_camera_translate_and_t_setter():
    eye = torch.tensor([[3.0, 1.0, 2.0], [-1.0, 2.0, 0.5]], dtype=torch.float64)
    cam = Camera.from_args(eye=eye, at=torch.zeros(3, dtype=torch.float64), up=torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64),
                           focal_x=20.0, width=8, height=8)
    rot = cam.view_matrix()[:, :3, :3].clone()
    center, scale = torch.tensor([0.5, -0.25, 1.0], dtype=torch.float64), 1.75
    cam.translate(-center)
    assert torch.allclose(cam.cam_pos(), eye - center, atol=1e-14, rtol=0)
    cam.t = cam.t * scale
    assert torch.allclose(cam.cam_pos(), (eye - center) * scale, atol=1e-14, rtol=0)
    assert torch.equal(cam.view_matrix()[:, :3, :3], rot)
    cam2 = Camera.from_args(eye=eye, at=torch.zeros(3, dtype=torch.float64), up=torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64),
                            focal_x=20.0, width=8, height=8).normalize(center, scale)
    assert torch.equal(cam2.view_matrix(), cam.view_matrix())


# ---- RTMVDataset on the host -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from shacira_amd.wisp.datasets import RTMVDataset
    path = str(tmp_path_factory.mktemp("rtmv"))
    harness.write_analytic_rtmv(path, VIEWS, H, W, seed=3)
    train = RTMVDataset(path, "white", device="cpu")
    ref = S.points_ref(train.records.numpy(), W, H, train.depth.numpy())
    return path, train, ref


def test_rtmv_splits(scene):
    from shacira_amd.wisp.datasets import RTMVDataset
    path, train, _ = scene
    assert len(train) == 20 and train.basenames[0] == "00000" and train.basenames[-1] == "00019"
    val, test = train.create_split("val"), train.create_split("test")
    assert val.basenames == ["00020"] and test.basenames == [f"{i:05d}" for i in range(21, 30)]
    for other in (val, test):       # the train split's normalisation is passed on, not recomputed
        assert other.coords_scale == train.coords_scale and torch.equal(other.coords_center, train.coords_center)
    with pytest.raises(RuntimeError):
        RTMVDataset(path, "white", split="all")
    with pytest.raises(ValueError):
        RTMVDataset(path, "white", train_ratio=0.0)
    with pytest.raises(NotImplementedError):
        RTMVDataset(path, "white", mip=1, device="cpu")
    assert train.supports_depth() and tuple(train.img_shape) == (H, W, 3)
    assert train.reference_resident_bytes() == 20 * H * W * 41
    assert train.resident_bytes() == 20 * H * W * 8 + 20 * 80
    assert RTMVDataset.is_root_of_dataset(path, ["00000.json", "00000.exr"])
    assert not RTMVDataset.is_root_of_dataset(path, ["00000.json", "00000.png"])


def test_rtmv_cloud_is_normalised_and_on_the_sphere(scene):
    _, train, ref = scene
    cloud = train.as_pointcloud()
    valid = ref["valid"]
    assert cloud.shape == (int(valid.sum()), 3) and cloud.dtype == torch.float32
    bound = ref["bound"][valid]
    # the host chain rounds the fp64 ray once and then follows the same two operations: inside the carried bound
    assert (np.abs(cloud.numpy().astype(np.float64) - ref["points"][valid]) <= bound).all()
    tol = 2.0 * bound.max() + 16 * U
    assert float(cloud.abs().max()) <= 1.0 + tol
    assert abs(float(cloud.max()) - 1.0) <= tol
    # every point lies on the scaled sphere. Besides the carried bound: the depth was rounded to fp32 when stored and when
    # scaled (2 U t s), the original and the moved camera positions were rounded to fp32 records (U |pos| s each)
    s, c = train.coords_scale, train.coords_center.double().numpy()
    dist = np.linalg.norm(cloud.numpy().astype(np.float64) / s + c, axis=1)
    t_max = harness.ANALYTIC_RTMV_DISTANCE + harness.ANALYTIC_RTMV_RADIUS
    slack = (np.linalg.norm(bound, axis=1) + U * s * (2 * math.sqrt(3) * harness.ANALYTIC_RTMV_DISTANCE + 2 * t_max)) / s
    assert (np.abs(dist - harness.ANALYTIC_RTMV_RADIUS) <= slack).all(), np.abs(dist - harness.ANALYTIC_RTMV_RADIUS).max()


def test_rtmv_invalid_pixels(scene):
    _, train, ref = scene
    valid = torch.from_numpy(ref["valid"]).reshape(20, H * W)
    assert 0 < int(valid.sum()) < valid.numel()
    assert torch.equal(torch.isfinite(train.depth).reshape(20, -1), valid) and torch.isnan(train.depth[~valid.reshape(20, H, W)]).all()
    view = train[3]
    assert set(view) == {"rays", "rgb", "masks", "depth", "alpha"}
    assert view["depth"].shape == (H * W, 1) and view["alpha"].dtype == torch.bool
    assert torch.equal(view["alpha"][:, 0], valid[3])
    assert (view["depth"][~valid[3]] == -train.coords_scale).all()
    assert torch.equal(view["depth"][valid[3]][:, 0], train.depth[3].reshape(-1)[valid[3]])
    # alpha 255 exactly on the object: the image mask agrees with the depth mask
    assert torch.equal(view["masks"][:, 0], valid[3])
    batch = train.sample(257, generator=torch.Generator().manual_seed(1))
    v, p = batch["view_idx"].long(), batch["pixel_idx"].long()
    assert torch.equal(batch["alpha"][:, 0], valid[v, p])
    expect = torch.where(valid[v, p], train.depth.reshape(20, -1)[v, p], torch.tensor(-train.coords_scale))
    assert torch.equal(batch["depth"][:, 0], expect)


def test_end_to_end_fixture_stays_under_the_cap():
    """The GPU end-to-end test excludes pixels whose fp64 point lies within the carried bound of a cell face: at most 2 %."""
    import tempfile
    from shacira_amd.wisp.datasets import RTMVDataset
    with tempfile.TemporaryDirectory() as path:
        harness.write_analytic_rtmv(path, 6, 16, 24, seed=0)
        ds = RTMVDataset(path, "white", train_ratio=1.0, val_ratio=0.0, device="cpu")
        ref = S.points_ref(ds.records.numpy(), 24, 16, ds.depth.numpy())
    valid = ref["valid"]
    cell = ref["points"][valid] * 16 + 16                      # in cells of level 5
    near = (np.abs(cell - np.round(cell)) <= ref["bound"][valid] * 16).any(axis=1)
    assert near.mean() <= 0.02, near.mean()


# ---- StructuredPointCloud, SPCField, the tracer's level rule -----------------------------------------------------------------
def _cloud(n=3000, seed=0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    pts[0] = torch.tensor([1.0, -1.0, 0.3])
    pts[1] = torch.tensor([float("nan"), 0.0, 0.0])
    pts[2] = torch.tensor([2.0, -3.0, 0.0])
    cols = torch.randint(0, 256, (n, 3), generator=g, dtype=torch.uint8)
    return pts, cols


@pytest.mark.parametrize("level", [1, 2, 4])
def test_structured_point_cloud_host_path(level):
    pts, cols = _cloud()
    spc = StructuredPointCloud.from_pointcloud(pts, cols, level)
    blas, means = pointcloud_to_octree(pts, level, attributes=cols.float())
    mine = spc.to_octree_as()
    assert torch.equal(mine.points, blas.points) and torch.equal(mine.occupancy_grid, blas.occupancy_grid)
    assert mine.packed_occupancy(level) is spc.words
    assert spc.num_cells == blas.points.shape[0] == spc.colors.shape[0]
    cm = spc.colors_morton()
    assert (cm[:, 3] == 255).all()
    assert (cm[:, :3].float() - means).abs().max() <= 0.5 + 1e-3      # the rounded mean; fp32 means carry a little rounding
    # bit for bit against the restatement
    keys, keep = S.cells_ref(pts.numpy(), level)
    words = S.words_ref(keys, level)
    rank, cells = S.rank_ref(words)
    _, colors = S.colors_ref(keys, cols.numpy()[keep], words, rank, cells)
    assert np.array_equal(spc.words.numpy().view(np.uint32), words) and np.array_equal(spc.rank.numpy(), rank)
    assert np.array_equal(spc.colors.numpy(), colors)
    from shacira_amd.wisp.accelstructs import _morton_index
    pidx = _morton_index(mine.points, level)
    assert torch.equal(spc.colors[spc.slots_of(pidx)], cm)


def test_spc_field_colour_modes():
    from shacira_amd.wisp.accelstructs import _morton_index
    from shacira_amd.wisp.models.nefs import SPCField
    pts, cols = _cloud(500, seed=1)
    spc = StructuredPointCloud.from_pointcloud(pts, cols, 3)
    blas = spc.to_octree_as()
    pidx = _morton_index(blas.points, 3)
    pick = torch.tensor([0, 5, blas.points.shape[0] - 1])
    field = SPCField(spc)
    out = field(channels="rgb", ridx_hit=pidx[pick])
    assert out.shape == (3, 1, 3) and field.grid.blas.max_level == 3
    assert torch.equal(out[:, 0], spc.colors_morton()[pick, :3].float() / 255.0)
    assert torch.equal(field.rgba(pidx[pick])["rgb"], out)
    by_dict = SPCField(blas, dict(colors=spc.colors_morton()))
    assert torch.equal(by_dict(channels="rgb", ridx_hit=pidx[pick]), out)
    normals = torch.nn.functional.normalize(torch.randn(blas.points.shape[0], 3, generator=torch.Generator().manual_seed(2)), dim=1)
    by_normal = SPCField(blas, dict(normals=normals))
    assert torch.equal(by_normal(channels="rgb", ridx_hit=pidx[pick])[:, 0], 0.5 * (normals[pick] + 1.0))
    bare = SPCField(blas)
    assert torch.equal(bare(channels="rgb", ridx_hit=pidx[pick])[:, 0], blas.points[pick].float() / 8.0)
    with pytest.raises(Exception):
        field(channels="sdf", ridx_hit=pidx[pick])


def test_tracer_rejects_coarser_levels():
    from shacira_amd.wisp.models.nefs import SPCField
    from shacira_amd.wisp.tracers import PackedSPCTracer
    pts, cols = _cloud(200, seed=4)
    field = SPCField(StructuredPointCloud.from_pointcloud(pts, cols, 3))
    rays = Rays(torch.zeros(4, 3), torch.ones(4, 3))
    tracer = PackedSPCTracer()
    assert tracer.get_supported_channels() == {"depth", "hit", "rgb", "alpha"}
    for fn in (tracer.trace, tracer.trace_composed):
        with pytest.raises(ValueError):
            fn(field, rays, {"rgb"}, set(), lod_idx=2)
