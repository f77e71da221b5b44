"""The structured-point-cloud kernels (shacira_amd/csrc/spc.hip) on the MI355X against the restatement tests/spc_ref.py, at the
smallest shapes that cross their edges: pixel counts around the 64-lane wavefront and the 256-pixel workgroup, both lenses, 3 and
4 channels, both backgrounds, a mip-1 sums source, a side stream; depth planes that are all invalid, all valid, sprinkled with
NaN / inf / 1e10, and 0; levels 1 (one word), 2 (two words) and 5.

Every call goes through the raw entry points on outputs pre-filled with a sentinel. Points: within the bound carried through the
fp32 sequence (tests/spc_ref.py). Colour bytes, cell sets, ranks, sums and colours: bit for bit, and the fused ``_depth`` results
bit for bit equal to the ``_points`` results on the emitted cloud. First hit: exactly the first nugget per ray of
``render.raytrace_dense`` (the parent's kernel) on the same set, and ``trace_composed`` for the ``RenderBuffer``."""
import ctypes
import math

import numpy as np
import pytest
import torch

import raygen_ref as R
import spc_ref as S
from shacira_amd import _lib, harness, hip_ops, render
from shacira_amd.wisp.core import Rays
from shacira_amd.wisp.ops.raygen import image_mip_torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENT = 777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def records(V, width, height, lens):
    """fp32 records [V, K] of cameras about 1.5 from the origin, looking roughly at it."""
    out = []
    for i in range(V):
        rot = rotation([0.3 + i, -1.0, 0.5], 0.2 + 0.3 * i)
        pos = rot @ np.array([0.1 * i, -0.05, 1.5])                     # the camera looks down its -z axis
        out.append(R.make_record(rot, pos, width / (2 * 1.2 * width), height / (2 * 1.2 * width), 0.0, 0.0,
                                 0.6 if lens == "ortho" else None, width / height))
    return np.stack(out) if V else np.zeros((0, R.K), np.float32)


def depth_plane(kind, V, H, W, rng):
    d = rng.uniform(0.6, 2.4, (V, H, W)).astype(np.float32)
    if kind == "invalid":
        d[:] = np.nan
    elif kind == "sprinkled":
        flat = d.reshape(-1)
        for k, bad in enumerate((np.nan, np.inf, -np.inf)):
            flat[k::7] = bad
        flat[3::11] = 1e10                                              # finite: a valid pixel, far outside the cube
    elif kind == "zero":
        d[:] = 0.0
    return d


class Case:
    """One depth data set on the device and its restatement."""

    def __init__(self, dev, V, H, W, lens="pinhole", channels=4, bg_black=False, plane="valid", mip=0, seed=0):
        rng = np.random.default_rng(seed)
        self.dev, self.V, self.H, self.W, self.channels, self.bg_black, self.mip = dev, V, H, W, channels, bg_black, mip
        self.rec = records(V, W, H, lens)
        self.depth = depth_plane(plane, V, H, W, rng)
        f = 1 << mip
        full = rng.integers(0, 256, (V, H * f, W * f, channels), dtype=np.uint8)
        if channels == 4:
            full[..., 3][full[..., 3] < 64] = 0
            full[..., 3][full[..., 3] > 192] = 255
        pixels = image_mip_torch(torch.from_numpy(full), mip).numpy() if mip else full
        self.n = V * H * W
        self.ref = S.points_ref(self.rec, W, H, self.depth) if V else dict(valid=np.zeros(0, bool), points=np.zeros((0, 3)),
                                                                            bound=np.zeros((0, 3)))
        self.valid = self.ref["valid"]
        self.bytes_ref = S.colour_bytes_ref(pixels.reshape(self.n, channels)[self.valid], bg_black, mip)
        self.rec_d = torch.from_numpy(self.rec).to(dev)
        self.depth_d = torch.from_numpy(self.depth).to(dev)
        self.img_d = torch.from_numpy(pixels.astype(np.uint16 if mip else np.uint8)).to(dev)
        self.head = (_p(self.rec_d), V, W, H, _p(self.depth_d))
        self.tail = (_p(self.img_d), channels, mip, int(bg_black))


def run_bounds(c, stream):
    bounds = torch.full((6,), SENT, device=c.dev)
    count = torch.full((1,), -5, dtype=torch.int64, device=c.dev)
    torch.cuda.synchronize()
    assert _lib.lib().shacira_depth_bounds(*c.head, _p(bounds), _p(count), ctypes.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()
    return bounds.cpu().numpy(), int(count.item())


def run_cloud(c, stream, colours=True):
    blocks = (c.n + 255) // 256
    counts = torch.full((blocks,), -7, dtype=torch.int32, device=c.dev)
    torch.cuda.synchronize()
    sp = ctypes.c_void_p(stream.cuda_stream)
    assert _lib.lib().shacira_depth_points_count(*c.head, _p(counts), sp) == 0
    stream.synchronize()
    counts_h = counts.cpu().numpy()
    if c.V:
        want = np.add.reduceat(c.valid.astype(np.int64), np.arange(0, c.n, 256))
        assert np.array_equal(counts_h, want)
    M = int(counts_h.sum())
    offsets = torch.from_numpy(np.cumsum(counts_h) - counts_h).to(torch.int64).to(c.dev)
    points = torch.full((M, 3), SENT, device=c.dev)
    rgb = torch.full((M, 3), 77, dtype=torch.uint8, device=c.dev) if colours else None
    if M:                   # nothing kept: there are no rows to pass, the writer is not launched
        torch.cuda.synchronize()
        assert _lib.lib().shacira_depth_points_emit(*c.head, *c.tail, _p(offsets), _p(points), _p(rgb), sp) == 0
        stream.synchronize()
    return points, rgb


def build_spc(c, level, cloud, cloud_rgb, stream):
    """(words, rank, cells, sums, colors) from the fused depth entries, asserted bit-equal to the entries fed the emitted cloud."""
    L, sp = _lib.lib(), ctypes.c_void_p(stream.cuda_stream)
    nw = S.num_words(level)
    assert L.shacira_spc_num_words(level) == nw
    wd = torch.zeros((nw,), dtype=torch.int32, device=c.dev)
    wp = torch.zeros((nw,), dtype=torch.int32, device=c.dev)
    pop = torch.full((nw,), -3, dtype=torch.int32, device=c.dev)
    torch.cuda.synchronize()
    assert L.shacira_spc_mark_depth(*c.head, level, _p(wd), sp) == 0
    assert L.shacira_spc_mark_points(cloud.shape[0], _p(cloud), level, _p(wp), sp) == 0
    assert L.shacira_spc_rank(level, _p(wd), _p(pop), sp) == 0
    stream.synchronize()
    assert torch.equal(wd, wp)
    words = wd.cpu().numpy().view(np.uint32)
    assert np.array_equal(pop.cpu().numpy(), S.popcount(words))
    rank, cells = S.rank_ref(words)
    rank_d = torch.from_numpy(rank).to(c.dev)
    sd = torch.zeros((cells, 4), dtype=torch.int64, device=c.dev)
    sq = torch.zeros((cells, 4), dtype=torch.int64, device=c.dev)
    colors = torch.full((cells, 4), 99, dtype=torch.uint8, device=c.dev)
    torch.cuda.synchronize()
    assert L.shacira_spc_accumulate_depth(*c.head, *c.tail, level, _p(wd), _p(rank_d), cells, _p(sd), sp) == 0
    assert L.shacira_spc_accumulate_points(cloud.shape[0], _p(cloud), _p(cloud_rgb), level, _p(wd), _p(rank_d), cells, _p(sq),
                                           sp) == 0
    assert L.shacira_spc_resolve(cells, _p(sd), _p(colors), sp) == 0
    stream.synchronize()
    assert torch.equal(sd, sq)
    return words, rank, cells, sd.cpu().numpy(), colors.cpu().numpy()


def check_case(c, stream=None, levels=(1, 2, 5)):
    stream = stream if stream is not None else torch.cuda.current_stream(c.dev)
    M = int(c.valid.sum())
    cloud, rgb = run_cloud(c, stream)
    again, rgb_again = run_cloud(c, stream)
    assert torch.equal(cloud.view(torch.int32), again.view(torch.int32)) and torch.equal(rgb, rgb_again)      # two calls, the same bits
    pts = cloud.cpu().numpy()
    assert pts.shape == (M, 3) and not (pts == SENT).any()
    err = np.abs(pts.astype(np.float64) - c.ref["points"][c.valid])
    finite = np.isfinite(c.ref["points"][c.valid])
    assert (err[finite] <= c.ref["bound"][c.valid][finite]).all(), (err[finite] / U).max()
    assert np.array_equal(rgb.cpu().numpy(), c.bytes_ref)
    if c.V:
        bounds, count = run_bounds(c, stream)
        assert count == M
        if M:       # min and max of the kernel's own points, bit for bit: the order cannot matter
            assert np.array_equal(bounds[:3], pts.min(axis=0)) and np.array_equal(bounds[3:], pts.max(axis=0))
        else:
            assert bounds.tolist() == [math.inf] * 3 + [-math.inf] * 3
    for level in levels:
        words, rank, cells, sums, colors = build_spc(c, level, cloud, rgb, stream)
        keys, keep = S.cells_ref(pts, level)
        assert np.array_equal(words, S.words_ref(keys, level))
        want_sums, want_colors = S.colors_ref(keys, c.bytes_ref[keep], words, rank, cells)
        assert np.array_equal(sums, want_sums) and np.array_equal(colors, want_colors)
    return pts


# pixel counts 1, 63, 64, 65, 257, 1025 and the 5 x 3 and 17 x 9 images with one and three views
SHAPES = [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (1, 1, 257), (1, 25, 41), (1, 3, 5), (3, 3, 5), (1, 9, 17), (3, 9, 17)]


@pytest.mark.parametrize("shape", SHAPES)
def test_depth_sources_shapes(dev, shape):
    V, H, W = shape
    k = SHAPES.index(shape)
    check_case(Case(dev, V, H, W, lens="ortho" if k % 3 == 1 else "pinhole", channels=3 if k % 2 else 4, bg_black=k % 4 >= 2,
                    plane="sprinkled" if k % 2 else "valid", seed=k))


@pytest.mark.parametrize("plane", ["invalid", "valid", "sprinkled", "zero"])
@pytest.mark.parametrize("lens", ["pinhole", "ortho"])
def test_depth_planes(dev, plane, lens):
    check_case(Case(dev, 3, 9, 17, lens=lens, channels=4, bg_black=lens == "ortho", plane=plane, seed=11))


def test_depth_mip_sums_and_side_stream(dev):
    side = torch.cuda.Stream(dev)
    for channels, bg in ((4, False), (3, True), (4, True)):
        check_case(Case(dev, 3, 9, 17, channels=channels, bg_black=bg, plane="sprinkled", mip=1, seed=5), stream=side)
    check_case(Case(dev, 1, 25, 41, channels=4, plane="sprinkled", seed=6), stream=side)


def test_no_views_is_a_no_op(dev):
    c = Case(dev, 0, 3, 5)
    L, sp = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    bounds, count = torch.full((6,), SENT, device=dev), torch.full((1,), -5, dtype=torch.int64, device=dev)
    words = torch.zeros((1,), dtype=torch.int32, device=dev)
    assert L.shacira_depth_bounds(*c.head, _p(bounds), _p(count), sp) == 0
    assert L.shacira_depth_points_count(*c.head, None, sp) == 0
    assert L.shacira_spc_mark_depth(*c.head, 1, _p(words), sp) == 0
    assert L.shacira_spc_mark_points(0, None, 1, None, sp) == 0
    assert L.shacira_spc_resolve(0, None, None, sp) == 0
    assert L.shacira_spc_first_hit(0, None, None, 1, None, None, None, None, None, None, None, sp) == 0
    torch.cuda.synchronize()
    assert (bounds == SENT).all() and int(count) == -5 and int(words) == 0            # nothing was enqueued
    b, n = hip_ops.depth_bounds(c.rec_d, c.depth_d)
    assert b.tolist() == [math.inf] * 3 + [-math.inf] * 3 and int(n) == 0
    pts, cols = hip_ops.depth_points(c.rec_d, c.depth_d, c.img_d)
    assert pts.shape == (0, 3) and cols.shape == (0, 3)


def test_validation_precedes_launch(dev):
    c = Case(dev, 1, 3, 5)
    L, sp, E = _lib.lib(), None, _lib.EINVAL
    out = torch.zeros(64, dtype=torch.int64, device=dev)
    assert L.shacira_depth_bounds(_p(c.rec_d), 1, 0, 3, _p(c.depth_d), _p(out), _p(out), sp) == E
    assert L.shacira_depth_bounds(_p(c.rec_d), -1, 5, 3, _p(c.depth_d), _p(out), _p(out), sp) == E
    assert L.shacira_depth_bounds(_p(c.rec_d), 1, 5, 3, None, _p(out), _p(out), sp) == E
    assert L.shacira_depth_points_emit(*c.head, _p(c.img_d), 5, 0, 0, _p(out), _p(out), _p(out), sp) == E
    assert L.shacira_depth_points_emit(*c.head, _p(c.img_d), 4, 5, 0, _p(out), _p(out), _p(out), sp) == E
    assert L.shacira_depth_points_emit(*c.head, _p(c.img_d), 4, 0, 2, _p(out), _p(out), _p(out), sp) == E
    assert L.shacira_spc_mark_depth(*c.head, 0, _p(out), sp) == E
    assert L.shacira_spc_mark_points(4, _p(out), 11, _p(out), sp) == E
    assert L.shacira_spc_mark_points(-1, _p(out), 1, _p(out), sp) == E
    assert L.shacira_spc_rank(3, None, _p(out), sp) == E
    assert L.shacira_spc_accumulate_points(4, _p(out), None, 1, _p(out), _p(out), 1, _p(out), sp) == E
    assert L.shacira_spc_resolve(-1, _p(out), _p(out), sp) == E
    assert L.shacira_spc_first_hit(4, _p(out), _p(out), 0, _p(out), None, None, _p(out), _p(out), _p(out), None, sp) == E
    assert L.shacira_spc_first_hit(4, _p(out), _p(out), 1, _p(out), None, _p(out), _p(out), _p(out), _p(out), None, sp) == E
    assert L.shacira_spc_num_words(0) == 0 and L.shacira_spc_num_words(11) == 0


# ---- explicit clouds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 5])
def test_points_edges(dev, level):
    G = 1 << level
    w = 2.0 / G
    centre = lambda x, y, z: [-1 + (x + 0.5) * w, -1 + (y + 0.5) * w, -1 + (z + 0.5) * w]
    pts = [[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [1.0, -1.0, 0.25], [5.0, -9.0, 0.1], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],
           centre(0, 0, 0), centre(0, 0, min(31, G - 1)),                 # bit 0 and bit 31 (level 1: bit 1) of the first word
           centre(G - 1, G - 1, G - 1), centre(G - 1, G - 1, max(G - 32, 0))]            # the last word: its last and first bit
    cols = [[k, 2 * k, 255 - k] for k in range(len(pts))]
    a, b = centre(G // 2, 0, G - 1), centre(0, G - 1, G // 2)
    rng = np.random.default_rng(level)
    crowd = rng.integers(0, 256, (1025, 3))
    pts += [a] * 1025 + [b, b]
    cols += crowd.tolist() + [[0, 255, 7], [1, 254, 8]]                 # two points: means 0.5 (a tie, up), 254.5 (up), 7.5
    pts, cols = np.array(pts, np.float32), np.array(cols, np.uint8)
    words, rank, colors, cells = hip_ops.spc_from_points(torch.from_numpy(pts).to(dev), torch.from_numpy(cols).to(dev), level)
    keys, keep = S.cells_ref(pts, level)
    assert keep.sum() == len(pts) - 2
    want_words = S.words_ref(keys, level)
    want_rank, want_cells = S.rank_ref(want_words)
    sums, want_colors = S.colors_ref(keys, cols[keep], want_words, want_rank, want_cells)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want_words) and cells == want_cells
    assert np.array_equal(rank.cpu().numpy(), want_rank) and np.array_equal(colors.cpu().numpy(), want_colors)
    ka = S.cells_ref(np.array([a], np.float32), level)[0]
    kb = S.cells_ref(np.array([b], np.float32), level)[0]
    sa, sb = int(S.slots_ref(ka, want_words, want_rank)[0]), int(S.slots_ref(kb, want_words, want_rank)[0])
    if level > 1:           # at level 1 the eight cells are shared with the special points
        assert sums[sa].tolist() == crowd.sum(axis=0).tolist() + [1025]
        assert want_colors[sb].tolist() == [1, 255, 8, 255]
    # the same set as OctreeAS.from_pointcloud on the same fp32 points
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.ops.spc import StructuredPointCloud
    blas = OctreeAS.from_pointcloud(torch.from_numpy(pts), level)
    spc = StructuredPointCloud(level, words, rank, colors, cells)
    assert torch.equal(spc.to_octree_as().occupancy_grid.cpu(), blas.occupancy_grid)


# ---- first hit -----------------------------------------------------------------------------------------------------------------
def occupancy(kind, level, rng):
    G = 1 << level
    occ = np.zeros((G, G, G), bool)
    if kind == "dense":
        occ[:] = True
    elif kind == "first":
        occ[0, 0, 0] = True
    elif kind == "last":
        occ[G - 1, G - 1, G - 1] = True
    elif kind == "random":
        occ = rng.random((G, G, G)) < 0.08
    return occ


def rays_for(occ, level, N, rng):
    """N rays: the special ones first (as many as fit), random ones towards the cube after them."""
    G = 1 << level
    w = 2.0 / G
    cells = np.argwhere(occ)
    inside = (-1 + (cells[0] + 0.5) * w) if len(cells) else np.zeros(3)
    empty = np.argwhere(~occ)
    hollow = (-1 + (empty[len(empty) // 2] + 0.5) * w) if len(empty) else np.zeros(3)
    far = -1 + (np.array([G - 1, G - 1, G - 1]) + 0.5) * w
    special = [
        ([-2.0, inside[1], inside[2]], [1, 0, 0]), ([inside[0], 3.0, inside[2]], [0, -1, 0]), ([inside[0], inside[1], -1.5], [0, 0, 1]),
        ([-2.0, -2.0, inside[2]], [1, 1, 0]), ([-2.0, far[1], -2.0], [0.6, 0, 0.8]),                  # zero components
        (inside, [0.3, -0.5, 0.81]), (inside, [0, 0, 0]),                                               # inside an occupied cell
        (hollow, [0.48, 0.6, -0.64]), (hollow, [0, 0, 0]),                                              # inside, in empty space
        ([-2.0, 0.1, 0.2], [-1, 0, 0]), ([0.2, 3.0, 0.1], [0.1, 1, 0.1]),                               # pointing away
        ([-2.0, 1.0, 0.3], [1, 0, 0]), ([-2.0, -1.0, -1.0], [1, 0, 0]), ([-2.0, -2.0, -2.0], [1, 1, 1]),   # grazing faces, an edge, the diagonal
        ([-3.0, -1.0 + w, 0.1], [1, 0, 0]), ([1.5, 1.5, 1.5], [-1, -1, -1]),
        ([np.nan, 0, 0], [1, 0, 0]), ([0, 0, -2.0], [0, np.inf, 1]), ([-np.inf, 0, 0], [1, 0, 0]), ([0, 0, -2.0], [0, np.nan, 1]),
    ]
    o = np.array([s[0] for s in special], np.float32)
    d = np.array([s[1] for s in special], np.float32)
    more = max(N - len(special), 0)
    ro = rng.normal(size=(more, 3))
    ro = 2.5 * ro / np.linalg.norm(ro, axis=1, keepdims=True)
    rd = rng.uniform(-0.9, 0.9, (more, 3)) - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    # N below the number of special rays: the non-finite ones (the last four) stay in
    keep = list(range(N - 4)) + list(range(len(special) - 4, len(special))) if 4 < N < len(special) else list(range(min(N, len(special))))
    return np.concatenate([o[keep], ro.astype(np.float32)]), np.concatenate([d[keep], rd.astype(np.float32)])


def first_nuggets(o, d, occ_d, level):
    """(depth, hit, pidx) per ray from the parent's raytrace_dense: the first nugget of every ray that has one."""
    N = o.shape[0]
    ridx, pidx, depth = render.raytrace_dense(o, d, occ_d, level)
    first = render.mark_pack_boundaries(ridx)
    rows = ridx[first].long()
    out_d = torch.zeros(N, device=o.device)
    out_h = torch.zeros(N, dtype=torch.bool, device=o.device)
    out_p = torch.full((N,), -1, dtype=torch.int32, device=o.device)
    out_d[rows], out_h[rows], out_p[rows] = depth[first][:, 0], True, pidx[first].to(torch.int32)
    return out_d, out_h, out_p


@pytest.mark.parametrize("kind,level", [("empty", 2), ("dense", 1), ("dense", 5), ("first", 2), ("last", 2), ("first", 5),
                                        ("last", 5), ("random", 5)])
def test_first_hit_equals_first_nugget(dev, kind, level):
    from shacira_amd.wisp.ops.spc.structured import pack_occupancy
    rng = np.random.default_rng(level * 10 + len(kind))
    occ = occupancy(kind, level, rng)
    occ_d = torch.from_numpy(occ).to(dev)
    words = pack_occupancy(occ_d)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), S.words_ref(np.flatnonzero(occ.reshape(-1)), level))
    rank_h, cells = S.rank_ref(words.cpu().numpy().view(np.uint32))
    rank = torch.from_numpy(rank_h).to(dev)
    colors = torch.from_numpy(rng.integers(0, 256, (cells, 4), dtype=np.uint8)).to(dev)
    L = _lib.lib()
    for N in (1, 63, 64, 65, 257):
        o_h, d_h = rays_for(occ, level, N, rng)
        assert o_h.shape == (N, 3)
        o, d = torch.from_numpy(o_h).to(dev), torch.from_numpy(d_h).to(dev)
        bad = ~(np.isfinite(o_h).all(axis=1) & np.isfinite(d_h).all(axis=1))
        depth = torch.full((N,), SENT, device=dev)
        hit = torch.full((N,), 9, dtype=torch.uint8, device=dev)
        pidx = torch.full((N,), -9, dtype=torch.int32, device=dev)
        rgb = torch.full((N, 3), SENT, device=dev)
        torch.cuda.synchronize()
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with_colors = cells > 0
        assert L.shacira_spc_first_hit(N, _p(o), _p(d), level, _p(words), _p(rank) if with_colors else None,
                                       _p(colors) if with_colors else None, _p(depth), _p(hit), _p(pidx),
                                       _p(rgb) if with_colors else None, sp) == 0
        torch.cuda.synchronize()
        # the oracle never sees the rays that are not finite: they are a miss by contract, and disturb no other row
        o_f, d_f = o.clone(), d.clone()
        bad_d = torch.from_numpy(bad).to(dev)
        o_f[bad_d], d_f[bad_d] = torch.tensor([3.0, 3.0, 3.0], device=dev), torch.tensor([1.0, 0.0, 0.0], device=dev)
        want_d, want_h, want_p = first_nuggets(o_f, d_f, occ_d, level)
        assert not bool(want_h[bad_d].any())
        assert torch.equal(hit, want_h.to(torch.uint8)) and torch.equal(pidx, want_p)
        assert torch.equal(depth.view(torch.int32), want_d.view(torch.int32))                        # bit for bit
        if with_colors:
            hits = hit.bool().cpu().numpy()
            got = rgb.cpu().numpy()
            assert (got[~hits] == 0).all()
            if hits.any():
                from shacira_amd.wisp.ops.spc import StructuredPointCloud
                spc = StructuredPointCloud(level, words, rank, colors, cells)
                slots = spc.slots_of(pidx[hit.bool()])
                want = colors[slots, :3].float() / torch.full((1,), 255.0, device=dev)
                assert torch.equal(rgb[hit.bool()], want)
        if kind == "empty":
            assert not bool(hit.any())
        if kind == "dense" and N >= 63:
            assert bool(hit.any()) and bool((depth[hit.bool()] == 0).any())                          # a start inside a cell
    # OctreeAS.first_hit: the same kernel without colours
    from shacira_amd.wisp.accelstructs import OctreeAS
    blas = OctreeAS(level, occ_d)
    h2, p2, d2 = blas.first_hit(Rays(o_f, d_f), level)
    assert torch.equal(h2, want_h) and torch.equal(p2, want_p) and torch.equal(d2, want_d)
    assert blas.packed_occupancy(level) is not None


def test_tracer_equals_composed(dev):
    from shacira_amd.wisp.models.nefs import SPCField
    from shacira_amd.wisp.ops.spc import StructuredPointCloud
    from shacira_amd.wisp.tracers import PackedSPCTracer
    rng = np.random.default_rng(7)
    pts = torch.from_numpy(rng.uniform(-0.7, 0.7, (4000, 3)).astype(np.float32)).to(dev)
    cols = torch.from_numpy(rng.integers(0, 256, (4000, 3), dtype=np.uint8)).to(dev)
    spc = StructuredPointCloud.from_pointcloud(pts, cols, 5)
    occ = spc.to_octree_as().occupancy_grid.cpu().numpy()
    o_h, d_h = rays_for(occ, 5, 257, rng)
    ok = np.isfinite(o_h).all(axis=1) & np.isfinite(d_h).all(axis=1)
    rays = Rays(torch.from_numpy(o_h[ok]).to(dev), torch.from_numpy(d_h[ok]).to(dev))
    tracer = PackedSPCTracer()
    for nef in (SPCField(spc), SPCField(spc.to_octree_as(), dict(colors=spc.colors_morton()))):
        fused, composed = tracer(nef, rays), tracer.trace_composed(nef, rays, {"rgb"}, set())
        assert fused.depth.shape == (rays.origins.shape[0], 1) and fused.hit.dtype == torch.bool
        assert bool(fused.hit.any()) and not bool(fused.hit.all())
        for name in ("depth", "hit", "rgb", "alpha"):
            assert torch.equal(getattr(fused, name), getattr(composed, name)), name


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_rtmv_end_to_end(dev, tmp_path):
    from shacira_amd.wisp.datasets import RTMVDataset
    from shacira_amd.wisp.models.nefs import SPCField
    from shacira_amd.wisp.tracers import PackedSPCTracer
    V, H, W, level = 6, 16, 24, 5
    G = 1 << level
    harness.write_analytic_rtmv(str(tmp_path), V, H, W, seed=0)
    ds = RTMVDataset(str(tmp_path), "white", train_ratio=1.0, val_ratio=0.0, device=dev)
    host = RTMVDataset(str(tmp_path), "white", train_ratio=1.0, val_ratio=0.0, device="cpu")
    assert len(ds) == V and ds.resident_bytes() == V * H * W * 8 + V * 80
    ref = S.points_ref(ds.records.cpu().numpy(), W, H, ds.depth.cpu().numpy())
    valid, bound = ref["valid"], ref["bound"]
    cloud = ds.as_pointcloud().cpu().numpy()
    assert (np.abs(cloud.astype(np.float64) - ref["points"][valid]) <= bound[valid]).all()
    # the device normalisation against the host restatement: the same rule on clouds that differ by the carried bound
    assert abs(ds.coords_scale - host.coords_scale) <= 64 * U * host.coords_scale
    assert float(np.abs(cloud).max()) <= 1.0 + 2 * bound.max() + 16 * U
    spc = ds.as_spc(level)
    keys, keep = S.cells_ref(cloud, level)
    assert keep.all() and np.array_equal(spc.words.cpu().numpy().view(np.uint32), S.words_ref(keys, level))
    nef, tracer = SPCField(spc), PackedSPCTracer()
    s, c = ds.coords_scale, ds.coords_center.double().numpy()
    centre, radius = -c * s, harness.ANALYTIC_RTMV_RADIUS * s
    excluded = total = 0
    for i in (0, 3):
        view = ds[i]
        rb = tracer(nef, view["rays"])
        hit = rb.hit.cpu().numpy()
        o, d = view["rays"].origins.cpu().numpy().astype(np.float64), view["rays"].dirs.cpu().numpy().astype(np.float64)
        p = o + d * rb.depth.cpu().numpy().astype(np.float64)
        lo = i * H * W
        slack = 2 * math.sqrt(3) / G + np.linalg.norm(bound[lo:lo + H * W], axis=1).max()
        # depth 1e10 pixels are "valid" only before the loader's rule: here they are NaN, so nothing hits from the background
        assert (np.abs(np.linalg.norm(p[hit] - centre, axis=1) - radius) <= slack).all()
        v = valid[lo:lo + H * W]
        cell = ref["points"][lo:lo + H * W] * (G / 2) + G / 2
        near = (np.abs(cell - np.round(cell)) <= bound[lo:lo + H * W] * (G / 2)).any(axis=1)
        assert hit[v & ~near].all()
        excluded += int((v & near).sum())
        total += int(v.sum())
        assert torch.equal(view["alpha"][:, 0].cpu(), torch.from_numpy(v))
    assert total > 0 and excluded <= 0.02 * total, (excluded, total)
    out = harness.render_spc(ds, level)
    assert len(out) == V and out[0].rgb.shape == (H, W, 3) and bool(out[0].hit.any())


def test_rtmv_mip_level(dev, tmp_path):
    """``mip=1`` on the device: the colours are the level's uint16 sums, the depth is the block's top-left pixel, the intrinsics
    follow the image plane, and the fused SPC equals the SPC of the emitted cloud bit for bit."""
    from shacira_amd.wisp.datasets import RTMVDataset
    from shacira_amd.wisp.ops.spc import StructuredPointCloud
    V, H, W = 3, 16, 24
    harness.write_analytic_rtmv(str(tmp_path), V, H, W, seed=2)
    kw = dict(train_ratio=1.0, val_ratio=0.0)
    full = RTMVDataset(str(tmp_path), "black", device="cpu", **kw)
    ds = RTMVDataset(str(tmp_path), "black", mip=1, device=dev, coords_center=full.coords_center, coords_scale=full.coords_scale,
                     **kw)
    assert tuple(ds.img_shape) == (H // 2, W // 2, 3) and ds.images.dtype == torch.uint16
    assert tuple(ds.images.shape) == (V, H // 2, W // 2, 4) and ds.coords_scale == full.coords_scale
    assert torch.equal(ds.images.cpu().to(torch.int32), image_mip_torch(full.images, 1))
    want = full.depth[:, ::2, ::2]
    assert torch.equal(torch.isfinite(ds.depth).cpu(), torch.isfinite(want))
    assert torch.equal(torch.nan_to_num(ds.depth).cpu(), torch.nan_to_num(want))
    assert torch.equal(ds.records[:, :14].cpu(), full.records[:, :14])           # pose and field of view are the full level's
    assert ds.resident_bytes() == V * (H // 2) * (W // 2) * 12 + V * 80
    pts, cols = ds.as_colored_pointcloud()
    assert pts.shape[0] == int(torch.isfinite(want).sum()) and cols.shape == pts.shape
    fused, two_step = ds.as_spc(4), StructuredPointCloud.from_pointcloud(pts, cols, 4)
    assert fused.num_cells == two_step.num_cells > 0
    for name in ("words", "rank", "colors"):
        assert torch.equal(getattr(fused, name), getattr(two_step, name)), name
    view = ds[1]
    assert view["depth"].shape == (H * W // 4, 1) and view["rgb"].shape == (H * W // 4, 3)
    assert torch.equal(view["alpha"][:, 0].cpu(), torch.isfinite(want[1]).reshape(-1))
