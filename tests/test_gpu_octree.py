"""OctreeGrid / CodebookOctreeGrid on the MI355X: the HIP octree kernels against the fp64 restatement (tests/octree_ref.py)
and the torch composition ``octree_torch`` on the same GPU, the autograd surface, graph capture, the modules, marching on
a coarser level and two training runs.

Bounds (eps = fp32 epsilon, L = levels of the call):
  forward               |got - ref| <= (16 + L) eps sum|w||v|: 5 roundings in a weight, 1 in the product, 7 in the eight-term
                        sum, L - 1 across levels, rounded up.
  feature gradients     1e-5 of each level's largest entry (the bar of test_gpu_triplane.py), N <= 2^18, standard-normal
                        grad_output.
  coordinate gradient   K eps gscale + 1e-6 with gscale the restatement's absolute sum and K = 8 F L + 8, the worst-case
                        linear bound on the term count; bitwise equal across two runs.
The restatement locates cells in fp32 exactly as the contract states, so no sample is excluded for lying near a cell face.
Every sample of every batch is compared with the restatement (numpy, fp64, evaluated in blocks of 65 536 samples), the 2^20
batches included.

The cases cover every value the lookup is specified for -- occupancies dense / shell / random, 'sum' and 'cat', F in
{1, 2, 4, 5, 8, 16} plus the runtime-F path (3, 32), levels [5, 6, 7, 8] / [3] / [2, 6], N in {0, 1, 63, 2^16 + 3, 2^20},
uniform and ray-ordered coordinates -- as a covering set and not as the full product (1 080 cases with a numpy yardstick).
"""
import warnings

import numpy as np
import pytest
import torch

import octree_ref as oref

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_AS = {}


def _blas(kind, level):
    """occupancy ``kind`` at ``level`` (cached: the structures are read-only here)."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    if (kind, level) not in _AS:
        if kind == "dense":
            _AS[kind, level] = OctreeAS.make_dense(level)
        else:
            cells = oref.shell_cells(level) if kind == "shell" else oref.random_cells(level)
            _AS[kind, level] = OctreeAS.from_quantized_points(torch.from_numpy(cells), level)
    return _AS[kind, level]


_INDEX = {}


def _index(kind, levels):
    from shacira_amd.wisp.ops.octree import build_octree_index
    key = (kind, tuple(levels))
    if key not in _INDEX:
        _INDEX[key] = build_octree_index(_blas(kind, max(levels)), levels)
    return _INDEX[key]


def _tables(rng, index, levels, fdim, dev):
    return [torch.from_numpy(rng.standard_normal((index[l].rows + 1, fdim)).astype(np.float32)).to(dev) for l in levels]


def _uniform(rng, n, dev, spread=1.3):
    return torch.from_numpy(rng.uniform(-spread, spread, (n, 3)).astype(np.float32)).to(dev)


def _ray_ordered(n, dev, steps=64, seed=0):
    """n samples ray by ray: ``steps`` equidistant points on every camera ray between depths 1.5 and 4.5."""
    from shacira_amd import harness
    rays = max(1, (n + steps - 1) // steps)
    o, d = harness.camera_rays(rays, torch.Generator().manual_seed(seed), dev)
    t = torch.linspace(1.5, 4.5, steps, device=dev)
    return (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3)[:n].contiguous()


def _coords(kind, rng, n, dev):
    return _uniform(rng, n, dev) if kind == "uniform" else _ray_ordered(n, dev)


def _np_index(index, levels):
    return ([index[l].level_points.cpu().numpy() for l in levels], [index[l].trinkets.cpu().numpy() for l in levels])


def _check_forward(coords, index, levels, tables, summed):
    from shacira_amd import hip_ops
    dev = coords.device
    got = hip_ops.octree_forward(coords, [index[l].to(dev) for l in levels], tables, summed)
    n, L = coords.shape[0], len(levels)
    assert got.shape == (n, tables[0].shape[1] * (1 if summed else L)) and got.dtype == torch.float32
    if n == 0:
        return got
    c_all, g_all = coords.cpu().numpy(), got.cpu().double().numpy()
    lp, tr = _np_index(index, levels)
    nt = [t.cpu().numpy() for t in tables]
    worst, hits = 0.0, 0
    for s0 in range(0, n, 65536):                                  # the whole batch, block by block
        c, g = c_all[s0:s0 + 65536], g_all[s0:s0 + 65536]
        ref = oref.forward(c, levels, lp, tr, nt, summed)
        scale = oref.abs_forward(c, levels, lp, tr, nt, summed)
        err = np.abs(g - ref)
        worst = max(worst, float((err / np.maximum(scale, 1e-30)).max() / EPS))
        hits += int((scale.sum(-1) > 0).sum())
        assert np.all(err <= (16 + L) * EPS * scale), worst
    print(f"forward: worst error {worst:.2f} eps sum|w||v| (bound {16 + L}); hits {hits / n:.3f}")
    # every sample: exact zeros where no level is occupied (the structure's own query says which)
    miss = torch.ones(n, dtype=torch.bool, device=dev)
    for l in levels:
        miss &= index.source.query(coords, l).pidx < 0
    assert (got[miss] == 0).all()
    from shacira_amd.wisp.ops.octree import octree_torch
    dev_torch = float((got - octree_torch(coords, levels, tables, index, summed)).abs().max())
    assert dev_torch <= 1e-4, dev_torch
    return got


FORWARD_CASES = [
    ("dense", [5, 6, 7, 8], 5, 1 << 20, "uniform", True),
    ("shell", [5, 6, 7, 8], 5, 1 << 20, "ray", True),
    ("shell", [5, 6, 7, 8], 4, (1 << 16) + 3, "uniform", False),
    ("random", [5, 6, 7, 8], 16, (1 << 16) + 3, "ray", False),
    ("random", [5, 6, 7, 8], 5, (1 << 16) + 3, "uniform", False),
    ("random", [5, 6, 7, 8], 4, 1 << 20, "uniform", True),
    ("dense", [3], 1, 63, "uniform", True),
    ("dense", [3], 16, 0, "uniform", False),
    ("random", [2, 6], 2, 1, "uniform", False),
    ("shell", [2, 6], 8, (1 << 16) + 3, "ray", True),
    ("dense", [2, 6], 2, 63, "ray", False),
    ("shell", [2, 6], 3, 4099, "uniform", True),
    ("random", [3], 32, 63, "uniform", False),
    ("shell", [3], 8, 1, "ray", True),
]


@pytest.mark.parametrize("occ,levels,fdim,n,kind,summed", FORWARD_CASES)
def test_forward_against_restatement(dev, occ, levels, fdim, n, kind, summed):
    rng = np.random.default_rng(n + fdim)
    index = _index(occ, levels)
    tables = _tables(rng, index, levels, fdim, dev)
    _check_forward(_coords(kind, rng, n, dev), index, levels, tables, summed)


def _check_backward(coords, index, levels, tables, summed, go):
    from shacira_amd import hip_ops
    dev = coords.device
    li = [index[l].to(dev) for l in levels]
    F, L = tables[0].shape[1], len(levels)
    grads, gc = hip_ops.octree_backward(coords, li, F, go, summed, features=tables, need_features=True, need_coords=True)
    _, gc2 = hip_ops.octree_backward(coords, li, F, go, summed, features=tables, need_features=False, need_coords=True)
    assert torch.equal(gc, gc2)                                    # a gather: the same bits every run
    lp, tr = _np_index(index, levels)
    nt = [t.cpu().numpy() for t in tables]
    rt, rc, rs = oref.backward(coords.cpu().numpy(), levels, lp, tr, nt, go.cpu().numpy(), summed)
    for l, (a, b) in enumerate(zip(grads, rt)):
        assert a.shape == b.shape
        assert (a[-1] == 0).all()                                  # the padding row
        err = float(np.abs(a.cpu().double().numpy() - b).max())
        big = float(np.abs(b).max())
        print(f"level {levels[l]}: feature gradient error {err:.3e}, largest entry {big:.3e} (bound 1e-5 of it)")
        assert err <= 1e-5 * big, (levels[l], err, big)
    K = 8 * F * L + 8
    err = np.abs(gc.cpu().double().numpy() - rc)
    print(f"coordinate gradient: worst {float((err / (EPS * rs + 1e-30)).max()):.2f} eps gscale (K = {K})")
    assert np.all(err <= K * EPS * rs + 1e-6)
    return grads, gc


BACKWARD_CASES = [
    ("shell", [5, 6, 7, 8], 5, 1 << 18, "uniform", True),
    ("dense", [5, 6, 7, 8], 5, 1 << 17, "ray", True),
    ("random", [5, 6, 7, 8], 4, (1 << 16) + 3, "uniform", False),
    ("dense", [2, 6], 4, 1 << 18, "ray", False),
    ("shell", [2, 6], 3, 4099, "uniform", True),
    ("dense", [3], 8, 63, "uniform", True),
    ("random", [3], 32, 1, "uniform", False),
    ("shell", [5, 6, 7, 8], 16, (1 << 16) + 3, "ray", False),
    ("dense", [3], 1, 1 << 16, "uniform", False),
    ("random", [2, 6], 2, 63, "ray", True),
]


@pytest.mark.parametrize("occ,levels,fdim,n,kind,summed", BACKWARD_CASES)
def test_gradients_against_restatement(dev, occ, levels, fdim, n, kind, summed):
    rng = np.random.default_rng(n * 3 + fdim)
    index = _index(occ, levels)
    tables = _tables(rng, index, levels, fdim, dev)
    coords = _coords(kind, rng, n, dev)
    go = torch.from_numpy(rng.standard_normal((n, fdim * (1 if summed else len(levels)))).astype(np.float32)).to(dev)
    _check_backward(coords, index, levels, tables, summed, go)


def test_level_9_wide_rows_take_the_direct_add_path(dev):
    """Levels [8, 9] at F = 32: the sort's block grid hits its cap of 64 blocks per axis (8^3 cells of level 9), the level-8
    window (5^3 points) fits LDS and the level-9 window (9^3 x 32 floats = 93 KB) does not, so level 9 adds straight to
    memory. Same bounds as everywhere else."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.ops.octree import build_octree_index
    rng = np.random.default_rng(21)
    levels, fdim, n = [8, 9], 32, (1 << 16) + 3
    centre = rng.standard_normal((150000, 3)) * 0.25
    cells = np.unique(np.clip(np.floor((centre + 1) * 256), 0, 511).astype(np.int64), axis=0)
    index = build_octree_index(OctreeAS.from_quantized_points(torch.from_numpy(cells), 9), levels)
    tables = _tables(rng, index, levels, fdim, dev)
    pick = cells[rng.integers(0, cells.shape[0], n)]
    inside = ((pick + rng.uniform(0, 1, pick.shape)) / 256 - 1).astype(np.float32)
    coords = torch.from_numpy(np.where(rng.uniform(size=(n, 1)) < 0.7, inside, rng.uniform(-1.3, 1.3, (n, 3)).astype(
        np.float32))).to(dev).contiguous()
    for summed in (True, False):
        got = _check_forward(coords, index, levels, tables, summed)
        assert float((got.abs().sum(-1) > 0).float().mean()) > 0.5
        _check_backward(coords, index, levels, tables, summed, torch.randn_like(got))


def test_feature_gradient_does_not_depend_on_the_batch_order_and_n_zero(dev):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(11)
    levels = [5, 6, 7, 8]
    index = _index("shell", levels)
    li = [index[l].to(dev) for l in levels]
    coords = _ray_ordered(1 << 16, dev)
    go = torch.randn(1 << 16, 5, device=dev)
    a, _ = hip_ops.octree_backward(coords, li, 5, go, True)
    perm = torch.randperm(1 << 16, device=dev)
    b, _ = hip_ops.octree_backward(coords[perm].contiguous(), li, 5, go[perm].contiguous(), True)
    for x, y in zip(a, b):
        assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max())
    empty, gc = hip_ops.octree_backward(coords[:0], li, 5, go[:0], True, features=_tables(rng, index, levels, 5, dev),
                                        need_coords=True)
    assert gc.shape == (0, 3) and all((g == 0).all() and g.shape[0] == index[l].rows + 1 for g, l in zip(empty, levels))


@pytest.mark.parametrize("occ", ["dense", "shell"])
def test_nonfinite_coordinates(dev, occ):
    rng = np.random.default_rng(2)
    levels = [3, 5] if occ == "dense" else [3, 6]
    index = _index(occ, levels)
    tables = _tables(rng, index, levels, 4, dev)
    vals = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.3, 1.0, -1.0], device=dev)
    coords = torch.cartesian_prod(vals, vals, vals).contiguous()
    finite_inside = (torch.isfinite(coords) & (coords < 1.0)).all(-1)
    for summed in (True, False):
        got = _check_forward(coords, index, levels, tables, summed)
        assert (got[~finite_inside] == 0).all() and torch.isfinite(got).all()
        if occ == "dense":
            assert (got[finite_inside].abs().sum(-1) > 0).all()
        go = torch.randn_like(got)
        grads, gc = _check_backward(coords, index, levels, tables, summed, go)
        assert (gc[~finite_inside] == 0).all() and torch.isfinite(gc).all()
        assert all(torch.isfinite(g).all() for g in grads)


def test_agreement_with_the_torch_composition(dev):
    """Forward and both gradients within 1e-4 absolute of ``octree_torch`` on standard-normal tables. The coordinate
    gradient grows with G / 2 and with F: at 1e-4 absolute and an fp32 epsilon of 6e-8 two evaluation orders can only agree
    while its entries stay below about a hundred, so this comparison runs at levels 3 and 4 with F = 2 (entries of a few
    tens) and 5 000 samples (about 50 addends per corner of level 3); the restatement tests above bound the finer levels
    relative to their scale."""
    from shacira_amd.wisp.ops.octree import octree_interpolate, octree_torch
    rng = np.random.default_rng(8)
    levels = [3, 4]
    for occ in ("dense", "random"):
        index = _index(occ, [3, 4] if occ == "dense" else [3, 4, 5])
        for summed in (True, False):
            tables = [t.requires_grad_(True) for t in _tables(rng, index, levels, 2, dev)]
            coords = _uniform(rng, 5000, dev, 1.1).requires_grad_(True)
            a = octree_interpolate(coords, levels, tables, index, summed)
            b = octree_torch(coords, levels, tables, index, summed)
            go = torch.randn_like(a)
            ga = torch.autograd.grad(a, [coords, *tables], go)
            gb = torch.autograd.grad(b, [coords, *tables], go)
            devs = [float((a - b).abs().max())] + [float((x - y).abs().max()) for x, y in zip(ga, gb)]
            print(f"{occ} {'sum' if summed else 'cat'}: deviations from octree_torch {['%.2e' % d for d in devs]}")
            assert max(devs) <= 1e-4, devs


def test_autograd_surface(dev):
    from shacira_amd.wisp.ops.octree import octree_interpolate, octree_torch
    rng = np.random.default_rng(7)
    levels = [3, 4]
    index = _index("dense", levels)
    tables = [t.requires_grad_(True) for t in _tables(rng, index, levels, 4, dev)]
    coords = _uniform(rng, 5000, dev, 1.1)
    out = octree_interpolate(coords, levels, tables, index, True)
    gt = torch.autograd.grad(out.square().sum(), tables)
    assert all(g is not None and g.shape == t.shape for g, t in zip(gt, tables))
    assert not coords.requires_grad and coords.grad is None
    c = coords.clone().requires_grad_(True)
    out = octree_interpolate(c, levels, tables, index, False)
    g = torch.autograd.grad(out.square().sum(), [c, tables[0]], create_graph=True)
    want = torch.autograd.grad(octree_torch(c, levels, tables, index, False).square().sum(), [c, tables[0]])
    assert torch.allclose(g[0], want[0], rtol=1e-4, atol=1e-3) and torch.allclose(g[1], want[1], rtol=1e-4, atol=1e-3)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g[0].sum(), c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        octree_interpolate(coords.cpu(), levels, [t.detach().cpu() for t in tables], index, True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_fallback_dtypes_warn_once_and_agree(dev, dtype):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.octree import octree_interpolate, octree_torch
    rng = np.random.default_rng(9)
    index = _index("dense", [3])
    tables = [t.to(dtype) for t in _tables(rng, index, [3], 2, dev)]
    coords = _uniform(rng, 300, dev, 1.0).to(dtype)
    hip_ops._warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = octree_interpolate(coords, [3], tables, index, True)
        octree_interpolate(coords, [3], tables, index, True)
    assert sum("octree lookup" in str(x.message) for x in w) == 1
    assert a.dtype == dtype and torch.equal(a, octree_torch(coords, [3], tables, index, True))


def test_graph_capture_replays_eager(dev):
    from shacira_amd.wisp.ops.octree import octree_interpolate
    rng = np.random.default_rng(10)
    levels = [5, 6, 7, 8]
    index = _index("shell", levels)
    tables = [t.requires_grad_(True) for t in _tables(rng, index, levels, 5, dev)]
    coords = _ray_ordered(1 << 16, dev).requires_grad_(True)
    go = torch.randn(1 << 16, 5, device=dev)

    def step():
        out = octree_interpolate(coords, levels, tables, index, True)
        return (out.detach(), *torch.autograd.grad(out, [coords, *tables], go))

    eager = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
    assert float(eager[0].abs().max()) > 0
    for a, b in zip(captured[2:], eager[2:]):
        assert torch.allclose(a, b, rtol=0, atol=1e-5 * float(b.abs().max()))


def test_module_shapes(dev):
    from shacira_amd.wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from shacira_amd.wisp.ops.octree import octree_torch
    torch.manual_seed(0)
    cells = torch.from_numpy(oref.shell_cells(5))
    for cls, kw in ((OctreeGrid, {}), (CodebookOctreeGrid, {"codebook_bitwidth": 3})):
        for ms in ("sum", "cat"):
            g = cls.from_quantized_points(cells, feature_dim=4, base_lod=3, num_lods=3, multiscale_type=ms,
                                          feature_std=0.5, **kw).to(dev)
            x3 = torch.rand(7, 5, 3, device=dev) * 2 - 1
            x2 = torch.rand(9, 3, device=dev) * 2 - 1
            for lod_idx in (0, 1, 2):
                K = 4 if ms == "sum" else 4 * (lod_idx + 1)
                assert g.interpolate(x3, lod_idx).shape == (7, 5, K)
                assert g.interpolate(x2, lod_idx).shape == (9, K)
                want = octree_torch(x2, g.active_lods[:lod_idx + 1], g._tables(lod_idx + 1), g.index, ms == "sum")
                assert torch.allclose(g.interpolate(x2, lod_idx), want, atol=1e-5)


def test_occupancy_change_rebuilds_the_index(dev):
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.models.grids import OctreeGrid
    torch.manual_seed(1)
    cells = torch.from_numpy(oref.shell_cells(5))
    g = OctreeGrid.from_quantized_points(cells, feature_dim=3, base_lod=5, num_lods=1, multiscale_type="sum",
                                         feature_std=1.0, feature_bias=2.0).to(dev)
    centres = ((cells.float() + 0.5) / 16 - 1).to(dev)
    before = g.interpolate(centres, 0)
    assert (before.abs().sum(-1) > 0).all()
    old_index = g.index
    g.blas = OctreeAS.from_quantized_points(cells[::2], 5)
    after = g.interpolate(centres, 0)
    assert g.index is not old_index and g.features[0].shape[0] == g.points_dual[5].shape[0] + 1
    assert (after[1::2] == 0).all()                                     # dropped cells
    assert torch.allclose(after[::2], before[::2], atol=1e-6)          # surviving cells keep their corner rows


def test_raymarch_runs_at_base_lod_inside_occupied_cells(dev):
    from shacira_amd import harness
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import OctreeGrid
    cells = torch.from_numpy(oref.shell_cells(6))
    g = OctreeGrid.from_quantized_points(cells, feature_dim=2, base_lod=4, num_lods=3)
    o, d = harness.camera_rays(2000, torch.Generator().manual_seed(4), dev)
    rays = Rays(o, d, 1.0, 5.0)
    m = g.raymarch(rays, raymarch_type="ray", num_samples=128)
    assert m.samples.shape[0] > 10000
    assert (g.blas.query(m.samples, g.base_lod).pidx >= 0).all()
    finest = g.blas.query(m.samples, 6).pidx >= 0
    assert 0 < int(finest.sum()) < m.samples.shape[0]                   # marched on level 4, which is coarser than the shell
    hits = g.raytrace(rays, level=4, with_exit=True)
    mid = o[hits.ridx.long()] + d[hits.ridx.long()] * hits.depth.mean(-1, keepdim=True)
    long_enough = (hits.depth[:, 1] - hits.depth[:, 0]) > 1e-3
    assert (g.blas.query(mid[long_enough], 4).pidx == hits.pidx.long()[long_enough]).all()


def _scene_cells(level=7, coarse=5):
    """cells of ``level`` inside the cells of ``coarse`` where the analytic scene has density, widened by one cell."""
    from shacira_amd import harness
    G = 1 << coarse
    idx = torch.stack(torch.meshgrid(*[torch.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 3)
    density, _ = harness.analytic_scene((idx.float() + 0.5) * (2.0 / G) - 1.0)
    occ = (density[:, 0] > 0.5).reshape(1, 1, G, G, G).float()
    occ = torch.nn.functional.max_pool3d(occ, 3, 1, 1)[0, 0] > 0
    s = 1 << (level - coarse)
    fine = occ.repeat_interleave(s, 0).repeat_interleave(s, 1).repeat_interleave(s, 2)
    return torch.nonzero(fine)


def _fit(nef, grid, dev, steps, lr_grid=1e-2):
    from shacira_amd import harness
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.tracers import PackedRFTracer
    truth = harness._AnalyticNef(grid)
    tracer = PackedRFTracer(raymarch_type="ray", num_steps=96, bg_color="white")
    gt_tracer = PackedRFTracer(raymarch_type="ray", num_steps=384, bg_color="white")
    opt = torch.optim.Adam([{"params": grid.parameters(), "lr": lr_grid},
                            {"params": [p for n, p in nef.named_parameters() if not n.startswith("grid.")], "lr": 1e-3}])
    gen = torch.Generator().manual_seed(1)
    losses = []
    for _ in range(steps):
        o, d = harness.camera_rays(2048, gen, dev)
        rays = Rays(o, d, dist_min=1.2, dist_max=4.8)
        with torch.no_grad():
            target = gt_tracer(truth, rays).rgb
        loss = (tracer(nef, rays).rgb - target).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses


def test_nerf_on_a_sparse_octree_grid_trains(dev):
    from shacira_amd.wisp.models.grids import OctreeGrid
    from shacira_amd.wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    grid = OctreeGrid.from_quantized_points(_scene_cells(8, 5), feature_dim=5, base_lod=5, num_lods=4,
                                            multiscale_type="sum", feature_std=0.01)
    assert grid.blas.points.shape[0] < 0.5 * 256 ** 3
    nef = NeuralRadianceField(grid, view_embedder="positional", view_multires=4, hidden_dim=64, num_layers=1).to(dev)
    with pytest.raises(NotImplementedError):
        nef.prune()
    losses = _fit(nef, grid, dev, 300)
    first, last = np.mean(losses[:20]), np.mean(losses[-20:])
    print(f"NeRF on a sparse OctreeGrid: L1 {first:.4f} -> {last:.4f}")
    assert last < 0.6 * first, (first, last)


def test_codebook_grid_trains_for_50_steps(dev):
    from shacira_amd.wisp.models.grids import CodebookOctreeGrid
    from shacira_amd.wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    grid = CodebookOctreeGrid.from_quantized_points(_scene_cells(6, 5), feature_dim=4, base_lod=4, num_lods=3,
                                                    multiscale_type="sum", feature_std=0.1, codebook_bitwidth=4)
    nef = NeuralRadianceField(grid, view_embedder="positional", view_multires=4, hidden_dim=64, num_layers=1).to(dev)
    losses = _fit(nef, grid, dev, 50)
    first, last = np.mean(losses[:10]), np.mean(losses[-10:])
    print(f"NeRF on a CodebookOctreeGrid: L1 {first:.4f} -> {last:.4f}")
    assert np.all(np.isfinite(losses)) and last < first, (first, last)
