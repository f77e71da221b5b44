"""TriplanarGrid on the MI355X: the HIP triplane kernels against the fp64 restatement (tests/triplane_ref.py) and torch's
own grid_sample composition on the same GPU, the autograd surface, the modules, the AABB structure and a NeRF fit."""
import warnings

import numpy as np
import pytest
import torch

import triplane_ref as tr

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _planes(rng, fdim, lods, dev):
    return [torch.from_numpy(rng.standard_normal((1, fdim, 2 ** l + 1, 2 ** l + 1)).astype(np.float32)).to(dev)
            for l in lods for _ in range(3)]


def _uniform(rng, n, dev, spread=1.0):
    return torch.from_numpy(rng.uniform(-spread, spread, (n, 3)).astype(np.float32)).to(dev)


def _ray_ordered(n_rays, steps, dev, seed=0):
    """samples of the AABB voxel marcher, ray by ray."""
    from shacira_amd import harness
    from shacira_amd.wisp.accelstructs import AxisAlignedBBoxAS
    from shacira_amd.wisp.core import Rays
    o, d = harness.camera_rays(n_rays, torch.Generator().manual_seed(seed), dev)
    torch.manual_seed(seed)
    return AxisAlignedBBoxAS().raymarch(Rays(o, d, 1.0, 5.0), raymarch_type="voxel", num_samples=steps,
                                        level=0).samples.contiguous()


def _ref_lists(planes, L):
    return [[planes[3 * l + p][0].double().cpu().numpy() for p in range(3)] for l in range(L)]


def _check_forward(coords, planes, lods, summed, sub=None):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.triplane import triplane_torch
    got = hip_ops.triplane_forward(coords, lods, planes, summed)
    c = coords if sub is None else coords[sub]
    g = got if sub is None else got[sub]
    cn = c.cpu().numpy()
    ref = tr.forward(cn, _ref_lists(planes, len(lods)), summed, index_dtype=np.float32)
    scale = tr.abs_forward(cn, _ref_lists(planes, len(lods)), summed, index_dtype=np.float32)
    err = np.abs(g.cpu().double().numpy() - ref)
    assert np.all(err <= 4 * len(lods) * EPS * scale + 1e-30), float((err / np.maximum(scale, 1e-30)).max())
    dev_torch = float((got - triplane_torch(coords, planes, len(lods), summed)).abs().max()) if coords.shape[0] else 0.0
    assert dev_torch <= 1e-4, dev_torch
    return dev_torch


@pytest.mark.parametrize("summed", [True, False])
@pytest.mark.parametrize("fdim,lods,n", [(4, [5, 6, 7, 8], 1 << 21), (4, [5, 6, 7, 8], (1 << 16) + 3), (1, [0, 1, 2], 63),
                                         (2, [3, 4], 1), (8, [6, 7], 4099), (4, [5], 0), (3, [2, 5], 999),
                                         (16, [4], 5000)])
def test_forward_against_restatement_and_torch(dev, summed, fdim, lods, n):
    rng = np.random.default_rng(n + fdim)
    planes = _planes(rng, fdim, lods, dev)
    coords = _uniform(rng, n, dev, spread=1.3)
    sub = torch.arange(0, n, max(1, n // 3000), device=dev) if n > 5000 else None
    d = _check_forward(coords, planes, lods, summed, sub)
    print(f"largest deviation from torch's grid_sample composition: {d:.3e}")


@pytest.mark.parametrize("layout", [0, 1])
def test_forward_layouts_agree_bitwise_and_ray_ordered_batch(dev, layout):
    from shacira_amd import _lib, hip_ops
    rng = np.random.default_rng(5)
    lods = [5, 6, 7, 8]
    planes = _planes(rng, 4, lods, dev)
    coords = _ray_ordered(4096, 64, dev)
    _lib.set_option("triplane_layout", layout)
    try:
        _check_forward(coords, planes, lods, True, torch.arange(0, coords.shape[0], 97, device=dev))
        a = hip_ops.triplane_forward(coords, lods, planes, False)
    finally:
        _lib.set_option("triplane_layout", -1)
    assert torch.equal(a, hip_ops.triplane_forward(coords, lods, planes, False))


def test_nonfinite_coordinates_match_torch(dev):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.triplane import triplane_torch
    rng = np.random.default_rng(2)
    planes = _planes(rng, 4, [3, 5], dev)
    vals = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.3, 1.0, -1.0], device=dev)
    coords = torch.cartesian_prod(vals, vals, vals).contiguous()
    for summed in (True, False):
        got = hip_ops.triplane_forward(coords, [3, 5], planes, summed)
        want = triplane_torch(coords, planes, 2, summed)
        assert torch.allclose(got, want, atol=1e-5, equal_nan=True)
    # backward: a non-finite coordinate contributes nothing, and its coordinate gradient is what torch gives
    c = coords.clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in planes]
    go = torch.randn(coords.shape[0], 12, device=dev)
    gw = torch.autograd.grad(triplane_torch(c, p, 2, True), [c, *p], go)
    from shacira_amd.wisp.ops.triplane import triplane_interpolate
    gh = torch.autograd.grad(triplane_interpolate(c, [3, 5], p, True), [c, *p], go)
    for a, b in zip(gh, gw):
        assert torch.allclose(a, b, atol=1e-4, equal_nan=True)


@pytest.mark.parametrize("summed", [True, False])
@pytest.mark.parametrize("fdim,lods,n,order", [(4, [5, 6, 7, 8], 1 << 18, "uniform"), (4, [5, 6, 7, 8], 0, "rays"),
                                               (1, [0, 1], 63, "uniform"), (2, [7], 70000, "uniform"),
                                               (8, [3, 9], 20000, "uniform"), (32, [4, 6], 3000, "uniform"),
                                               (5, [2], 1, "uniform")])
def test_backward_against_restatement(dev, summed, fdim, lods, n, order):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(17 + fdim)
    planes = _planes(rng, fdim, lods, dev)
    coords = _ray_ordered(1024, 256, dev) if order == "rays" else _uniform(rng, n, dev, spread=2.5)
    n = coords.shape[0]
    K = 3 * fdim * (1 if summed else len(lods))
    go = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).to(dev)
    grads, gc = hip_ops.triplane_backward(coords, lods, fdim, go, summed, planes=planes, need_coords=True)
    gref, gcref, gscale = tr.backward(coords.cpu().numpy(), _ref_lists(planes, len(lods)), go.cpu().numpy(), summed,
                                      index_dtype=np.float32)
    for l in range(len(lods)):
        for p in range(3):
            want = gref[l][p]
            err = float(np.abs(grads[3 * l + p][0].cpu().double().numpy() - want).max())
            assert err <= 1e-5 * max(float(np.abs(want).max()), 1e-30), (l, p, err)
    # coordinate gradient: fp32 sums of up to 4 * 3F * L terms per plane, scaled by (S - 1) / 2
    err = np.abs(gc.cpu().double().numpy() - gcref)
    assert np.all(err <= 64 * EPS * gscale + 1e-6), float((err - 64 * EPS * gscale).max())
    # without the coordinate flag the planes are not needed and the plane gradients come out the same (to atomics)
    g2, gc2 = hip_ops.triplane_backward(coords, lods, fdim, go, summed)
    assert gc2 is None
    for a, b in zip(grads, g2):
        assert torch.allclose(a, b, rtol=0, atol=1e-5 * max(float(a.abs().max()), 1e-30))


def test_autograd_surface(dev):
    from shacira_amd.wisp.ops.triplane import triplane_interpolate, triplane_torch
    rng = np.random.default_rng(8)
    lods = [2, 4]
    planes = [t.requires_grad_(True) for t in _planes(rng, 4, lods, dev)]
    coords = _uniform(rng, 5000, dev, 1.2)
    # coordinates that do not require a gradient get none
    out = triplane_interpolate(coords, lods, planes, True)
    gp = torch.autograd.grad(out.square().sum(), planes)
    assert all(g is not None and g.shape == p.shape for g, p in zip(gp, planes))
    # autocast: fp16 coordinates, fp32 planes -> fp32 samples, like torch's own op
    with torch.autocast("cuda", dtype=torch.float16):
        a = triplane_interpolate(coords.half(), lods, planes, True)
        b = triplane_torch(coords.half(), planes, 2, True)
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    assert torch.allclose(a, b, atol=1e-4)
    # create_graph=True gives first-order gradients; a second differentiation raises
    c = coords.clone().requires_grad_(True)
    out = triplane_interpolate(c, lods, planes, False)
    g = torch.autograd.grad(out.square().sum(), [c, planes[0]], create_graph=True)
    want = torch.autograd.grad(triplane_torch(c, planes, 2, False).square().sum(), [c, planes[0]])
    assert torch.allclose(g[0], want[0], atol=1e-3) and torch.allclose(g[1], want[1], atol=1e-3)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g[0].sum(), c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_fallback_dtypes_warn_once_and_agree(dev, dtype):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.triplane import triplane_interpolate, triplane_torch
    rng = np.random.default_rng(9)
    planes = [t.to(dtype) for t in _planes(rng, 2, [3], dev)]
    coords = _uniform(rng, 300, dev).to(dtype)
    hip_ops._warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = triplane_interpolate(coords, [3], planes, True)
        triplane_interpolate(coords, [3], planes, True)
    assert sum("triplane sampling" in str(x.message) for x in w) == 1
    assert a.dtype == dtype and torch.equal(a, triplane_torch(coords, planes, 1, True))


def test_graph_capture_replays_eager(dev):
    from shacira_amd.wisp.ops.triplane import triplane_interpolate
    rng = np.random.default_rng(10)
    lods = [5, 6, 7, 8]
    planes = [t.requires_grad_(True) for t in _planes(rng, 4, lods, dev)]
    coords = _uniform(rng, 1 << 18, dev).requires_grad_(True)
    go = torch.randn(1 << 18, 12, device=dev)

    def step():
        out = triplane_interpolate(coords, lods, planes, True)
        return (out.detach(), *torch.autograd.grad(out, [coords, *planes], go))

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
    for a, b in zip(captured[2:], eager[2:]):
        assert torch.allclose(a, b, rtol=0, atol=1e-5 * float(b.abs().max()))


def test_module_shapes_and_reference_state_dict(dev):
    from shacira_amd.wisp.models.grids import TriplanarGrid
    from shacira_amd.wisp.ops.triplane import triplane_torch
    torch.manual_seed(0)
    sd = {f"features.{i}.{n}": torch.randn(1, 2, 2 ** l + 1, 2 ** l + 1) for i, l in enumerate([3, 4, 5])
          for n in ("fmx", "fmy", "fmz")}
    for ms in ("sum", "cat"):
        g = TriplanarGrid(2, 3, 3, multiscale_type=ms)
        g.load_state_dict(sd)
        g = g.to(dev)
        x3 = torch.rand(7, 5, 3, device=dev) * 2 - 1
        x2 = torch.rand(7, 3, device=dev) * 2 - 1
        for lod_idx in (0, 1, 2):
            K = 6 if ms == "sum" else 6 * (lod_idx + 1)
            assert g.interpolate(x3, lod_idx).shape == (7, 5, K)
            assert g.interpolate(x2, lod_idx).shape == ((7, 6) if ms == "sum" else (7, 1, K))
            planes = [sd[f"features.{i}.{n}"].to(dev) for i in range(lod_idx + 1) for n in ("fmx", "fmy", "fmz")]
            want = triplane_torch(x2, planes, lod_idx + 1, ms == "sum")
            assert torch.allclose(g.interpolate(x2, lod_idx).reshape(want.shape), want, atol=1e-5)
        vol = g.features[0]
        assert vol(x2).shape == (7, 3, 2) and vol(x3).shape == (7, 5, 3, 2)


def _slab(o, d):
    inv = 1.0 / d
    t0, t1 = (-1 - o) * inv, (1 - o) * inv
    tn = torch.minimum(t0, t1).max(dim=1).values
    tf = torch.maximum(t0, t1).min(dim=1).values
    return tn.clamp(min=0), tf


def test_aabb_raytrace_and_voxel_march_match_the_slab_test(dev):
    from shacira_amd import harness
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import TriplanarGrid
    g = TriplanarGrid(2, 2)
    o, d = harness.camera_rays(3000, torch.Generator().manual_seed(4), dev)
    o[:500] *= 0.1                                                # some rays start inside the cube
    d[500:600] = torch.tensor([0.0, 0.0, 1.0], device=dev)        # some miss or graze it
    rays = Rays(o, d, 0.0, 10.0)
    res = g.raytrace(rays, with_exit=True)
    tn, tf = _slab(o.double().cpu(), d.double().cpu())
    hit = tf > tn
    assert torch.equal(res.ridx.long().cpu(), torch.nonzero(hit).flatten())
    assert torch.allclose(res.depth.cpu().double(), torch.stack([tn, tf], 1)[hit], atol=1e-5)
    torch.manual_seed(1)
    m = g.raymarch(rays, raymarch_type="voxel", num_samples=16)
    assert m.samples.shape[0] == 16 * int(hit.sum())
    assert (m.samples.abs() <= 1 + 1e-5).all()
    dep = m.depth_samples.view(-1, 16).cpu().double()
    lo, hi = torch.stack([tn, tf], 1)[hit].unbind(1)
    assert ((dep >= lo[:, None] - 1e-5) & (dep <= hi[:, None] + 1e-5)).all()


def test_nerf_on_a_triplanar_grid_trains(dev):
    from shacira_amd import harness
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import TriplanarGrid
    from shacira_amd.wisp.models.nefs import NeuralRadianceField
    from shacira_amd.wisp.tracers import PackedRFTracer
    torch.manual_seed(0)
    grid = TriplanarGrid(feature_dim=4, base_lod=5, num_lods=4, multiscale_type="sum", feature_std=0.01)
    nef = NeuralRadianceField(grid, view_embedder="positional", view_multires=4, hidden_dim=64, num_layers=1).to(dev)
    with pytest.raises(NotImplementedError):
        nef.prune()
    truth = harness._AnalyticNef(TriplanarGrid(1, 0))
    tracer = PackedRFTracer(raymarch_type="voxel", num_steps=48, bg_color="white")
    gt_tracer = PackedRFTracer(raymarch_type="voxel", num_steps=192, bg_color="white")
    opt = torch.optim.Adam([{"params": grid.parameters(), "lr": 1e-2},
                            {"params": [p for n, p in nef.named_parameters() if not n.startswith("grid.")], "lr": 1e-3}])
    gen = torch.Generator().manual_seed(1)
    losses = []
    for _ in range(300):
        o, d = harness.camera_rays(2048, gen, dev)
        rays = Rays(o, d, dist_min=1.2, dist_max=4.8)
        with torch.no_grad():
            target = gt_tracer(truth, rays).rgb
        loss = (tracer(nef, rays).rgb - target).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    first, last = np.mean(losses[:20]), np.mean(losses[-20:])
    print(f"NeRF on TriplanarGrid: L1 {first:.4f} -> {last:.4f}")
    assert last < 0.6 * first, (first, last)
