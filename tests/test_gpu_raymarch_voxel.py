"""The fused seeded voxel march (render.hip: raymarch_voxel_nuggets_kernel / raymarch_voxel_expand_kernel) against its contract
(include/shacira_hip.h, shacira_raymarch_voxel_emit): the nuggets are those of raytrace_dense, the rows those of
tests/raymarch_voxel_ref.py (restated jitter + oracle.render.raymarch_voxel) bit for bit; then the capped form, the independence
of a row from the rest of the batch, and the way up through OctreeAS, PackedRFTracer and the graphed fitter."""
import numpy as np
import pytest
import torch

import raymarch_voxel_ref as V
import test_gpu_render as T
from oracle import render as orr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _family(kind, n, rng):
    """float32 (origins, dirs) [n, 3] of one family of rays."""
    if kind == "through":                                         # from the radius-3 sphere towards the cube
        return T._rays(rng, n)
    if kind == "miss":                                            # from the sphere, outwards
        o = 3.0 * _unit(rng.standard_normal((n, 3)))
        d = _unit(o + 0.1 * rng.standard_normal((n, 3)))
    elif kind == "inside":                                        # start inside the volume: the entry is clipped to 0
        o = rng.uniform(-0.9, 0.9, (n, 3))
        d = _unit(rng.standard_normal((n, 3)))
    elif kind == "axis":                                          # two zero components, then one
        o = rng.uniform(-0.9, 0.9, (n, 3))
        d = np.zeros((n, 3))
        a = np.arange(n) % 3
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        o[np.arange(n), a] = -3.0 * sign
        d[np.arange(n), a] = sign
        half = np.arange(n) >= n // 2                             # ... the second half: one zero component
        b = (a + 1) % 3
        d[half, b[half]] = 0.25
        d = _unit(d)
    elif kind == "graze":                                         # along a face of the cube: on it, just inside, just outside
        o = rng.uniform(-0.9, 0.9, (n, 3))
        d = np.zeros((n, 3))
        o[:, 0], d[:, 0] = -3.0, 1.0
        o[:, 2] = np.choose(np.arange(n) % 4, [1.0, 1.0 - 2.0 ** -24, -1.0, 1.0 + 2.0 ** -23])
    else:
        raise ValueError(kind)
    return torch.from_numpy(o.astype(np.float32)), torch.from_numpy(d.astype(np.float32))


def _rays(kind, n, rng):
    if kind != "mixed":
        return _family(kind, n, rng)
    kinds = ("through", "miss", "inside", "axis", "graze")
    parts = [_family(k, n, rng) for k in kinds]
    pick = torch.from_numpy(rng.integers(0, len(kinds), n))
    o = torch.stack([p[0] for p in parts])[pick, torch.arange(n)]
    d = torch.stack([p[1] for p in parts])[pick, torch.arange(n)]
    return o, d


def _occupancy(kind, level, rng):
    G = 1 << level
    if kind == "all":
        return torch.ones((G, G, G), dtype=torch.bool)
    if kind == "none":
        return torch.zeros((G, G, G), dtype=torch.bool)
    return torch.from_numpy(rng.random((G, G, G)) < 0.3)


def _restated(dev, o, d, occ, level, ns, seed, step):
    """The rows of the contract on the CPU, from the nuggets raytrace_dense writes on the device."""
    from shacira_amd import render
    ridx, _, depth = [t.cpu() for t in render.raytrace_dense(o.to(dev), d.to(dev), occ.to(dev), level)]
    return V.march(o, d, ridx, depth, ns, seed, step), ridx.shape[0]


def _assert_rows_equal(got, want, rows=None):
    names = ("ridx", "samples", "depth", "deltas", "boundary")
    for name, g, w in zip(names, got, want):
        g, w = (g.cpu(), w.cpu()) if rows is None else (g.cpu()[:rows], w.cpu()[:rows])
        assert g.dtype == w.dtype and torch.equal(g, w), name


# level, ns, N, occupancy, rays, hit and missed rays both present
CASES = [(0, 130, 257, "all", "mixed", True), (0, 5, 64, "all", "mixed", True), (0, 1, 1, "all", "through", False),
         (1, 3, 257, "random", "mixed", True), (1, 64, 64, "all", "mixed", True), (1, 1, 257, "random", "axis", True),
         (5, 5, 257, "random", "mixed", True), (5, 1, 64, "random", "mixed", True), (5, 3, 1, "all", "through", False),
         (5, 130, 64, "random", "inside", False), (5, 3, 257, "all", "graze", True), (5, 64, 257, "none", "mixed", None),
         (5, 5, 64, "all", "miss", None)]


@pytest.mark.parametrize("level,ns,N,occ_kind,ray_kind,both", CASES)
def test_rows_equal_the_restatement(dev, level, ns, N, occ_kind, ray_kind, both):
    from shacira_amd import render
    rng = np.random.default_rng(1000 * level + ns + N)
    o, d = _rays(ray_kind, N, rng)
    occ = _occupancy(occ_kind, level, rng)
    seed, step = 0xC0FFEE0000000000 + ns, 3 + level
    want, K = _restated(dev, o, d, occ, level, ns, seed, step)
    got = [t.cpu() for t in render.raymarch_voxel(o.to(dev), d.to(dev), occ.to(dev), level, ns, seed, step)]
    ridx, samples, depth, deltas, boundary, offsets = got
    S = K * ns
    assert ridx.shape == (S,) and samples.shape == (S, 3) and depth.shape == (S, 1) and deltas.shape == (S, 1)
    assert ridx.dtype == torch.int64 and boundary.dtype == torch.bool and offsets.dtype == torch.int64
    if both is None:                                              # nothing occupied or every ray misses: every offset is 0
        assert K == 0 and not offsets.any() and offsets.shape == (N + 1,)
    else:
        hit = offsets[1:] > offsets[:-1]
        assert K > 0 and bool(hit.any()) and (not both or not bool(hit.all())), "the case compares nothing"
    assert torch.equal(ridx, want[0]) and torch.equal(offsets, want[5])
    assert torch.equal(depth, want[2]), float((depth - want[2]).abs().max())
    assert torch.equal(deltas, want[3]), float((deltas - want[3]).abs().max())
    assert torch.equal(boundary, want[4])
    exact = o.double()[ridx] + d.double()[ridx] * depth.double()
    err = float((samples.double() - exact).abs().max()) if S else 0.0
    print(f"level {level} ns {ns} N {N} {occ_kind}/{ray_kind}: K {K}, samples off fp64 by {err:.3e}")
    assert err <= 2.0 ** -23                                      # one rounding of a value in or at the face of [-1, 1]^3
    if S:
        assert bool((deltas >= 0).all()) and int(boundary.sum()) == int((offsets[1:] > offsets[:-1]).sum())


@pytest.fixture(scope="module")
def scene(dev):
    """One batch shared by the tests below: rays, occupancy, and its seeded rows on the device."""
    from shacira_amd import render
    rng = np.random.default_rng(77)
    N, level, ns, seed, step = 257, 5, 5, 1234567, 9
    o, d = _rays("mixed", N, rng)
    occ = _occupancy("random", level, rng)
    args = (o.to(dev), d.to(dev), occ.to(dev), level, ns, seed)
    rows = render.raymarch_voxel(*args, step)
    assert rows[0].shape[0] > 1000
    return dict(args=args, step=step, rows=rows, N=N, ns=ns)


def test_a_row_depends_on_its_ray_only(dev, scene):
    from shacira_amd import render
    o, d, occ, level, ns, seed = scene["args"]
    rows, step, N = scene["rows"], scene["step"], scene["N"]
    again = render.raymarch_voxel(o, d, occ, level, ns, seed, step)
    _assert_rows_equal(again, rows)
    assert torch.equal(again[5], rows[5])
    # every other ray replaced by one that misses: the kept rays stay at their index and keep their rows
    o2, d2 = o.clone(), d.clone()
    o2[1::2] = torch.tensor([5.0, 5.0, 5.0], device=dev)
    d2[1::2] = torch.tensor([0.0, 1.0, 0.0], device=dev)
    sub = render.raymarch_voxel(o2, d2, occ, level, ns, seed, step)
    keep = rows[0] % 2 == 0
    assert 0 < int(keep.sum()) < keep.shape[0]
    for a, b in zip(sub[1:4], rows[1:4]):
        assert torch.equal(a, b[keep])
    assert torch.equal(sub[0], rows[0][keep]) and torch.equal(sub[4], rows[4][keep])
    # ... and a prefix of the batch
    head = render.raymarch_voxel(o[:100], d[:100], occ, level, ns, seed, step)
    _assert_rows_equal(head, rows, rows=head[0].shape[0])
    assert torch.equal(head[5], rows[5][:101]) and head[0].shape[0] == int(rows[5][100])
    # another seed or step: the same nuggets, other depths
    for other in (render.raymarch_voxel(o, d, occ, level, ns, seed + 1, step),
                  render.raymarch_voxel(o, d, occ, level, ns, seed, step + 1)):
        assert torch.equal(other[0], rows[0]) and torch.equal(other[4], rows[4])
        assert float((other[2] != rows[2]).float().mean()) > 0.99
    # the step on the device, alone and added to a host part
    on_dev = render.raymarch_voxel(o, d, occ, level, ns, seed, torch.tensor([step], device=dev))
    _assert_rows_equal(on_dev, rows)
    with pytest.raises(RuntimeError):
        render.raymarch_voxel(o, d, occ, level, ns, seed, torch.tensor([step], device=dev, dtype=torch.int32))


def test_capped_form(dev, scene):
    from shacira_amd import render
    o, d, occ, level, ns, seed = scene["args"]
    rows, step = scene["rows"], scene["step"]
    S = rows[0].shape[0]
    cut = S // 2 // ns * ns + 2                                   # in the middle of a nugget
    assert cut % ns != 0
    for cap in (S + 333, S, cut, 1):
        ridx, samples, depth, deltas, boundary, offsets, total = render.raymarch_voxel(o, d, occ, level, ns, seed, step,
                                                                                       capacity=cap)
        assert int(total) == S and ridx.shape[0] == cap and samples.shape == (cap, 3)
        k = min(S, cap)
        _assert_rows_equal((ridx, samples, depth, deltas, boundary), rows, rows=k)
        assert torch.equal(offsets, rows[5].clamp(max=cap)) and int(offsets[-1]) == k
        if cap > S:                                               # the rows behind the last survivor are the padding
            assert not ridx[S:].any() and not depth[S:].any() and not deltas[S:].any() and not boundary[S:].any()
            assert torch.equal(samples[S:], render._padding_positions(cap, dev)[S:])
    # nothing is written at or beyond the capacity: guard rows behind the buffers the library sees stay as they were
    from shacira_amd import _lib
    from shacira_amd.hip_ops import _ptr, _stream
    guard = 64
    counts = torch.bincount(rows[0], minlength=scene["N"]) // ns
    nuggets = torch.zeros(scene["N"] + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=nuggets[1:])
    ridx = torch.full((cut + guard,), -7, dtype=torch.int64, device=dev)
    samples = torch.full((cut + guard, 3), -7.0, device=dev)
    depth, deltas = torch.full((cut + guard,), -7.0, device=dev), torch.full((cut + guard,), -7.0, device=dev)
    boundary = torch.full((cut + guard,), 7, dtype=torch.uint8, device=dev)
    L = _lib.lib()
    ws_bytes = int(L.shacira_raymarch_voxel_workspace_bytes(cut, ns))
    ws = torch.zeros(ws_bytes + guard, dtype=torch.uint8, device=dev)
    occ8 = occ.to(torch.uint8).contiguous()
    _lib.check(L.shacira_raymarch_voxel_emit(scene["N"], ns, _ptr(o), _ptr(d), _ptr(occ8), level, _ptr(nuggets), seed, step, None,
                                             cut, _ptr(ws), ws_bytes, _ptr(ridx), _ptr(samples), _ptr(depth), _ptr(deltas),
                                             _ptr(boundary), _stream(o)))
    assert torch.equal(ridx[:cut], rows[0][:cut]) and torch.equal(depth[:cut], rows[2][:cut, 0])
    assert bool((ridx[cut:] == -7).all()) and bool((samples[cut:] == -7).all()) and bool((depth[cut:] == -7).all())
    assert bool((deltas[cut:] == -7).all()) and bool((boundary[cut:] == 7).all()) and not ws[ws_bytes:].any()


def _closed_form_setup(dev):
    """The grid, field and rays of test_gpu_render.test_tracer_composites_like_the_reference_formula."""
    from shacira_amd import harness
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import HashGrid
    grid = HashGrid.from_geometric(feature_dim=2, num_lods=2, multiscale_type="cat", resolution_dim=3, feature_std=0.0,
                                   codebook_bitwidth=4, min_grid_res=2, max_grid_res=4, blas_level=4)
    occ = torch.from_numpy(np.random.default_rng(3).random((16, 16, 16)) < 0.6)
    grid.blas = grid.blas.__class__.from_quantized_points(torch.nonzero(occ), 4)
    o, d = harness.camera_rays(300, torch.Generator().manual_seed(1), dev)
    return grid, occ, harness._AnalyticNef(grid), Rays(o, d, dist_min=1.0, dist_max=5.0)


def test_seeded_tracer_composites_like_the_reference_formula(dev):
    from shacira_amd import harness
    from shacira_amd.wisp.tracers import PackedRFTracer
    grid, occ, nef, rays = _closed_form_setup(dev)
    ns, seed = 3, 42
    tracer = PackedRFTracer(raymarch_type="voxel", num_steps=ns, bg_color="white", seed=seed)
    for call in range(2):                                         # the tracer's host counter: step 0, then step 1
        marched = grid.raymarch(rays, raymarch_type="voxel", num_samples=ns, level=grid.active_lods[-1], seed=seed, step=call)
        assert marched.ray_offsets is not None and marched.ray_offsets.shape == (301,)
        rb = tracer(nef, rays, channels=("rgb", "depth"))
        assert tracer.step == call + 1
        ridx, boundary = marched.ridx.cpu(), marched.boundary.cpu()
        assert ridx.shape[0] > 0 and orr.query_dense(occ, marched.samples.cpu(), 4).all()
        density, color = harness.analytic_scene(marched.samples.cpu())
        tau = density * marched.deltas.cpu()
        ray_colors, w = orr.exponential_integration(color.double(), tau.double(), boundary)
        alpha = orr.sum_reduce(w, boundary)
        depth = orr.sum_reduce(marched.depth_samples.cpu().double() * w, boundary)
        hit_rays = ridx[boundary]
        assert hit_rays.shape[0] > 0
        want_rgb = torch.ones(300, 3, dtype=torch.float64)
        want_rgb[hit_rays] = (1.0 - alpha) + ray_colors
        np.testing.assert_allclose(rb.rgb.cpu().numpy(), want_rgb.numpy(), rtol=1e-5, atol=2e-6)
        want_alpha = torch.zeros(300, 1, dtype=torch.float64)
        want_alpha[hit_rays] = alpha
        np.testing.assert_allclose(rb.alpha.cpu().numpy(), want_alpha.numpy(), rtol=1e-5, atol=2e-6)
        want_depth = torch.zeros(300, 1, dtype=torch.float64)
        want_depth[hit_rays] = depth
        np.testing.assert_allclose(rb.depth.cpu().numpy(), want_depth.numpy(), rtol=1e-5, atol=1e-5)
        sure = (want_alpha[:, 0] > 1e-6) | (want_alpha[:, 0] == 0)    # fp32 rounds 1 - exp(-tau) to 0 below ~6e-8
        assert torch.equal(rb.hit.cpu()[sure], (want_alpha[:, 0] > 0)[sure])


def test_without_a_seed_the_march_is_the_composed_one(dev):
    from shacira_amd.wisp.accelstructs import AxisAlignedBBoxAS
    grid, _, _, rays = _closed_form_setup(dev)
    for blas, level, ns in ((grid.blas, 4, 3), (grid.blas, 2, 5), (AxisAlignedBBoxAS(), 0, 7)):
        torch.manual_seed(5)
        got = blas.raymarch(rays, "voxel", ns, level=level)
        torch.manual_seed(5)
        want = blas._raymarch_voxel(rays, ns, level)
        assert got.ray_offsets is None and got.ridx.shape[0] > 0
        for a, b in zip(got[:5], want[:5]):
            assert a.dtype == b.dtype and torch.equal(a, b)
        seeded = blas.raymarch(rays, "voxel", ns, level=level, seed=1)       # the same nuggets, its own jitter
        assert torch.equal(seeded.ridx, got.ridx) and torch.equal(seeded.boundary, got.boundary)
        assert not torch.equal(seeded.depth_samples, got.depth_samples)


def test_gradient_equals_the_composed_path_on_the_same_samples(dev):
    from shacira_amd import harness
    from shacira_amd.wisp.accelstructs import ASRaymarchResults
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import HashGrid
    from shacira_amd.wisp.models.nefs import NeuralRadianceField
    from shacira_amd.wisp.tracers import PackedRFTracer
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(feature_dim=2, num_lods=4, multiscale_type="cat", resolution_dim=3, feature_std=0.1,
                                   codebook_bitwidth=10, min_grid_res=4, max_grid_res=32, blas_level=3)
    occ = torch.from_numpy(np.random.default_rng(8).random((8, 8, 8)) < 0.5)
    grid.blas = grid.blas.__class__.from_quantized_points(torch.nonzero(occ), 3)
    nef = NeuralRadianceField(grid, view_embedder="positional", view_multires=4, hidden_dim=64, num_layers=1).to(dev)
    o, d = harness.camera_rays(200, torch.Generator().manual_seed(2), dev)
    rays = Rays(o, d, dist_min=1.0, dist_max=5.0)
    target = torch.rand(200, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    ns, seed = 3, 11

    def grads(tracer):
        nef.zero_grad(set_to_none=True)
        rb = tracer(nef, rays)
        ((rb.rgb - target) ** 2).sum().backward()
        return rb.rgb.detach().clone(), grid.codebook.grad.detach().clone()

    rgb_s, g_s = grads(PackedRFTracer(raymarch_type="voxel", num_steps=ns, seed=seed))
    assert torch.isfinite(g_s).all() and float(g_s.abs().max()) > 0
    real = grid.raymarch

    def composed(rays, level=None, num_samples=64, raymarch_type="voxel"):
        m = real(rays, raymarch_type=raymarch_type, num_samples=num_samples, level=level, seed=seed, step=0)
        assert m.ray_offsets is not None
        return ASRaymarchResults(ridx=m.ridx, samples=m.samples, depth_samples=m.depth_samples, deltas=m.deltas,
                                 boundary=m.boundary)

    grid.raymarch = composed
    rgb_c, g_c = grads(PackedRFTracer(raymarch_type="voxel", num_steps=ns))
    print(f"gradient: max {float(g_c.abs().max()):.3e}, seeded - composed {float((g_s - g_c).abs().max()):.3e}; "
          f"rgb {float((rgb_s - rgb_c).abs().max()):.3e}")
    np.testing.assert_allclose(rgb_s.cpu().numpy(), rgb_c.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g_s.cpu().numpy(), g_c.cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_graphed_voxel_fit(dev, monkeypatch):
    """fit_nerf(graphed=True, raymarch_type='voxel') at the configuration of test_gpu_render's graphed 'ray' fit (the voxel
    march samples per crossed cell: 4 of them give about the sample count of 96 per ray): it captures, drops no sample, ends
    where the eager seeded fit ends, and two replays on the same pool batch draw different jitter."""
    from shacira_amd import harness
    fitters = []

    class Watched(harness.GraphedNerfFitter):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            fitters.append(self)
            self.captured = {}
            march = self.blas.raymarch

            def watched(*a, **k):
                m = march(*a, **k)
                if torch.cuda.is_current_stream_capturing():
                    self.captured[self.capacity] = m            # the buffers the graph of this capacity writes
                return m

            self.blas.raymarch = watched

    monkeypatch.setattr(harness, "GraphedNerfFitter", Watched)
    kw = dict(steps=350, rays=2048, num_steps=4, codebook_bitwidth=16, max_grid_res=512, prune_every=100, val_rays=4096,
              ray_pool=32, raymarch_type="voxel")
    eager = harness.fit_nerf(dev, **kw)
    graphed = harness.fit_nerf(dev, graphed=True, **kw)
    print("eager", eager, "\ngraphed", graphed)
    assert graphed["overflow_steps"] == 0, graphed
    assert 1 <= graphed["graph_captures"] <= 4, graphed
    assert graphed["psnr"] > 17.5 and abs(graphed["psnr"] - eager["psnr"]) < 1.5, (eager, graphed)
    assert 0 < graphed["occupied_cells"] < graphed["total_cells"], graphed
    (fitter,) = fitters
    m = fitter.captured[fitter.capacity]
    assert m.ray_offsets is not None and m.samples.shape[0] == fitter.capacity
    seen = []
    for _ in range(2):
        fitter.index.zero_()                                      # the same pool batch
        before = int(fitter.march_step)
        fitter.graph.replay()
        torch.cuda.synchronize()
        assert int(fitter.march_step) == before + 1
        seen.append((m.ridx.clone(), m.depth_samples.clone(), m.ray_offsets.clone()))
    live = int(seen[0][2][-1])
    assert live > 0 and torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][2], seen[1][2])
    assert float((seen[0][1][:live] != seen[1][1][:live]).float().mean()) > 0.99
