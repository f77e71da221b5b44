"""The CPU restatement of the volume-integration / sample-generation steps (oracle/render.py) against naive per-ray
loops written from the formulas, and the host-side occupancy mirror. No golden vectors exist for these steps in the
reference (kaolin is not vendored): the restatement is "parity unpinned" and anchored on the published formula."""
import numpy as np
import torch

from oracle import render as orr
from shacira_amd.wisp.accelstructs import OctreeAS, _morton_points


def _boundary(lens):
    b = np.zeros(sum(lens), dtype=bool)
    b[np.concatenate([[0], np.cumsum(lens)[:-1]])] = True
    return torch.from_numpy(b)


def test_exponential_integration_equals_per_ray_loop():
    rng = np.random.default_rng(0)
    lens = [1, 7, 64, 3, 130]
    boundary = _boundary(lens)
    S = sum(lens)
    feats = torch.from_numpy(rng.random((S, 3)))
    tau = torch.from_numpy(rng.random((S, 1)) * 1.5)
    ray, w = orr.exponential_integration(feats, tau, boundary)
    i = 0
    for r, n in enumerate(lens):
        T, acc = 1.0, np.zeros(3)
        for k in range(n):
            a = 1.0 - np.exp(-tau[i + k, 0].item())
            wk = T * a
            assert abs(w[i + k, 0].item() - wk) < 1e-12
            acc += wk * feats[i + k].numpy()
            T *= np.exp(-tau[i + k, 0].item())
        np.testing.assert_allclose(ray[r].numpy(), acc, rtol=1e-12)
        i += n
    np.testing.assert_allclose(orr.sum_reduce(feats, boundary).numpy(),
                               np.stack([feats[s:s + n].sum(0).numpy() for s, n in zip(np.cumsum([0] + lens[:-1]), lens)]))
    assert torch.equal(orr.mark_pack_boundaries(torch.tensor([4, 4, 7, 9, 9, 9])),
                       torch.tensor([True, False, True, True, False, False]))


def test_raymarch_ray_keeps_exactly_the_occupied_samples():
    rng = np.random.default_rng(1)
    level, ns, N = 3, 12, 40
    G = 1 << level
    o = torch.from_numpy(rng.uniform(-0.9, 0.9, (N, 3)).astype(np.float32))
    d = torch.from_numpy(rng.standard_normal((N, 3)).astype(np.float32))
    d = d / d.norm(dim=1, keepdim=True)
    occ = torch.from_numpy(rng.random((G, G, G)) < 0.5)
    jit = torch.from_numpy(rng.random((N, ns)).astype(np.float32))
    ridx, samples, depth, deltas, boundary = orr.raymarch_ray(o, d, 0.0, 0.8, occ, level, ns, jit)
    assert orr.query_dense(occ, samples, level).all()
    np.testing.assert_allclose(samples.numpy(), (o[ridx] + d[ridx] * depth).numpy(), rtol=1e-6, atol=1e-6)
    assert (deltas > 0).all() and (ridx[1:] >= ridx[:-1]).all() and boundary.sum() == ridx.unique().numel()
    # the first sample of a ray measures its delta from dist_min, the others from the previous (kept or not) sample
    all_depth = (torch.linspace(0, 1.0, ns)[None] + jit / ns) * 0.8
    first = torch.isclose(depth[:, 0], all_depth[ridx, 0])
    np.testing.assert_allclose(deltas[first, 0].numpy(), depth[first, 0].numpy(), rtol=1e-6)


def test_raytrace_and_voxel_sampling_are_consistent():
    rng = np.random.default_rng(2)
    level, N, ns = 3, 30, 4
    G = 1 << level
    o = torch.from_numpy(rng.standard_normal((N, 3)).astype(np.float32))
    o = 3.0 * o / o.norm(dim=1, keepdim=True)
    d = -o / o.norm(dim=1, keepdim=True) + torch.from_numpy(rng.normal(0, 0.1, (N, 3)).astype(np.float32))
    d = d / d.norm(dim=1, keepdim=True)
    occ = torch.from_numpy(rng.random((G, G, G)) < 0.5)
    ridx, cells, depth = orr.raytrace_dense(o, d, occ, level)
    assert (depth[:, 1] > depth[:, 0]).all() and occ[cells[:, 0], cells[:, 1], cells[:, 2]].all()
    mid = o[ridx] + d[ridx] * depth.mean(1, keepdim=True)
    assert torch.equal(orr.quantize_points(mid, level), cells)          # interval midpoints lie in the reported cell
    for r in ridx.unique():                                              # per ray: sorted, non-overlapping intervals
        dr = depth[ridx == r]
        assert (dr[1:, 0] >= dr[:-1, 1] - 1e-5).all()
    jit = torch.from_numpy(rng.random((ridx.shape[0], ns)).astype(np.float32))
    rs, samples, ds, deltas, boundary = orr.raymarch_voxel(o, d, ridx, depth, ns, jit)
    assert samples.shape[0] == ridx.shape[0] * ns and boundary.sum() == ridx.unique().numel()
    long_enough = (depth[:, 1] - depth[:, 0] > 1e-3).repeat_interleave(ns)
    assert torch.equal(orr.quantize_points(samples, level)[long_enough], cells.repeat_interleave(ns, 0)[long_enough])
    np.testing.assert_allclose(deltas.reshape(-1, ns).sum(1).numpy(), (ds.reshape(-1, ns)[:, -1] - depth[:, 0]).numpy(),
                               rtol=1e-4, atol=1e-6)


def test_occupancy_mirror_query_and_pruned_set():
    level = 3
    dense = OctreeAS.make_dense(level)
    assert dense.points.shape == (512, 3) and torch.equal(dense.points, _morton_points(level))
    pts = torch.tensor([[-1.0, -1.0, -1.0], [0.99, 0.99, 0.99], [0.0, 0.0, 0.0], [5.0, -5.0, 0.1]])
    pidx = dense.query(pts).pidx
    assert pidx[0] == 0 and pidx[1] == 511 and pidx[2] >= 0 and pidx[3] == -1   # a point outside the cube has no cell
    assert torch.equal(dense.points[pidx[2]].long(), torch.tensor([4, 4, 4]))
    kept = torch.tensor([[4, 4, 4], [0, 0, 0], [7, 0, 3]])
    pruned = OctreeAS.from_quantized_points(kept, level)
    assert pruned.points.shape == (3, 3) and pruned.occupancy_grid.sum() == 3
    q = pruned.query(pts).pidx
    assert q[0] == 0 and q[1] == -1 and q[2] >= 0
    # points come back in Morton order
    codes = [int(c) for c in (pruned.points.long() * torch.tensor([1, 1, 1])).sum(1)]
    assert torch.equal(pruned.points[0].long(), torch.tensor([0, 0, 0])) and len(codes) == 3


def test_points_outside_the_cube_have_no_cell():
    """kaolin's float query (spc `identify`: "check if in bounds" -> -1): a point outside [-1, 1)^3 belongs to no cell,
    whatever the border cells hold. Known answers at level 2 (4 cells per axis, all occupied)."""
    level = 2
    occ = torch.ones(4, 4, 4, dtype=torch.bool)
    pts = torch.tensor([[0.0, 0.0, 0.0], [-1.0, -1.0, -1.0], [0.999, 0.999, 0.999],     # inside (incl. the -1 faces)
                        [1.0, 0.0, 0.0], [0.0, 1.0001, 0.0], [0.0, 0.0, -1.0001],       # on the +1 face / outside
                        [2.5, 0.0, 0.0], [float("nan"), 0.0, 0.0]])
    assert orr.query_dense(occ, pts, level).tolist() == [True, True, True, False, False, False, False, False]


# ------------------------------------------------------------------------------------------------------------------------------
# Closed-form known answers for the kaolin half. kaolin 0.13.0 is not vendored: these pin the restatement to
# the PUBLISHED formula (kaolin/render/spc/raytrace.py: alpha = 1 - exp(-tau); T = exp(-exclusive_cumsum(tau)); w = T * alpha;
# out = sum_reduce(w * feats)) and to analytic results, not to kaolin's output -- "parity unpinned (dependency absent)".
def test_parity_unpinned_dependency_absent__constant_medium_has_analytic_transmittance():
    """Constant density sigma and constant colour c over n equal steps of length d: tau = sigma d per sample, so
    w_k = exp(-k sigma d) (1 - exp(-sigma d)), the weights sum to 1 - exp(-n sigma d) (a geometric series) and the ray colour
    is c (1 - exp(-sigma L)), L = n d -- the closed form of the volume-rendering integral for a homogeneous medium."""
    for n, sigma, d in ((1, 0.7, 0.3), (16, 2.0, 0.05), (200, 0.3, 0.01), (64, 40.0, 0.02)):
        colour = torch.tensor([0.2, 0.5, 0.9], dtype=torch.float64)
        tau = torch.full((n, 1), sigma * d, dtype=torch.float64)
        feats = colour[None].repeat(n, 1)
        ray, w = orr.exponential_integration(feats, tau, _boundary([n]))
        k = np.arange(n)
        np.testing.assert_allclose(w[:, 0].numpy(), np.exp(-k * sigma * d) * (1 - np.exp(-sigma * d)), rtol=1e-12)
        np.testing.assert_allclose(w.sum().item(), 1 - np.exp(-n * sigma * d), rtol=1e-12)
        np.testing.assert_allclose(ray[0].numpy(), colour.numpy() * (1 - np.exp(-sigma * n * d)), rtol=1e-12)


def test_parity_unpinned_dependency_absent__opaque_and_empty_samples():
    """tau = 0 contributes nothing and hides nothing; a sample with tau -> infinity takes all the remaining transmittance and
    everything behind it gets weight 0; packs are independent (the second ray does not see the first ray's wall)."""
    tau = torch.tensor([[0.0], [0.5], [1e9], [0.5], [0.0], [0.25]], dtype=torch.float64)
    feats = torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0], [6.0]], dtype=torch.float64)
    ray, w = orr.exponential_integration(feats, tau, _boundary([4, 2]))
    a = 1 - np.exp(-0.5)
    np.testing.assert_allclose(w[:, 0].numpy(), [0.0, a, np.exp(-0.5), 0.0, 0.0, 1 - np.exp(-0.25)], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(ray[:, 0].numpy(), [2.0 * a + 3.0 * np.exp(-0.5), 6.0 * (1 - np.exp(-0.25))], rtol=1e-12)
    # inclusive form (exclusive=False): the sample's own tau already attenuates it
    _, wi = orr.exponential_integration(feats, tau, _boundary([4, 2]), exclusive=False)
    np.testing.assert_allclose(wi[1, 0].item(), np.exp(-0.5) * a, rtol=1e-12)


def test_parity_unpinned_dependency_absent__ray_cell_slab_cases_by_hand():
    """Ray / cell intersections of a level-1 grid (2 x 2 x 2 cells of side 1 on [-1, 1]^3), worked by hand with the slab
    method: entry = max over axes of the near plane's t, exit = min over axes of the far plane's t."""
    occ = torch.zeros(2, 2, 2, dtype=torch.bool)
    occ[0, 0, 0] = True            # cell [-1, 0]^3
    occ[1, 0, 0] = True            # cell [0, 1] x [-1, 0]^2
    occ[1, 1, 1] = True            # cell [0, 1]^3
    o = torch.tensor([[-2.0, -0.5, -0.5],      # along +x through the two lower cells: [1, 2] then [2, 3]
                      [-2.0, 0.5, 0.5],        # along +x at y = z = 0.5: only cell (1, 1, 1): [2, 3]
                      [-0.5, -0.5, -0.5],      # starts INSIDE cell (0, 0, 0): entry clipped to 0, exit 0.5; then [0.5, 1.5]
                      [-2.0, -2.0, -2.0],      # the main diagonal, direction (1, 1, 1) / sqrt 3: cell 0 [sqrt 3, 2 sqrt 3], cell 7 [2 sqrt 3, 3 sqrt 3]
                      [-2.0, 1.5, 0.0]])       # misses the cube
    d = torch.tensor([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [3 ** -0.5] * 3, [1.0, 0, 0]])
    ridx, cell, depth = orr.raytrace_dense(o, d, occ, 1)
    got = {}
    for r, c, t in zip(ridx.tolist(), cell.tolist(), depth.tolist()):
        got.setdefault(r, []).append((tuple(c), t))
    r3 = 3 ** 0.5
    want = {0: [((0, 0, 0), [1.0, 2.0]), ((1, 0, 0), [2.0, 3.0])],
            1: [((1, 1, 1), [2.0, 3.0])],
            2: [((0, 0, 0), [0.0, 0.5]), ((1, 0, 0), [0.5, 1.5])],
            3: [((0, 0, 0), [r3, 2 * r3]), ((1, 1, 1), [2 * r3, 3 * r3])]}
    assert sorted(got) == sorted(want)
    for r in want:
        assert [c for c, _ in got[r]] == [c for c, _ in want[r]], r
        np.testing.assert_allclose([t for _, t in got[r]], [t for _, t in want[r]], rtol=1e-6, atol=1e-6)


def test_parity_unpinned_dependency_absent__depth_interval_sampling_by_hand():
    """sampling.py:49-55 on one interval [2, 4] with 4 samples and jitter 0.5: depths 2 + 2 (k + 0.5) / 4 = 2.25, 2.75, 3.25,
    3.75; the deltas start from the interval's entry: 0.25, then 0.5 each (octree_as.py:212-216)."""
    depth = torch.tensor([[2.0, 4.0]])
    z = orr.sample_from_depth_intervals(depth, 4, torch.full((1, 4), 0.5))
    np.testing.assert_allclose(z[0].numpy(), [2.25, 2.75, 3.25, 3.75], rtol=1e-7)
    o, d = torch.zeros(1, 3), torch.tensor([[0.0, 0.0, 1.0]])
    ridx_s, samples, ds, deltas, boundary = orr.raymarch_voxel(o, d, torch.tensor([0]), depth, 4, torch.full((1, 4), 0.5))
    np.testing.assert_allclose(deltas[:, 0].numpy(), [0.25, 0.5, 0.5, 0.5], rtol=1e-6)
    np.testing.assert_allclose(samples[:, 2].numpy(), [2.25, 2.75, 3.25, 3.75], rtol=1e-6)
    assert boundary.tolist() == [True, False, False, False] and ridx_s.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------------------
# Per-pack offsets (empty packs, rows no pack covers) and the fp32 restatement of the integration kernels (tests/render_ref.py)
def test_packed_offsets_form_equals_the_boundary_flag_form():
    """`exponential_integration_packed` / `sum_reduce_packed` take the marcher's per-ray offsets. On packs without empties they
    equal the boundary-flag form, values and autograd gradients; an empty pack adds a zero row and changes nothing else."""
    rng = np.random.default_rng(4)
    lens = [1, 7, 64, 3, 130, 65]
    boundary, S = _boundary(lens), sum(lens)
    ps = np.concatenate([[0], np.cumsum(lens)])
    feats = torch.from_numpy(rng.random((S, 5)))
    tau = torch.from_numpy(rng.random((S, 1)) ** 3 * 2.0)
    g_ray, g_w = torch.from_numpy(rng.standard_normal((len(lens), 5))), torch.from_numpy(rng.standard_normal((S, 1)))

    def run(fn, *where):
        f, t = feats.clone().requires_grad_(), tau.clone().requires_grad_()
        ray, w = fn(f, t, *where)
        return ray, w, f, t

    ray_a, w_a, f_a, t_a = run(orr.exponential_integration, boundary)
    ray_b, w_b, f_b, t_b = run(orr.exponential_integration_packed, ps)
    ((ray_a * g_ray).sum() + (w_a * g_w).sum()).backward()
    ((ray_b * g_ray).sum() + (w_b * g_w).sum()).backward()
    np.testing.assert_allclose(ray_b.detach().numpy(), ray_a.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(w_b.detach().numpy(), w_a.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(f_b.grad.numpy(), f_a.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(t_b.grad.numpy(), t_a.grad.numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(orr.sum_reduce_packed(feats, ps).numpy(), orr.sum_reduce(feats, boundary).numpy(), rtol=1e-13)
    # empties first, twice in the middle and last; three rows behind the last offset belong to no pack
    ps_e = np.concatenate([[0], ps[:3], [ps[2]] * 2, ps[3:], [ps[-1]]])
    pad = torch.from_numpy(rng.random((3, 5)))
    f, t = torch.cat([feats, pad]).requires_grad_(), torch.cat([tau, pad[:, :1]]).requires_grad_()
    ray_e, w_e = orr.exponential_integration_packed(f, t, ps_e)
    live = [1, 2, 5, 6, 7, 8]
    assert ray_e.shape[0] == len(lens) + 4 and not ray_e[[0, 3, 4, 9]].any() and not w_e[S:].any()
    assert torch.equal(ray_e[live], ray_b) and torch.equal(w_e[:S], w_b)
    (ray_e.sum() + w_e.sum()).backward()
    assert not f.grad[S:].any() and not t.grad[S:].any() and f.grad[:S].any()
    assert not orr.sum_reduce_packed(f, ps_e)[[0, 3, 4, 9]].any()
    # an infinite tau: the sample takes all the transmittance that is left, nothing behind it gets any, the next pack is untouched
    tau_inf = torch.tensor([[0.5], [float("inf")], [0.5], [0.25]], dtype=torch.float64)
    _, w_inf = orr.exponential_integration_packed(torch.ones(4, 1, dtype=torch.float64), tau_inf, [0, 3, 4])
    np.testing.assert_allclose(w_inf[:, 0].numpy(), [1 - np.exp(-0.5), np.exp(-0.5), 0.0, 1 - np.exp(-0.25)], rtol=1e-12)


def test_fp32_restatement_meets_the_bars_and_the_subtracted_prefix_does_not():
    """The bars the GPU edge tests hold the kernels to (rays 1e-5 / 1e-6, weights 1e-5 / 1e-7, g_feats 1e-5 / 1e-6, g_tau
    1e-4 / 2e-6 of the pack's largest) are attainable in fp32: the restatement of the kernels' own arithmetic with the
    exclusive prefix taken from the neighbour lane stays inside them on every tau family, forward and backward. Taken as
    `incl - t` -- the kernels' earlier form -- it misses them on the two families whose wall shares a chunk with many thin
    samples: (d) 40 x 1e-3 then 1e3 puts the wall's weight ~2e-5 off, (f) 63 x 2e-4 then 2e4 ~1e-3 off."""
    import render_ref as rr
    missed = {}
    for seed, C in ((0, 3), (1, 16), (2, 1)):
        rng = np.random.default_rng(seed)
        for name, tau in rr.tau_families(rng).items():
            n, ps = tau.shape[0], [0, tau.shape[0]]
            feats = rng.random((n, C)).astype(np.float32)
            g_ray, g_w = rng.standard_normal((1, C)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
            f64 = torch.from_numpy(feats).double().requires_grad_()
            t64 = torch.from_numpy(tau).double().reshape(-1, 1).requires_grad_()
            ray_o, w_o = orr.exponential_integration_packed(f64, t64, ps)
            ((ray_o * torch.from_numpy(g_ray).double()).sum() + (w_o[:, 0] * torch.from_numpy(g_w).double()).sum()).backward()
            ray, w = rr.integrate_fwd(feats, tau, ps)
            rr.assert_forward_close(ray, w, ray_o.detach().numpy(), w_o.detach().numpy())
            g_f, g_t = rr.integrate_bwd(feats, tau, ps, g_ray, g_w)
            rr.assert_backward_close(g_f, g_t, f64.grad.numpy(), t64.grad.numpy(), ps)
            for what, fn in (("fwd", lambda: rr.assert_forward_close(*rr.integrate_fwd(feats, tau, ps, "subtract"),
                                                                      ray_o.detach().numpy(), w_o.detach().numpy())),
                             ("bwd", lambda: rr.assert_backward_close(*rr.integrate_bwd(feats, tau, ps, g_ray, g_w, "subtract"),
                                                                       f64.grad.numpy(), t64.grad.numpy(), ps))):
                try:
                    fn()
                except AssertionError:
                    missed.setdefault(name, set()).add(what)
            if name == "d":           # the size of the miss the issue predicts for the wall sample (index 40)
                _, w_sub = rr.integrate_fwd(feats, tau, ps, "subtract")
                rel = abs(float(w_sub[40]) - w_o[40, 0].item()) / w_o[40, 0].item()
                assert 1e-5 < rel < 1e-4, rel
    assert missed.get("d") == {"fwd", "bwd"} and missed.get("f") == {"fwd", "bwd"}, missed
    assert not ({"a", "c", "g"} & set(missed)), missed
