"""The sphere tracer on the MI355X: ``find_depth_bound`` and the fused step kernel (sphere_trace.hip) against the numpy
restatement of their contract (tests/sphere_trace_ref.py, written from include/shacira_hip.h), exactly: indices equal, floats
bit for bit; then ``PackedSDFTracer`` on an analytic sphere and on a ``NeuralSDF`` over an ``OctreeGrid``.

Shapes: packs of 1..40 nuggets plus one each of 1, 64 and 257 (longer than a wave, longer than a workgroup); P = 1, below, at
and above one wave (63, 64, 65), above one workgroup (257, 300)."""
import numpy as np
import pytest
import torch

import sphere_trace_ref as ref

pytestmark = pytest.mark.gpu

MIN_DIS = 0.0003
F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def same_bits(a, b):
    """Equal bit for bit; a NaN matches any NaN (its payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and \
        np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])


def synthetic_packs(P, seed):
    """P packs: lengths 257, 64, 1 first (as many as fit), then random in 1..40; nuggets 0.02..0.12 wide, gaps 0.01..0.08."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 41, P)
    special = [257, 64, 1][:min(P, 3)]
    lengths[:len(special)] = special
    first = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int32)
    end = np.cumsum(lengths).astype(np.int32)
    K = int(end[-1])
    width = rng.uniform(0.02, 0.12, K)
    gap = rng.uniform(0.01, 0.08, K)
    depth = np.zeros((K, 2), dtype=F)
    for p in range(P):
        lo, hi = first[p], end[p]
        entry = rng.uniform(0.5, 2.5) + np.cumsum(gap[lo:hi] + np.concatenate([[0], width[lo:hi - 1]]))
        depth[lo:hi, 0] = entry
        depth[lo:hi, 1] = entry + width[lo:hi]
    return first, end, depth, rng


# ---- find_depth_bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 300])
def test_find_depth_bound_equals_the_contract(dev, P):
    from shacira_amd import render
    first, end, depth, rng = synthetic_packs(P, seed=P)
    lengths = end - first
    curr = (first + rng.integers(0, 1 << 30, P) % lengths).astype(np.int32)
    curr[rng.uniform(size=P) < 0.1] = -1
    at = (first + rng.integers(0, 1 << 30, P) % lengths).astype(np.int64)        # a random nugget of the pack
    frac = rng.uniform(0.05, 0.95, P).astype(F)
    below = depth[first, 0] - F(0.25)
    inside = depth[at, 0] + (depth[at, 1] - depth[at, 0]) * frac
    nxt = np.minimum(at + 1, end - 1)
    in_gap = np.where(nxt > at, depth[at, 1] + (depth[nxt, 0] - depth[at, 1]) * F(0.5), depth[at, 1] + F(0.005))
    beyond = depth[end - 1, 1] + F(0.25)
    on_edge = np.where(frac < 0.5, depth[at, 0], depth[at, 1])                   # q == entry, q == exit: both inclusive
    nan = np.full(P, np.nan, dtype=F)
    mixed = np.choose(rng.integers(0, 6, P), [below, inside, in_gap, beyond, on_edge, nan])
    gd, ge = torch.from_numpy(depth).to(dev), torch.from_numpy(end).to(dev)
    for name, query, c in [("below", below, curr), ("inside", inside, curr), ("gap", in_gap, curr), ("beyond", beyond, curr),
                           ("edge", on_edge, curr), ("nan", nan, curr), ("mixed", mixed, curr), ("from the start", inside, first)]:
        want = ref.find_depth_bound_ref(query, c, end, depth)
        got = render.find_depth_bound(torch.from_numpy(query.astype(F)).to(dev), torch.from_numpy(c).to(dev), ge, gd)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), name
    # the categories are what they claim (P >= 63: enough packs for each to occur)
    if P >= 63:
        live = curr >= 0
        assert (ref.find_depth_bound_ref(beyond, curr, end, depth) == -1).all()
        assert np.array_equal(ref.find_depth_bound_ref(below, curr, end, depth)[live], curr[live])
        assert (ref.find_depth_bound_ref(inside, first, end, depth) == at).all()


def test_find_depth_bound_stays_inside_its_pack_and_advances_the_last_one(dev):
    from shacira_amd.wisp.ops.geometric import find_depth_bound
    depth = np.array([[10 * p + k, 10 * p + k + 0.5] for p in range(3) for k in range(3)], dtype=F)
    info = torch.tensor([1, 0, 0, 1, 0, 0, 1, 0, 0], dtype=torch.bool, device=dev)
    gd = torch.from_numpy(depth).to(dev)
    end = np.array([3, 6, 9], dtype=np.int32)
    # pack 1 has advanced to nugget 4 and pack 0 runs off its own end: -1, not pack 1's first nugget
    curr = np.array([0, 4, 6], dtype=np.int32)
    query = np.array([5.0, 11.2, 20.0], dtype=F)
    got = find_depth_bound(torch.from_numpy(query).to(dev)[:, None], gd, info, curr_idxes=torch.from_numpy(curr).to(dev))
    assert got.cpu().tolist() == ref.find_depth_bound_ref(query, curr, end, depth).tolist() == [-1, 4, 6]
    assert ref.find_depth_bound_reference_rule(query, curr, depth)[0] == 3
    # the last pack must advance to its third nugget; curr defaults to the pack starts
    query = np.array([0.2, 10.2, 22.2], dtype=F)
    got = find_depth_bound(torch.from_numpy(query).to(dev), gd, info)
    assert got.cpu().tolist() == [0, 3, 8]
    assert ref.find_depth_bound_reference_rule(query, np.array([0, 3, 6]), depth).tolist() == [0, 3, -1]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        find_depth_bound(torch.from_numpy(query), gd.cpu(), info.cpu())


# ---- the step kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step_size,finite_max", [(1.0, False), (0.5, True)])
@pytest.mark.parametrize("P", [1, 64, 65, 257])
def test_step_kernel_equals_the_contract_after_every_iteration(dev, P, step_size, finite_max):
    from shacira_amd import render
    rounds = 8
    first, end, depth, rng = synthetic_packs(P, seed=100 + P)
    K = depth.shape[0]
    o = rng.uniform(-1, 1, (P, 3)).astype(F)
    d = rng.standard_normal((P, 3)).astype(F)
    pidx = rng.integers(0, 1 << 20, K).astype(np.int32)
    given = rng.uniform(0.0, 0.25, (rounds, P)).astype(F)
    kind = rng.uniform(size=(rounds, P))
    given[kind < 0.04] = F(MIN_DIS * 0.5)                                  # below min_dis: a hit by the first criterion
    given[(kind >= 0.04) & (kind < 0.08)] = F(MIN_DIS * 3.0)               # in round 0 or twice in a row: by the second
    given[(kind >= 0.08) & (kind < 0.16)] *= F(-0.5)                       # negative: steps back
    given[(kind >= 0.16) & (kind < 0.18)] = np.nan
    given[(kind >= 0.18) & (kind < 0.20)] = np.inf
    dist_max = float(np.median(depth[end - 1, 1])) if finite_max else float("inf")

    snaps = []
    ref.trace_ref(o, d, depth, first, end, lambda x, packs, i: given[i][packs], rounds, step_size, MIN_DIS, dist_max,
                  snapshots=snaps)
    if P >= 64:
        assert len(snaps) >= 2

    tens = [torch.from_numpy(a).to(dev) for a in (o, d, depth, first, end)]
    state = render.SphereTrace(*tens, pidx=torch.from_numpy(pidx).to(dev), step_size=step_size, min_dis=MIN_DIS,
                               dist_max=dist_max)
    ggiven = torch.from_numpy(given).to(dev)
    assert same_bits(state.x.cpu().numpy(), o + d * depth[first, 0][:, None])
    for i, want in enumerate(snaps):
        assert state.count > 0
        state.step(ggiven[i].index_select(0, state.active_list[:state.count].long()))
        for name in ("t", "dist", "dist_prev", "x"):
            assert same_bits(getattr(state, name).cpu().numpy(), want[name]), (i, name)
        assert np.array_equal(state.curr.cpu().numpy(), want["curr"]), i
        assert np.array_equal(state.active.cpu().numpy().astype(bool), want["active"]), i
        assert np.array_equal(state.hit.cpu().numpy().astype(bool), want["hit"]), i
        alive = np.nonzero(want["active"])[0]
        assert state.count == alive.shape[0], i
        got_list = state.active_list[:state.count].cpu().numpy()
        assert np.array_equal(np.sort(got_list), alive), i
        assert same_bits(state.coords[:state.count].cpu().numpy(), want["x"][got_list]), i
        assert np.array_equal(state.pidx_active[:state.count].cpu().numpy(), pidx[want["curr"][got_list]]), i
    if len(snaps) < rounds:
        assert state.count == 0 and state.step(ggiven[0][:0]) == 0


# ---- PackedSDFTracer on an analytic sphere ------------------------------------------------------------------------------------
class _Grid:
    """What the tracer asks of a grid: the occupancy structure's raytrace and the level list."""

    def __init__(self, blas, level):
        self.blas, self.active_lods, self.num_lods = blas, [level], 1

    def raytrace(self, rays, level=None, with_exit=False):
        return self.blas.raytrace(rays, level, with_exit=with_exit)


class SphereNef(torch.nn.Module):
    """sdf = |x| - 0.7 with the operator order of sphere_trace_ref.analytic_sdf, evaluated where the coordinates live."""

    def __init__(self, grid):
        super().__init__()
        self.grid = grid

    def sdf(self, coords, lod_idx=None):
        x = coords
        return dict(sdf=(torch.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) - ref.RADIUS)[:, None])

    def forward(self, channels=None, coords=None, lod_idx=None, pidx=None):
        assert pidx is None or (pidx.shape[0] == coords.shape[0] and bool((pidx >= 0).all()))
        return self.sdf(coords)[channels]

    def get_forward_function(self, channel):
        return lambda x: self.sdf(x)[channel]


@pytest.fixture(scope="module", params=[(4, False), (2, True)], ids=["shell4", "dense2"])
def sphere_scene(request, dev):
    """(nef, rays, the contract's result per pack, pack -> ray) for 512 rays; the reference loop runs once per scene."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.core import Rays
    level, dense = request.param
    blas = OctreeAS(level, ref.occupancy_grid(level, dense).to(dev))
    nef = SphereNef(_Grid(blas, level))
    origins, dirs = ref.make_rays(512)
    rays = Rays(torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev))
    res = blas.raytrace(rays, level, with_exit=True)
    first, end, ray, depth = ref.packs_of(res.ridx.cpu().numpy(), res.depth.cpu().numpy())

    def sdf_fn(x, packs, i):
        return nef.sdf(torch.from_numpy(x).to(dev))["sdf"].cpu().numpy()
    want = {n: ref.trace_ref(origins[ray], dirs[ray], depth, first, end, sdf_fn, n, 1.0, MIN_DIS) for n in (128, 1)}
    return nef, rays, want, ray, origins, dirs


def _expected_buffers(want, ray, N):
    hit = np.zeros(N, dtype=bool)
    xyz, depth = np.zeros((N, 3), dtype=F), np.zeros((N, 1), dtype=F)
    hit[ray] = want["hit"]
    xyz[ray[want["hit"]]] = want["x"][want["hit"]]
    depth[ray[want["hit"]], 0] = want["t"][want["hit"]]
    return hit, xyz, depth


def test_tracer_equals_the_contract_on_the_sphere(sphere_scene):
    from shacira_amd.wisp.tracers import PackedSDFTracer
    nef, rays, want, ray, origins, dirs = sphere_scene
    N = origins.shape[0]
    tracer = PackedSDFTracer(min_dis=MIN_DIS)
    rb = tracer(nef, rays, channels=("rgb", "normal", "depth", "hit", "xyz"))
    hit, xyz, depth = _expected_buffers(want[128], ray, N)
    got_hit, got_xyz, got_depth = rb.hit.cpu().numpy(), rb.xyz.cpu().numpy(), rb.depth.cpu().numpy()
    P = ray.shape[0]
    print(f"packs {P}, hits {int(hit.sum())}, jumps {want[128]['jumps']}, rounds {want[128]['iterations']}")
    assert hit.sum() >= 0.25 * P and (~want[128]["hit"]).sum() >= 0.20 * P
    assert rb.hit.dtype == torch.bool and tuple(rb.xyz.shape) == (N, 3) and tuple(rb.depth.shape) == (N, 1)
    assert np.array_equal(got_hit, hit)
    assert same_bits(got_xyz, xyz) and same_bits(got_depth, depth)
    assert same_bits(got_xyz[hit], origins[hit] + dirs[hit] * got_depth[hit])
    assert not got_xyz[~hit].any() and not got_depth[~hit].any()
    assert not rb.normal.cpu().numpy()[~hit].any() and np.array_equal(rb.alpha.cpu().numpy()[:, 0], hit.astype(F))
    # every hit lies on the sphere (the bound derived in tests/test_sphere_trace_cpu.py)
    radius = np.linalg.norm(got_xyz[hit].astype(np.float64), axis=1)
    assert np.abs(radius - ref.RADIUS).max() <= 20 * MIN_DIS
    # normals: central differences of f = |x| - 0.7 with step e. Truncation e^2 / 6 * |f'''| per axis, and along an axis
    # |f'''| = 3 c (1 - c^2) / rho^2 <= (2 / sqrt(3)) / rho^2 with rho >= r_min - e, r_min = 0.7 - 20 min_dis. Rounding: each of
    # the two field values carries at most 4 * 2^-23 (the rounded x +- e, three products, two sums, a root and a difference of
    # numbers below 1), divided by 2 e. Normalising a vector within delta of a unit vector moves it by at most 2 delta.
    e = 0.005
    trunc = e * e / 6.0 * (2.0 / np.sqrt(3.0)) / (ref.RADIUS - 20 * MIN_DIS - e) ** 2
    rounding = 2 * (4 * 2.0 ** -23) / (2 * e)
    bound = 2.0 * np.sqrt(3.0) * (trunc + rounding)
    err = np.linalg.norm(rb.normal.cpu().numpy()[hit].astype(np.float64) - got_xyz[hit] / radius[:, None], axis=1)
    print(f"largest normal error {err.max():.3e} (bound {bound:.3e})")
    assert err.max() <= bound
    assert same_bits(rb.rgb.cpu().numpy(), ((rb.normal + 1.0) / 2.0).cpu().numpy())
    # twice the same bits
    again = tracer(nef, rays, channels=("rgb", "normal", "depth", "hit", "xyz"))
    for name in ("hit", "xyz", "depth", "normal", "rgb", "alpha"):
        assert torch.equal(getattr(rb, name), getattr(again, name)), name


def test_tracer_step_limits_extra_channels_and_misses(sphere_scene, dev):
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.tracers import PackedSDFTracer
    nef, rays, want, ray, origins, dirs = sphere_scene
    N = origins.shape[0]
    tracer = PackedSDFTracer(min_dis=MIN_DIS)
    none = tracer(nef, rays, channels=("hit", "xyz", "depth"), num_steps=0)
    assert not none.hit.any() and not none.xyz.any() and not none.depth.any() and not none.alpha.any()
    one = tracer(nef, rays, channels=("hit", "xyz", "depth"), num_steps=1)
    hit, xyz, depth = _expected_buffers(want[1], ray, N)
    assert np.array_equal(one.hit.cpu().numpy(), hit) and same_bits(one.xyz.cpu().numpy(), xyz)
    assert same_bits(one.depth.cpu().numpy(), depth)
    # an extra channel is evaluated at the hit points and returned under its name
    rb = tracer(nef, rays, channels=("hit",), extra_channels=("sdf",))
    assert tuple(rb.sdf.shape) == (N, 1) and not rb.sdf[~rb.hit].any()
    assert torch.equal(rb.sdf[rb.hit], nef.sdf(rb.xyz[rb.hit])["sdf"])
    assert not rb.normal.any() and not rb.rgb.any()          # neither was asked for
    # rays that miss the cube: zero buffers, nothing evaluated
    away = Rays(torch.full((7, 3), 3.0, device=dev), torch.nn.functional.normalize(torch.ones(7, 3, device=dev), dim=-1))
    rb = tracer(nef, away, channels=("rgb", "hit"))
    for name, shape in (("xyz", (7, 3)), ("depth", (7, 1)), ("hit", (7,)), ("normal", (7, 3)), ("rgb", (7, 3)), ("alpha", (7, 1))):
        buf = getattr(rb, name)
        assert tuple(buf.shape) == shape and not buf.any(), name
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tracer(nef, Rays(rays.origins.cpu(), rays.dirs.cpu()))


# ---- NeuralSDF on an octree grid ----------------------------------------------------------------------------------------------
def test_neural_sdf_on_a_dense_octree_grid(dev):
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.grids import OctreeGrid
    from shacira_amd.wisp.models.nefs import NeuralSDF
    from shacira_amd.wisp.tracers import PackedSDFTracer
    torch.manual_seed(0)
    grid = OctreeGrid.make_dense(feature_dim=4, base_lod=2, num_lods=2, feature_std=0.1)
    nef = NeuralSDF(grid, hidden_dim=16, num_layers=1).to(dev)
    x = torch.rand(1000, 3, device=dev) * 2 - 1
    with torch.no_grad():
        for batch in (x, x.reshape(250, 4, 3)):
            got = nef.sdf(batch, lod_idx=1)["sdf"]
            assert tuple(got.shape) == (*batch.shape[:-1], 1) and got.dtype == torch.float32
            feats = torch.cat([batch, grid.interpolate(batch, 1)], dim=-1).double()
            h = torch.relu(feats @ nef.decoder.layers[0].weight.double().T + nef.decoder.layers[0].bias.double())
            want = h @ nef.decoder.lout.weight.double().T + nef.decoder.lout.bias.double()
            err = float((got.double() - want).abs().max())
            print(f"sdf error {err:.3e}, largest value {float(want.abs().max()):.3e} (bound 1e-5 of it)")
            assert err <= 1e-5 * float(want.abs().max())
        assert torch.equal(nef(coords=x, lod_idx=1, pidx=torch.zeros(1000, dtype=torch.int32, device=dev), channels="sdf"),
                           nef.sdf(x, lod_idx=1)["sdf"])
        # a field with a closed surface, positive outside it: sum_a relu(|x_a| - 0.3) - 0.05 through six hidden units (a box
        # of half-width about 0.33 with cut corners), bent a little by the grid features through the random weights that stay
        # on those units. Its slope along a ray is at most sqrt(3) (+ the features' share), so step_size = 0.5 never oversteps
        w0, b0 = nef.decoder.layers[0].weight, nef.decoder.layers[0].bias
        w0[:6, 3:] *= 0.05
        w0[:6, :3] = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]], device=dev)
        b0[:6] = -0.3
        nef.decoder.lout.weight.zero_()
        nef.decoder.lout.weight[0, :6] = 1.0
        nef.decoder.lout.bias.fill_(-0.05)
    origins, dirs = ref.make_rays(512, seed=3)
    rays = Rays(torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev))
    rb = PackedSDFTracer(num_steps=128, step_size=0.5)(nef, rays, channels=("rgb", "hit", "depth"))
    assert tuple(rb.xyz.shape) == (512, 3) and tuple(rb.depth.shape) == (512, 1) and tuple(rb.hit.shape) == (512,)
    assert tuple(rb.normal.shape) == (512, 3) and tuple(rb.rgb.shape) == (512, 3) and tuple(rb.alpha.shape) == (512, 1)
    assert rb.hit.dtype == torch.bool and all(getattr(rb, n).dtype == torch.float32 for n in ("xyz", "depth", "normal", "rgb"))
    hit = rb.hit.cpu().numpy()
    print(f"hits {int(hit.sum())} of 512")
    assert hit.sum() >= 32
    xyz, depth = rb.xyz.cpu().numpy(), rb.depth.cpu().numpy()
    assert same_bits(xyz[hit], origins[hit] + dirs[hit] * depth[hit])
    assert not xyz[~hit].any() and not depth[~hit].any()
    assert bool((grid.blas.query(rb.xyz[rb.hit], grid.active_lods[1]).pidx >= 0).all())
    # on the field's own surface: a hit has |dist| < 10 min_dis = 0.003, so the value that caused it was below 0.003 / 0.5, and
    # the field changes by at most its slope (sqrt(3) from the box, well below 0.3 from the scaled features) times that step
    assert bool((nef.sdf(rb.xyz[rb.hit], lod_idx=1)["sdf"].abs() < 0.003 / 0.5 + 2.1 * 0.003).all())
