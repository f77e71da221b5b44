"""The sphere tracer without a GPU: the entry points' validation codes, the restatement of the contract
(tests/sphere_trace_ref.py ``trace_ref``) against the reference tracer's masked loop and against the closed form of a sphere,
the two find_depth_bound rules, and the host-side pieces (NeuralSDF, the gradient operators, the sphere samplers)."""
import ctypes

import numpy as np
import pytest
import torch

import sphere_trace_ref as ref
from shacira_amd import _lib

MIN_DIS = 0.0003


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_validate_before_any_launch():
    L = _lib.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first, or there is nothing to do
    fdb, step = L.shacira_find_depth_bound, L.shacira_sphere_trace_step
    assert fdb(0, 0, one, one, one, one, one, None) == 0                          # P == 0: nothing launched
    assert fdb(0, 5, None, None, None, None, None, None) == 0
    assert fdb(-1, 5, one, one, one, one, one, None) == _lib.EINVAL
    assert fdb(5, -1, one, one, one, one, one, None) == _lib.EINVAL
    assert fdb(1 << 31, 1 << 31, one, one, one, one, one, None) == _lib.EINVAL    # int32 indices
    assert fdb(5, 1 << 31, one, one, one, one, one, None) == _lib.EINVAL
    assert fdb(6, 5, one, one, one, one, one, None) == _lib.EINVAL                # a pack holds at least one nugget
    for hole in range(5):
        args = [one] * 5
        args[hole] = None
        assert fdb(5, 9, *args, None) == _lib.EINVAL, hole

    def call(P, K, n, ptrs, pidx=None, pidx_out=None, same_counter=False):
        a_in, sdf, o, d, depth, end, t, dist, prev, curr, x, act, hit, a_out, c_out, cnt, nxt = ptrs
        if same_counter:
            nxt = cnt
        return step(P, K, n, 1, a_in, sdf, o, d, depth, end, pidx, 1.0, MIN_DIS, float("inf"), t, dist, prev, curr, x, act,
                    hit, a_out, c_out, pidx_out, cnt, nxt, None)

    ptrs = [ctypes.c_void_p(16 * (k + 1)) for k in range(17)]
    assert call(5, 9, 0, ptrs) == 0                                               # no active pack: nothing launched
    assert call(0, 0, 0, ptrs) == 0
    assert call(5, 9, -1, ptrs) == _lib.EINVAL
    assert call(5, 9, 6, ptrs) == _lib.EINVAL                                     # more slots than packs
    assert call(-1, 9, 1, ptrs) == _lib.EINVAL
    assert call(5, 1 << 31, 1, ptrs) == _lib.EINVAL
    assert call(1 << 31, 1 << 31, 1, ptrs) == _lib.EINVAL
    assert call(6, 5, 1, ptrs) == _lib.EINVAL
    for hole in range(17):
        holed = list(ptrs)
        holed[hole] = None
        assert call(5, 9, 3, holed) == _lib.EINVAL, hole
    assert call(5, 9, 3, ptrs, pidx=one, pidx_out=None) == _lib.EINVAL            # cell ids asked for, nowhere to put them
    assert call(5, 9, 3, ptrs, same_counter=True) == _lib.EINVAL                  # the two counters must differ
    assert L.shacira_abi_version() == 11


# ---- the contract's loop against the reference's loop and the closed form ----------------------------------------------------
def _literal(case, num_steps, **kw):
    def sdf(x):
        return torch.from_numpy(ref.analytic_sdf(x.numpy()))
    tensors = [torch.from_numpy(np.ascontiguousarray(case[k])) for k in ("o", "d", "depth", "first", "end")]
    return ref.trace_literal(*tensors, sdf, num_steps, **kw)


@pytest.fixture(scope="module")
def level4():
    case = ref.make_case(4)
    out = ref.trace_ref(case["o"], case["d"], case["depth"], case["first"], case["end"], ref.analytic_sdf, 128, 1.0, MIN_DIS)
    return case, out


def test_the_inputs_exercise_hits_misses_and_jumps(level4):
    case, out = level4
    P = case["first"].shape[0]
    print(f"packs {P}, nuggets {case['depth'].shape[0]}, hits {int(out['hit'].sum())}, jumps {out['jumps']}, "
          f"iterations {out['iterations']}")
    assert P >= 100
    assert out["hit"].sum() >= 0.25 * P
    assert (~out["hit"]).sum() >= 0.20 * P
    assert out["jumps"] >= P
    assert out["iterations"] < 128            # the trace ended by itself, not at the step limit
    assert not out["active"].any()


@pytest.mark.parametrize("level,dense,num_steps", [(4, False, 128), (5, False, 128), (2, True, 128), (4, False, 6)])
def test_trace_ref_equals_the_reference_loop_bitwise_on_hit_and_x(level, dense, num_steps):
    case = ref.make_case(level, dense=dense)
    mine = ref.trace_ref(case["o"], case["d"], case["depth"], case["first"], case["end"], ref.analytic_sdf, num_steps, 1.0,
                         MIN_DIS)
    lit = _literal(case, num_steps, min_dis=MIN_DIS)
    assert np.array_equal(mine["hit"], lit["hit"].numpy())
    assert np.array_equal(mine["x"].view(np.uint32), lit["x"].numpy().view(np.uint32))
    assert np.array_equal(mine["x"].view(np.uint32), (case["o"] + case["d"] * mine["t"][:, None]).view(np.uint32))
    if num_steps == 128:
        # the stated deviation: the reference's depth drifts after a ray has retired, the contract's does not
        drift = np.abs(lit["t"].numpy() - mine["t"])[mine["hit"]]
        print(f"level {level}{' dense' if dense else ''}: largest drift of a hit ray's reference depth {drift.max():.4f}")


def test_trace_ref_hits_lie_on_the_sphere(level4):
    """Rays start outside, so dist and dist_prev are positive; the second criterion bounds dist < 10 * min_dis; |x| - 0.7 is
    1-Lipschitz along the step: every hit has ||x| - 0.7| <= 20 * min_dis."""
    case, out = level4
    off = np.abs(np.linalg.norm(out["x"][out["hit"]].astype(np.float64), axis=1) - ref.RADIUS)
    print(f"largest distance of a hit point from the sphere {off.max():.3e} (bound {20 * MIN_DIS:.3e})")
    assert off.max() <= 20 * MIN_DIS


def test_trace_ref_hit_flag_follows_the_discriminant(level4):
    case, out = level4
    approach = ref.closest_approach(case["o"], case["d"])
    clear = np.abs(approach - ref.RADIUS) > 20 * MIN_DIS
    print(f"{int((~clear).sum())} of {clear.shape[0]} packs left out as grazing")
    assert (~clear).sum() <= 0.05 * clear.shape[0]
    assert np.array_equal(out["hit"][clear], (approach < ref.RADIUS)[clear])


# ---- find_depth_bound: the contract's rule and the reference's ------------------------------------------------------------------
def test_both_rules_agree_on_the_first_call_for_every_pack_but_the_last():
    case = ref.make_case(4)
    first, end, depth = case["first"], case["end"], case["depth"]
    rng = np.random.default_rng(1)
    lo, hi = depth[first, 0], depth[end - 1, 1]
    for query in (lo - 0.1, lo + (hi - lo) * rng.uniform(0, 1, lo.shape[0]).astype(np.float32), hi + 0.1):
        a = ref.find_depth_bound_ref(query, first, end, depth)
        b = ref.find_depth_bound_reference_rule(query, first, depth)
        assert np.array_equal(a[:-1], b[:-1])
    inside = ref.find_depth_bound_ref(lo + (hi - lo) * 0.5, first, end, depth)
    assert (inside >= first).all() and (inside < end).all()


def test_a_case_where_the_reference_rule_is_wrong():
    # three packs of three nuggets each: [0, 3), [3, 6), [6, 9); pack p's nuggets cover [10p + k, 10p + k + 0.5], k = 0..2
    depth = np.array([[10 * p + k, 10 * p + k + 0.5] for p in range(3) for k in range(3)], dtype=np.float32)
    first, end = np.array([0, 3, 6], dtype=np.int32), np.array([3, 6, 9], dtype=np.int32)
    # (a) the neighbour has advanced: pack 0 asks for a depth behind its own last exit while pack 1 stands at its 2nd nugget
    curr = np.array([0, 4, 6], dtype=np.int32)
    query = np.array([5.0, 11.2, 20.0], dtype=np.float32)
    mine = ref.find_depth_bound_ref(query, curr, end, depth)
    theirs = ref.find_depth_bound_reference_rule(query, curr, depth)
    assert mine[0] == -1          # pack 0 is exhausted
    assert theirs[0] == 3         # ... the reference hands it pack 1's first nugget
    assert mine[1] == theirs[1] == 4
    # (b) the last pack must advance to its third nugget; the reference bounds its walk by num_packs = 3 < 6
    query = np.array([0.2, 10.2, 22.2], dtype=np.float32)
    mine = ref.find_depth_bound_ref(query, first, end, depth)
    theirs = ref.find_depth_bound_reference_rule(query, first, depth)
    assert mine.tolist() == [0, 3, 8]
    assert theirs.tolist() == [0, 3, -1]
    # NaN and a spent pack
    assert ref.find_depth_bound_ref(np.array([np.nan, 10.0, 20.0], np.float32), np.array([0, -1, 6], np.int32), end,
                                    depth).tolist() == [-1, -1, 6]


# ---- host-side pieces -----------------------------------------------------------------------------------------------------
def _grid(**kw):
    from shacira_amd.wisp.models.grids import OctreeGrid
    return OctreeGrid.make_dense(feature_dim=4, base_lod=1, num_lods=2, feature_std=0.1, **kw)


def test_neural_sdf_constructor_variants_and_names():
    from shacira_amd.wisp.models.nefs import NeuralSDF
    nef = NeuralSDF(_grid(), hidden_dim=16, num_layers=2)
    names = [k for k, _ in nef.named_parameters()]
    assert names == ["grid.features.0", "grid.features.1", "decoder.layers.0.weight", "decoder.layers.0.bias",
                     "decoder.layers.1.weight", "decoder.layers.1.bias", "decoder.lout.weight", "decoder.lout.bias"]
    assert nef.effective_feature_dim() == 8 and nef.pos_embed_dim == 3 and nef.decoder_input_dim() == 11
    assert nef.decoder.layers[0].in_features == 11 and nef.decoder.lout.out_features == 1
    assert set(nef.public_properties()) == {"Grid", "Pos. Embedding", "Decoder (sdf)"}
    assert nef.get_supported_channels() == {"sdf"}
    summed = NeuralSDF(_grid(multiscale_type="sum"), pos_embedder="none", position_input=False)
    assert summed.pos_embedder is None and summed.decoder_input_dim() == 4 and summed.hidden_dim == 128
    embedded = NeuralSDF(_grid(), pos_embedder="positional", pos_multires=4, position_input=True)
    assert embedded.pos_embed_dim == 3 + 3 * 4 * 2 and embedded.decoder_input_dim() == 8 + 27
    bare = NeuralSDF(_grid(), pos_embedder="positional", pos_multires=4, position_input=False)
    assert bare.pos_embed_dim == 24 and bare.decoder_input_dim() == 8     # the reference adds the embedding only with position_input
    assert NeuralSDF(_grid(), pos_embedder="identity").pos_embed_dim == 3
    with pytest.raises(NotImplementedError):
        NeuralSDF(_grid(), pos_embedder="fourier")
    with pytest.raises(NotImplementedError):
        NeuralSDF(_grid(), activation_type="sin")
    with pytest.raises(NotImplementedError):
        NeuralSDF(_grid(), layer_type="spectral_norm")


def test_neural_sdf_forward_drops_arguments_its_function_does_not_take():
    from shacira_amd.wisp.models.nefs import NeuralSDF
    nef = NeuralSDF(_grid(), hidden_dim=16)
    seen = {}

    def fake_sdf(coords, lod_idx=None):
        seen["args"] = (tuple(coords.shape), lod_idx)
        return dict(sdf=coords[..., 0:1] * 2.0)
    nef.sdf = fake_sdf
    nef._forward_functions["sdf"] = fake_sdf
    x = torch.rand(5, 3)
    out = nef(coords=x, lod_idx=1, pidx=torch.arange(5), channels="sdf")
    assert torch.equal(out, x[:, 0:1] * 2.0) and seen["args"] == ((5, 3), 1)
    assert torch.equal(nef(coords=x, pidx=None, channels=["sdf"])["sdf"], out)
    assert torch.equal(nef.get_forward_function("sdf")(x, pidx=torch.arange(5)), out)
    with pytest.raises(Exception, match="not supported"):
        nef(coords=x, channels="rgb")
    with pytest.raises(Exception, match="not supported"):
        nef.get_forward_function("rgb")
    # an empty batch never reaches the grid
    assert NeuralSDF(_grid(), hidden_dim=16).sdf(torch.zeros(0, 3))["sdf"].shape == (0, 1)


def test_gradient_operators_on_a_quadratic():
    from shacira_amd.wisp.ops.differential import autodiff_gradient, finitediff_gradient, tetrahedron_gradient
    A = torch.tensor([[2.0, 0.5, -1.0], [0.5, 1.0, 0.25], [-1.0, 0.25, 3.0]], dtype=torch.float64)
    b = torch.tensor([0.3, -0.7, 1.1], dtype=torch.float64)

    def f(x):
        return (0.5 * ((x @ A) * x).sum(-1, keepdim=True) + x @ b[:, None])
    x = torch.rand(64, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 2 - 1
    want = x @ A + b
    # central differences are exact on a quadratic: fp64 rounding only, |f| <= 10 over the cube and a division by
    # 2 eps = 0.01 -> 1e3 * 10 * 2^-52. The tetrahedron stencil sum_j k_j f(x + h k_j) / (4 h) keeps the second-order term
    # (h / 8) * sum_j k_j (k_j^T A k_j), which vanishes only for a diagonal A (k_j^T A k_j constant, sum_j k_j = 0)
    assert (finitediff_gradient(x, f) - want).abs().max() < 1e-11
    ks = torch.tensor([[1.0, -1.0, -1.0], [-1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    second = (0.005 / 8.0) * sum(k * (k @ A @ k) for k in ks)
    assert (tetrahedron_gradient(x, f) - (want + second)).abs().max() < 1e-11
    diag = torch.diag(torch.tensor([2.0, 1.0, 3.0], dtype=torch.float64))
    assert (tetrahedron_gradient(x, lambda y: 0.5 * ((y @ diag) * y).sum(-1, keepdim=True)) - x @ diag).abs().max() < 1e-11
    assert (autodiff_gradient(x.clone(), f) - want).abs().max() < 1e-13
    assert finitediff_gradient(x.float(), lambda y: f(y.double()).float()).dtype == torch.float32


def test_sphere_samplers():
    from shacira_amd.wisp.models.nefs import nerf
    from shacira_amd.wisp.ops import geometric
    assert nerf.sample_unif_sphere is geometric.sample_unif_sphere
    np.random.seed(0)
    u = geometric.sample_unif_sphere(1000)
    assert u.shape == (1000, 3) and np.allclose(np.linalg.norm(u, axis=1), 1.0)
    assert np.abs(u.mean(axis=0)).max() < 0.1
    fib = geometric.sample_fib_sphere(1000)
    assert fib.shape == (1000, 3) and np.allclose(np.linalg.norm(fib, axis=1), 1.0)
    assert np.abs(fib.mean(axis=0)).max() < 1e-2 and np.all(np.diff(fib[:, 2]) < 0)      # even, and ordered pole to pole


def test_the_tracer_names_its_channels_and_refuses_host_tensors():
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.tracers import PackedSDFTracer
    tracer = PackedSDFTracer()
    assert (tracer.num_steps, tracer.step_size, tracer.min_dis) == (128, 1.0, 0.0003)
    assert tracer.get_supported_channels() == {"depth", "normal", "xyz", "hit", "rgb", "alpha"}
    assert tracer.get_required_nef_channels() == {"sdf"}

    class Nef:
        grid = _grid()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tracer(Nef(), Rays(torch.zeros(4, 3), torch.ones(4, 3)))
