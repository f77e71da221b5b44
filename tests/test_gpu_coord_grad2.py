"""Second-order gradients of the hash-grid operator on the MI355X: the C-ABI call behind ``hip_ops.hashgrid_coords_backward2``
against the fp64 restatement (tests/coord_grad2_ref.py), output selection, bit equality of the gathers across runs, sample
order and planned / plain calls, autograd through ``wisp.ops.grid`` with the ``second_order`` switch on and off, autocast, an
eikonal loss end to end against the CPU oracle, and graph capture."""
import functools
import itertools

import numpy as np
import pytest
import torch

from conftest import CONFIGS, geo, table_layout
from coord_grad2_ref import coord_grad2
from coord_grad_ref import assert_close

pytestmark = pytest.mark.gpu

NERF_LEGO = (3, geo(16, 512, 24), 19)      # nerf_lego.yaml's table: 24 levels, F = 4, bw 19
SHAPES = {"A": CONFIGS["A"] + (2,), "B": CONFIGS["B"] + (2,), "Bp": CONFIGS["Bp"] + (2,), "D": CONFIGS["D"] + (2,),
          "lego": NERF_LEGO + (4,)}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16}
HALF_ULP = 2.0 ** -11                      # one rounding to half, relative


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ops():
    from shacira_amd import hip_ops
    return hip_ops


def _coords(dim, N, seed, res0):
    """Uniform samples, edge rows, and points exactly on level-0 / finer cell boundaries (test_gpu_coord_grad's recipe)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    if N >= 16:
        c[0] = 1.0
        c[1] = -1.0
        c[2] = np.nan
        c[3] = 2.5
        c[4] = -9.0
        c[5] = np.float32(1.0) - np.float32(2.0 ** -24)
        c[6] = np.float32(-1.0) + np.float32(2.0 ** -24)
        c[7, 0] = 1.0
        nb = min(N - 8, 64)
        k = rng.integers(0, 4 * res0, (nb, dim))
        c[8:8 + nb] = (k / (2.0 * res0) - 1.0).astype(np.float32)
        c[8:8 + nb:2] = ((k[::2] // 4) * 2.0 / res0 - 1.0).astype(np.float32)   # exact level-0 boundaries
    return c


@functools.lru_cache(maxsize=None)
def _problem(name, N, dtype, seed=0):
    dim, res, bw, F = SHAPES[name]
    sizes, first, T = table_layout(res, bw, dim)
    rng = np.random.default_rng(seed + 1)
    coords = _coords(dim, N, seed, res[0])
    table = (rng.standard_normal((T, F)) * 0.05).astype(np.float32)
    go = rng.standard_normal((N, len(res) * F)).astype(np.float32)
    v = rng.standard_normal((N, dim)).astype(np.float32)
    # the values the device sees (a half table and half gradients are what the restatement widens)
    table = torch.from_numpy(table).to(DTYPES[dtype]).numpy()
    go = torch.from_numpy(go).to(DTYPES[dtype]).numpy()
    return dim, res, bw, F, first, coords, table, go, v


@functools.lru_cache(maxsize=None)
def _reference(name, N, dtype, seed=0):
    dim, res, bw, F, first, coords, table, go, v = _problem(name, N, dtype, seed)
    return coord_grad2(coords, table, first, res, bw, go, v)


def _to(dev, *arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def _assert_gather(got, ref, bound, half, what):
    """|got - ref| <= 1e-5 * A, plus one half rounding of the value where the result is stored as half."""
    got = got.detach().double().cpu().numpy()
    if not half:
        assert_close(got, ref, bound, rel=1e-5, what=what)
        return
    err, lim = np.abs(got - ref), 1e-5 * bound + HALF_ULP * np.abs(ref) + 1e-30
    assert (err <= lim).all(), f"{what}: worst {np.max(err / lim):.3f} of the limit"


def _assert_table_grad(got, ref, first, half, what):
    """(2) against the restatement's touched rows, level by level at the codebook backward's bar (rtol 1e-5, atol 1e-5 of the
    level's maximum; fp16: plus the one final rounding); every other row exactly zero."""
    T = got.shape[0]
    rows, vals = ref["rows"], ref["vals"]
    rest = got.detach().clone()
    if rows.size:
        rest[torch.from_numpy(rows).to(got.device)] = 0
    assert int(torch.count_nonzero(rest)) == 0, f"{what}: rows no sample touches must stay exactly zero"
    if not rows.size:
        return
    g = got.detach()[torch.from_numpy(rows).to(got.device)].double().cpu().numpy()
    edges = list(first) + [T]
    for l in range(len(first)):
        m = (rows >= edges[l]) & (rows < edges[l + 1])
        if not m.any():
            continue
        r = vals[m]
        lim = 1e-5 * np.abs(r) + 1e-5 * max(np.abs(r).max(), 1e-30) + (HALF_ULP * np.abs(r) if half else 0.0)
        err = np.abs(g[m] - r)
        assert (err <= lim).all(), f"{what}: level {l}, worst {np.max(err / lim):.3f} of the limit"


def _assert_table_grads_agree(a, b, first, half=False):
    """Two device results of (2) for the same inputs: the bar above with one of them as the reference."""
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    edges = list(np.asarray(first.cpu() if torch.is_tensor(first) else first)) + [a.shape[0]]
    for l in range(len(edges) - 1):
        x, r = a[edges[l]:edges[l + 1]], b[edges[l]:edges[l + 1]]
        lim = 1e-5 * np.abs(r) + 1e-5 * max(np.abs(r).max(), 1e-30) + (2 * HALF_ULP * np.abs(r) if half else 0.0)
        assert (np.abs(x - r) <= lim).all(), f"level {l}"


def _call(dev, name, N, dtype, seed=0, want=(True, True, True), plan=None):
    dim, res, bw, F, first, coords, table, go, v = _problem(name, N, dtype, seed)
    tc, tg, tv, tt, tf = _to(dev, coords, go, v, table, first)
    return _ops().hashgrid_coords_backward2(dim, tc, tg, tv, tt, tf, res, bw, want=want, plan=plan)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["A", "B", "Bp", "D", "lego"])
def test_parity_with_the_restatement(dev, name, dtype):
    half = dtype == "fp16"
    for N in (0, 1, 17, 4099):
        dim, res, bw, F, first, coords, table, go, v = _problem(name, N, dtype, N)
        ggo, gcb, gc = _call(dev, name, N, dtype, N)
        torch.cuda.synchronize()
        assert ggo.dtype == DTYPES[dtype] and tuple(ggo.shape) == (N, len(res) * F)
        assert gcb.dtype == DTYPES[dtype] and tuple(gcb.shape) == table.shape
        assert gc.dtype == torch.float32 and tuple(gc.shape) == (N, dim)
        if N == 0:
            assert int(torch.count_nonzero(gcb)) == 0
            continue
        ref = _reference(name, N, dtype, N)
        what = f"{name} {dtype} N={N}"
        _assert_gather(ggo, ref["ggo"], ref["ggo_bound"], half, what + " grad_grad_output")
        _assert_gather(gc, ref["gc"], ref["gc_bound"], False, what + " grad_coords")
        _assert_table_grad(gcb, ref, first, half, what + " grad_codebook")
        if N >= 16:
            for n in (0, 2, 3, 4):          # +1, NaN, 2.5, -9: every axis clamped, nothing comes back
                assert not ggo[n].any() and not gc[n].any(), n
            assert gc[7, 0] == 0.0          # x = +1 alone: no x component ...
            assert ggo[7].any()             # ... while the other axes still carry the directional derivative
            assert gc[1].any() and ggo[1].any()       # -1 passes


@pytest.mark.parametrize("name,dtype", [("D", "fp32"), ("B", "fp16"), ("lego", "fp16")])
def test_every_subset_of_the_outputs_gives_the_same_results(dev, name, dtype):
    N = 4099
    dim, res, bw, F, first, *_ = _problem(name, N, dtype, 3)
    full = _call(dev, name, N, dtype, 3)
    for want in itertools.product((False, True), repeat=3):
        out = _call(dev, name, N, dtype, 3, want=want)
        for i in range(3):
            assert (out[i] is not None) == want[i]
        if want[0]:
            assert torch.equal(out[0], full[0])
        if want[2]:
            assert torch.equal(out[2], full[2])
        if want[1]:
            _assert_table_grads_agree(out[1], full[1], first, half=dtype == "fp16")


def test_the_gathers_are_deterministic_across_runs_plans_order_and_alignment(dev):
    ops = _ops()
    N = (1 << 18) + 13
    dim, res, bw, F, first, coords, table, go, v = _problem("D", N, "fp32", 7)
    tc, tg, tv, tt, tf = _to(dev, coords, go, v, table, first)
    plan = ops.hashgrid_plan_buffer(dim, tc, tt, res, bw)
    assert plan is not None, "this batch sorts"
    ops.hashgrid_interpolate_cuda(tc, tt, tf, res, bw, plan=plan)
    want = (True, False, True)
    plain = ops.hashgrid_coords_backward2(dim, tc, tg, tv, tt, tf, res, bw, want=want)
    again = ops.hashgrid_coords_backward2(dim, tc, tg, tv, tt, tf, res, bw, want=want)
    planned = ops.hashgrid_coords_backward2(dim, tc, tg, tv, tt, tf, res, bw, want=want, plan=plan)
    for i in (0, 2):
        assert torch.equal(plain[i], again[i]) and torch.equal(plain[i], planned[i]), i
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(dev)
    permuted = ops.hashgrid_coords_backward2(dim, tc[perm].contiguous(), tg[perm].contiguous(), tv[perm].contiguous(), tt, tf,
                                             res, bw, want=want)
    for i in (0, 2):
        assert torch.equal(permuted[i], plain[i][perm]), i
    # an unaligned view of grad_output takes the scalar path: same bits
    buf = torch.empty(tg.numel() + 1, dtype=tg.dtype, device=dev)
    view = buf[1:].view(tg.shape)
    view.copy_(tg)
    unaligned = ops.hashgrid_coords_backward2(dim, tc, view, tv, tt, tf, res, bw, want=want)
    for i in (0, 2):
        assert torch.equal(unaligned[i], plain[i]), i
    idx = np.random.default_rng(0).choice(N, 2048, replace=False)
    ref = coord_grad2(coords[idx], table, first, res, bw, go[idx], v[idx])
    _assert_gather(plain[0][torch.from_numpy(idx).to(dev)], ref["ggo"], ref["ggo_bound"], False, "subset (1)")
    _assert_gather(plain[2][torch.from_numpy(idx).to(dev)], ref["gc"], ref["gc_bound"], False, "subset (3)")


def _grid_inputs(dev, name, N, seed=11):
    dim, res, bw, F, first, coords, table, go, v = _problem(name, N, "fp32", seed)
    tc, tg, tv, tt, tf = _to(dev, coords, go, v, table, first)
    sizes = torch.zeros(len(res), dtype=torch.int32, device=dev)
    return dim, res, bw, tc, tt, tf, tg, tv, sizes


def _spy_on_want(monkeypatch):
    ops = _ops()
    real, wants = ops.hashgrid_coords_backward2, []

    def spy(*args, **kwargs):
        wants.append(tuple(kwargs["want"]))
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, "hashgrid_coords_backward2", spy)
    return wants


@pytest.mark.parametrize("name,N", [("A", 5000), ("D", 40_001)])
def test_autograd_returns_the_direct_results_and_computes_only_what_is_needed(dev, name, N, monkeypatch):
    from shacira_amd.wisp.ops import grid
    ops = _ops()
    dim, res, bw, tc, tt, tf, tg, tv, sizes = _grid_inputs(dev, name, N)
    fn = grid.hashgrid if dim == 3 else grid.hashgrid2d
    direct = ops.hashgrid_coords_backward2(dim, tc, tg, tv, tt, tf, res, bw)
    first_order = ops.hashgrid_coords_backward(dim, tc, tg, tt, tf, res, bw)
    wants = _spy_on_want(monkeypatch)

    def second(learn_g, learn_cb):
        c = tc.clone().requires_grad_(True)
        cb = tt.clone().requires_grad_(learn_cb)
        g = tg.clone().requires_grad_(learn_g)
        with grid.second_order():
            feats = fn(c, res, bw, len(res) - 1, cb, sizes, tf)
        (gc,) = torch.autograd.grad(feats, c, g, create_graph=True)
        assert torch.equal(gc, first_order)
        wrt = [c] + ([g] if learn_g else []) + ([cb] if learn_cb else [])
        grads = dict(zip(["c"] + (["g"] if learn_g else []) + (["cb"] if learn_cb else []),
                         torch.autograd.grad((gc * tv).sum(), wrt)))
        return grads

    out = second(True, True)
    assert wants == [(True, True, True)]
    assert torch.equal(out["g"], direct[0]) and torch.equal(out["c"], direct[2])
    _assert_table_grads_agree(out["cb"], direct[1], tf)
    out = second(False, False)
    assert wants[-1] == (False, False, True) and torch.equal(out["c"], direct[2])
    out = second(False, True)
    assert wants[-1] == (False, True, True) and torch.equal(out["c"], direct[2])
    out = second(True, False)
    assert wants[-1] == (True, False, True) and torch.equal(out["g"], direct[0])
    assert len(wants) == 4


def _op_node(out):
    """The autograd node of the operator behind hashgrid()'s output (which is a reshape of it)."""
    node = out.grad_fn
    while not type(node).__name__.startswith("HashGridInterpolate"):
        node = node.next_functions[0][0]
    return node


def test_switch_off_keeps_the_first_order_functions(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg, tv, sizes = _grid_inputs(dev, "D", 3000)
    assert not grid.second_order_enabled()
    c = tc.clone().requires_grad_(True)
    off = grid.hashgrid(c, res, bw, len(res) - 1, tt, sizes, tf)
    assert type(_op_node(off)).__name__.startswith("HashGridInterpolateBackward")
    assert len(_op_node(off).saved_tensors) == 3
    with grid.second_order():
        assert grid.second_order_enabled()
        on = grid.hashgrid(c, res, bw, len(res) - 1, tt, sizes, tf)
        plain = grid.hashgrid(tc, res, bw, len(res) - 1, tt.clone().requires_grad_(True), sizes, tf)
    assert not grid.second_order_enabled()
    assert type(_op_node(on)).__name__.startswith("HashGridInterpolateSOBackward")
    assert len(_op_node(on).saved_tensors) == 3
    assert type(_op_node(plain)).__name__.startswith("HashGridInterpolateBackward")   # no coordinate gradient: today's path
    assert len(_op_node(plain).saved_tensors) == 2
    assert torch.equal(on, off) and torch.equal(plain, off)
    # the plain setter
    grid.second_order(True)
    try:
        assert grid.second_order_enabled()
    finally:
        grid.second_order(False)
    assert not grid.second_order_enabled()
    # the switch is read when hashgrid() is called, not at backward time
    with grid.second_order():
        with pytest.raises(RuntimeError, match="second derivative"):
            torch.autograd.grad((off * tg).sum(), c, create_graph=True)


@pytest.mark.parametrize("name,N", [("B", 20_001), ("D", 300_000)])
def test_switch_on_first_order_only_matches_the_switch_off_path(dev, name, N):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg, tv, sizes = _grid_inputs(dev, name, N)
    fn = grid.hashgrid if dim == 3 else grid.hashgrid2d
    grads = []
    for on in (False, True):
        c = tc.clone().requires_grad_(True)
        cb = tt.clone().requires_grad_(True)
        with grid.second_order(on):
            fn(c, res, bw, len(res) - 1, cb, sizes, tf).backward(tg)
        grads.append((c.grad, cb.grad))
    assert torch.equal(grads[0][0], grads[1][0])
    _assert_table_grads_agree(grads[1][1], grads[0][1], tf)


def test_differentiating_the_codebook_gradient_or_a_third_time_raises(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg, tv, sizes = _grid_inputs(dev, "A", 300)
    c = tc.clone().requires_grad_(True)
    cb = tt.clone().requires_grad_(True)
    g = tg.clone().requires_grad_(True)
    with grid.second_order():
        feats = grid.hashgrid2d(c, res, bw, 0, cb, sizes, tf)
    gc, gcb = torch.autograd.grad(feats, [c, cb], g, create_graph=True)
    assert gcb.requires_grad
    with pytest.raises(RuntimeError, match="double backward of the hash-grid codebook gradient"):
        torch.autograd.grad(gcb.sum(), g, retain_graph=True)
    (d_c,) = torch.autograd.grad((gc ** 2).sum(), c, create_graph=True)     # (a loss whose dL/dgc itself has a graph)
    with pytest.raises(RuntimeError, match="third-order"):
        torch.autograd.grad(d_c.sum(), c)
    with grid.second_order():
        with pytest.raises(RuntimeError, match="fp32 and fp16"):
            grid.hashgrid2d(c, res, bw, 0, tt.double(), sizes, tf)


def test_autocast_round_trip(dev):
    from shacira_amd.wisp.ops import grid
    from coord_grad_ref import coord_grad
    dim, res, bw, tc, tt, tf, tg, tv, sizes = _grid_inputs(dev, "D", 50_000)
    c = tc.clone().requires_grad_(True)
    cb = tt.clone().requires_grad_(True)
    with grid.second_order(), torch.autocast("cuda", dtype=torch.float16):
        feats = grid.hashgrid(c, res, bw, len(res) - 1, cb, sizes, tf)
        off = grid.hashgrid(tc, res, bw, len(res) - 1, tt, sizes, tf)
    assert feats.dtype == torch.float16 and torch.equal(feats, off)
    g16 = tg.half().requires_grad_(True)
    (gc,) = torch.autograd.grad(feats, c, g16, create_graph=True)
    assert gc.dtype == torch.float32
    d_g, d_cb, d_c = torch.autograd.grad((gc * tv).sum(), [g16, cb, c])
    assert d_g.dtype == torch.float16 and d_cb.dtype == torch.float32 and d_c.dtype == torch.float32
    c16 = tc.half().float().cpu().numpy()
    t16, g16n, first = tt.half().cpu().numpy(), g16.detach().cpu().numpy(), tf.cpu().numpy()
    ref1, bound1 = coord_grad(c16, t16, first, res, bw, g16n)
    assert_close(gc.detach().cpu().numpy(), ref1, bound1, what="autocast, first order")
    ref = coord_grad2(c16, t16, first, res, bw, g16n, tv.cpu().numpy())
    _assert_gather(d_g, ref["ggo"], ref["ggo_bound"], True, "autocast (1)")
    _assert_gather(d_c, ref["gc"], ref["gc_bound"], False, "autocast (3)")
    _assert_table_grad(d_cb, ref, first, True, "autocast (2)")


@pytest.mark.parametrize("mtype", ["cat", "sum"])
def test_eikonal_loss_end_to_end_against_the_cpu_oracle(dev, mtype):
    from oracle.hashgrid_torch import hashgrid_forward
    from shacira_amd.wisp.models.grids.hash_grid import HashGrid
    from shacira_amd.wisp.ops import grid as grid_ops
    torch.manual_seed(0)
    g = HashGrid.from_geometric(feature_dim=2, num_lods=8, multiscale_type=mtype, resolution_dim=3, feature_std=0.1,
                                codebook_bitwidth=14, min_grid_res=16, max_grid_res=256, blas_level=3)
    L = len(g.resolutions)
    width = 2 * L if mtype == "cat" else 2
    mlp = torch.nn.Sequential(torch.nn.Linear(width, 32), torch.nn.Softplus(), torch.nn.Linear(32, 1))
    x0 = torch.rand(7, 33, 3) * 2 - 1

    def eikonal(interp, params, x):
        sigma = mlp(interp(x))
        (n,) = torch.autograd.grad(sigma.sum(), x, create_graph=True)
        loss = ((n.norm(dim=-1) - 1) ** 2).mean()
        # (the last layer's bias drops out of d sigma / dx: the loss does not depend on it, its gradient is None)
        grads = torch.autograd.grad(loss, params + [x], allow_unused=True)
        return [None if t is None else t.detach().cpu().double().numpy() for t in grads]

    table = g.codebook.detach().clone().requires_grad_(True)
    first, res, bw = g.codebook_lod_first_idx, g.resolutions, g.codebook_bitwidth

    def cpu_interp(x):
        feats = hashgrid_forward(x.reshape(-1, 3), table, first, res, bw).reshape(7, 33, L, 2)
        return feats.reshape(7, 33, -1) if mtype == "cat" else feats.sum(-2)
    ref = eikonal(cpu_interp, [table] + list(mlp.parameters()), x0.clone().requires_grad_(True))
    g, mlp = g.to(dev), mlp.to(dev)
    with grid_ops.second_order():
        got = eikonal(lambda x: g.interpolate(x, L - 1), [g.codebook] + list(mlp.parameters()),
                      x0.to(dev).requires_grad_(True))
    assert len(got) == len(ref) == 6
    for name, a, b in zip(["codebook", "w0", "b0", "w1", "b1", "x"], got, ref):
        if name == "b1":
            assert a is None and b is None
            continue
        assert np.abs(b).max() > 0, name
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * np.abs(b).max(), err_msg=name)


def test_graph_replay_of_forward_and_both_backwards(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg, tv, sizes = _grid_inputs(dev, "D", 300_000)
    c = tc.clone().requires_grad_(True)
    cb = tt.clone().requires_grad_(True)
    g = tg.clone().requires_grad_(True)

    def step():
        with grid.second_order():
            feats = grid.hashgrid(c, res, bw, len(res) - 1, cb, sizes, tf)
        (gc,) = torch.autograd.grad(feats, c, g, create_graph=True)
        return torch.autograd.grad((gc * tv).sum(), [g, cb, c])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    eager = [t.clone() for t in step()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[2], eager[2])
    _assert_table_grads_agree(out[1], eager[1], tf)
