"""The coordinate gradient of the hash-grid operator on the MI355X: the C-ABI call against the fp64 restatement
(tests/coord_grad_ref.py), bit equality of its variants and of planned / plain / permuted calls, autograd through
``wisp.ops.grid`` and the grid modules, graph capture, and an end-to-end registration against the same loop on the CPU
oracle."""
import numpy as np
import pytest
import torch

from conftest import CONFIGS, geo, table_layout
from coord_grad_ref import assert_close, coord_grad

pytestmark = pytest.mark.gpu

NERF_LEGO = (3, geo(16, 512, 24), 19)      # nerf_lego.yaml's table: 24 levels, F = 4, bw 19
SHAPES = {"A": CONFIGS["A"] + (2,), "B": CONFIGS["B"] + (2,), "Bp": CONFIGS["Bp"] + (2,), "D": CONFIGS["D"] + (2,),
          "lego": NERF_LEGO + (4,)}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "fp64": torch.float64}


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
    """Uniform samples, _problem's edge rows, and points exactly on level-0 / finer cell boundaries."""
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
        c[8:8 + nb] = (k / (2.0 * res0) - 1.0).astype(np.float32)      # res0 * (c * 0.5 + 0.5) = k / 4: integers among them
        c[8:8 + nb:2] = ((k[::2] // 4) * 2.0 / res0 - 1.0).astype(np.float32)   # exact level-0 boundaries
    return c


def _problem(name, N, dtype, seed=0):
    dim, res, bw, F = SHAPES[name]
    sizes, first, T = table_layout(res, bw, dim)
    rng = np.random.default_rng(seed + 1)
    coords = _coords(dim, N, seed, res[0])
    table = (rng.standard_normal((T, F)) * 0.05).astype(np.float32)
    go = rng.standard_normal((N, len(res) * F)).astype(np.float32)
    # the values the device sees (a half table and half gradients are what the restatement widens)
    table = torch.from_numpy(table).to(DTYPES[dtype]).numpy()
    go = torch.from_numpy(go).to(DTYPES[dtype]).numpy()
    return dim, res, bw, F, first, coords, table, go


def _device_call(dev, dim, res, bw, first, coords, table, go, plan=None):
    ops = _ops()
    return ops.hashgrid_coords_backward(dim, torch.from_numpy(coords).to(dev), torch.from_numpy(go).to(dev),
                                        torch.from_numpy(table).to(dev), torch.from_numpy(first).to(dev), res, bw,
                                        plan=plan)


def _with_variant(v):
    from shacira_amd import _lib

    class _V:
        def __enter__(self):
            _lib.set_option("coord_variant", v)

        def __exit__(self, *exc):
            _lib.set_option("coord_variant", -1)
    return _V()


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "fp64"])
@pytest.mark.parametrize("name", ["A", "B", "Bp", "D", "lego"])
def test_parity_with_the_restatement(dev, name, dtype):
    for N in (0, 1, 17, 4099):
        dim, res, bw, F, first, coords, table, go = _problem(name, N, dtype, seed=N)
        got = _device_call(dev, dim, res, bw, first, coords, table, go)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, dim)
        if N == 0:
            continue
        ref, bound = coord_grad(coords, table, first, res, bw, go)
        assert_close(got.cpu().numpy(), ref, bound, rel=1e-5, what=f"{name} {dtype} N={N}")
        if N >= 16:
            g = got.cpu().numpy()
            assert g[3].tolist() == [0.0] * dim and g[4].tolist() == [0.0] * dim     # clamped on every axis
            assert g[2].tolist() == [0.0] * dim                                       # NaN
            assert g[0, 0] == 0.0 and g[1, 0] != 0.0                                  # +1 clamps, -1 passes


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["A", "B", "D", "lego"])
def test_every_variant_gives_the_same_bits(dev, name, dtype):
    ops = _ops()
    N = 100_003 if name in ("D", "lego") else 40_001
    dim, res, bw, F, first, coords, table, go = _problem(name, N, dtype, seed=5)
    tc, tt, tf = torch.from_numpy(coords).to(dev), torch.from_numpy(table).to(dev), torch.from_numpy(first).to(dev)
    tg = torch.from_numpy(go).to(dev)
    plan = ops.hashgrid_plan_buffer(dim, tc, tt, res, bw)
    fwd = ops.hashgrid_interpolate_cuda if dim == 3 else ops.hashgrid_interpolate2d_cuda
    fwd(tc, tt, tf, res, bw, **({} if plan is None else {"plan": plan}))
    outs = {}
    for v in (-1, 0, 3, 8):
        with _with_variant(v):
            outs[v] = ops.hashgrid_coords_backward(dim, tc, tg, tt, tf, res, bw, plan=plan).cpu()
    for v in (0, 3, 8):
        assert torch.equal(outs[v], outs[-1]), f"variant {v}"
    # an unaligned view of grad_output takes the scalar path: same bits
    buf = torch.empty(tg.numel() + 1, dtype=tg.dtype, device=dev)
    view = buf[1:].view(tg.shape)
    view.copy_(tg)
    assert torch.equal(ops.hashgrid_coords_backward(dim, tc, view, tt, tf, res, bw).cpu(), outs[-1])


@pytest.mark.parametrize("N", [1 << 20, (1 << 18) + 13])
def test_planned_and_plain_calls_agree_and_permutation_permutes(dev, N):
    ops = _ops()
    dim, res, bw, F, first, coords, table, go = _problem("D", N, "fp32", seed=7)
    tc, tt, tf = torch.from_numpy(coords).to(dev), torch.from_numpy(table).to(dev), torch.from_numpy(first).to(dev)
    tg = torch.from_numpy(go).to(dev)
    plan = ops.hashgrid_plan_buffer(dim, tc, tt, res, bw)
    assert plan is not None, "S1-shaped batches sort"
    ops.hashgrid_interpolate_cuda(tc, tt, tf, res, bw, plan=plan)
    planned = ops.hashgrid_coords_backward(dim, tc, tg, tt, tf, res, bw, plan=plan)
    plain = ops.hashgrid_coords_backward(dim, tc, tg, tt, tf, res, bw)
    assert torch.equal(planned, plain)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(dev)
    permuted = ops.hashgrid_coords_backward(dim, tc[perm].contiguous(), tg[perm].contiguous(), tt, tf, res, bw)
    assert torch.equal(permuted, plain[perm])
    idx = np.random.default_rng(0).choice(N, 4096, replace=False)
    ref, bound = coord_grad(coords[idx], table, first, res, bw, go[idx])
    assert_close(plain.cpu().numpy()[idx], ref, bound, what="S1 subset")


def _assert_codebook_grads_agree(a, b, first):
    """Two codebook gradients of the same inputs, held to the backward's own 1e-5 bar level by level: every codebook backward
    path (scattered atomics for small batches, the binned passes for large ones) sums with float atomics, so two runs of one
    and the same call differ in the last bits -- bit equality across runs does not exist to be tested."""
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    edges = list(first.cpu().numpy()) + [a.shape[0]]
    for l in range(len(edges) - 1):
        ref = b[edges[l]:edges[l + 1]]
        np.testing.assert_allclose(a[edges[l]:edges[l + 1]], ref, rtol=1e-5, atol=1e-5 * max(np.abs(ref).max(), 1e-30),
                                   err_msg=f"level {l}")


def _grid_inputs(dev, name, N, dtype=torch.float32, seed=11):
    dim, res, bw, F, first, coords, table, go = _problem(name, N, "fp32", seed=seed)
    return (dim, res, bw, torch.from_numpy(coords).to(dev), torch.from_numpy(table).to(dev).to(dtype),
            torch.from_numpy(first).to(dev), torch.from_numpy(go).to(dev))


def _record_codebook_backward(monkeypatch):
    """Spy on the codebook backward the autograd wrapper calls: a copy of every call's arguments, then the real call."""
    ops = _ops()
    real, calls = ops.hashgrid_backward, []

    def spy(*args, **kwargs):
        snap = lambda v: v.detach().clone() if torch.is_tensor(v) else v
        calls.append(([snap(a) for a in args], {k: snap(v) for k, v in kwargs.items()}))
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, "hashgrid_backward", spy)
    return calls


def _same_call(x, y):
    (ax, kx), (ay, ky) = x, y
    assert len(ax) == len(ay) and sorted(kx) == sorted(ky)
    for u, v in list(zip(ax, ay)) + [(kx[k], ky[k]) for k in kx]:
        if torch.is_tensor(u):
            assert u.dtype == v.dtype and u.shape == v.shape and u.is_contiguous() == v.is_contiguous()
            if u.dtype != torch.uint8:          # (plan buffers: same size; their contents are the forward's to fill)
                if u.is_floating_point():       # bit patterns: the edge rows hold NaN coordinates
                    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[u.element_size()]
                    u, v = u.contiguous().view(bits), v.contiguous().view(bits)
                assert torch.equal(u, v)
        else:
            assert u == v


@pytest.mark.parametrize("name,N", [("A", 5000), ("B", 40_001), ("D", 300_000), ("lego", 100_003)])
def test_autograd_gives_coordinates_the_direct_gradient(dev, name, N, monkeypatch):
    from shacira_amd.wisp.ops import grid
    ops = _ops()
    dim, res, bw, tc, tt, tf, tg = _grid_inputs(dev, name, N)
    fn = grid.hashgrid if dim == 3 else grid.hashgrid2d
    sizes = torch.zeros(len(res), dtype=torch.int32, device=dev)
    calls = _record_codebook_backward(monkeypatch)
    # codebook and coordinates learnable
    c = tc.clone().requires_grad_(True)
    cb = tt.clone().requires_grad_(True)
    fn(c, res, bw, len(res) - 1, cb, sizes, tf).backward(tg)
    assert torch.equal(c.grad, ops.hashgrid_coords_backward(dim, tc, tg, tt, tf, res, bw))
    # the codebook gradient comes from exactly the call made without coordinate grad (same arguments, same plan hand-off),
    # and agrees with that call's result to the backward's own bar (its float atomics make two runs differ in the last bits)
    cb2 = tt.clone().requires_grad_(True)
    feats2 = fn(tc, res, bw, len(res) - 1, cb2, sizes, tf)
    feats2.backward(tg)
    assert len(calls) == 2
    _same_call(calls[0], calls[1])
    _assert_codebook_grads_agree(cb.grad, cb2.grad, tf)
    # forward outputs do not depend on who needs a gradient
    c3 = tc.clone().requires_grad_(True)
    assert torch.equal(fn(c3, res, bw, len(res) - 1, tt, sizes, tf), feats2.detach())
    # frozen codebook, learnable coordinates (pose refinement): no codebook backward runs
    c4 = tc.clone().requires_grad_(True)
    fn(c4, res, bw, len(res) - 1, tt, sizes, tf).backward(tg)
    assert torch.equal(c4.grad, c.grad)
    assert len(calls) == 2


def test_no_coordinate_grad_saves_nothing_more(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg = _grid_inputs(dev, "B", 2000)
    sizes = torch.zeros(len(res), dtype=torch.int32, device=dev)
    cb = tt.clone().requires_grad_(True)
    out = grid.HashGridInterpolate2D.apply(tc, res, bw, 0, cb, sizes, tf)
    assert len(out.grad_fn.saved_tensors) == 2          # coords, first_idx: as before
    c = tc.clone().requires_grad_(True)
    out = grid.HashGridInterpolate2D.apply(c, res, bw, 0, cb, sizes, tf)
    assert len(out.grad_fn.saved_tensors) == 3          # + the table


def test_autocast_gradient_is_fp32_at_the_rounded_coordinates(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg = _grid_inputs(dev, "D", 50_000)
    sizes = torch.zeros(len(res), dtype=torch.int32, device=dev)
    c = tc.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        feats = grid.hashgrid(c, res, bw, len(res) - 1, tt, sizes, tf)
    assert feats.dtype == torch.float16
    g16 = tg.half()
    feats.backward(g16)
    assert c.grad.dtype == torch.float32
    c16 = tc.half().float().cpu().numpy()
    ref, bound = coord_grad(c16, tt.half().cpu().numpy(), tf.cpu().numpy(), res, bw, g16.cpu().numpy())
    assert_close(c.grad.cpu().numpy(), ref, bound, what="autocast")


def test_create_graph_raises_for_coordinates(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg = _grid_inputs(dev, "A", 300)
    sizes = torch.zeros(len(res), dtype=torch.int32, device=dev)
    c = tc.clone().requires_grad_(True)
    feats = grid.hashgrid2d(c, res, bw, 0, tt, sizes, tf)
    with pytest.raises(RuntimeError, match="second derivative"):
        torch.autograd.grad((feats * tg).sum(), c, create_graph=True)
    # the codebook-only path keeps today's behaviour
    cb = tt.clone().requires_grad_(True)
    feats = grid.hashgrid2d(tc, res, bw, 0, cb, sizes, tf)
    (g,) = torch.autograd.grad((feats * tg).sum(), cb, create_graph=True)
    assert g.shape == tt.shape


def _direct(dev, grid_mod, coords, table, go_flat):
    ops = _ops()
    dim = coords.shape[-1]
    return ops.hashgrid_coords_backward(dim, coords.reshape(-1, dim).contiguous(), go_flat, table,
                                        grid_mod.codebook_lod_first_idx, grid_mod.resolutions,
                                        grid_mod.codebook_bitwidth)


@pytest.mark.parametrize("mtype", ["sum", "cat"])
def test_hashgrid_module_propagates_to_coordinates(dev, mtype):
    from shacira_amd.wisp.models.grids.hash_grid import HashGrid
    torch.manual_seed(0)
    g = HashGrid.from_geometric(feature_dim=2, num_lods=8, multiscale_type=mtype, resolution_dim=3, feature_std=0.1,
                                codebook_bitwidth=14, min_grid_res=16, max_grid_res=256, blas_level=3).to(dev)
    x = (torch.rand(7, 33, 3, device=dev) * 2 - 1).requires_grad_(True)     # [batch, samples, 3]
    out = g.interpolate(x, len(g.resolutions) - 1)
    w = torch.randn_like(out)
    (out * w).sum().backward()
    # the per-level gradient the module's reductions hand to the operator
    go = w.reshape(-1, w.shape[-1])
    go = go.repeat(1, len(g.resolutions)) if mtype == "sum" else go
    ref = _direct(dev, g, x.detach(), g.codebook.detach(), go.contiguous())
    assert torch.equal(x.grad.reshape(-1, 3), ref)


@pytest.mark.parametrize("mtype", ["sum", "cat"])
def test_latentgrid_kodak_shape_propagates_to_coordinates(dev, mtype):
    from shacira_amd import harness
    torch.manual_seed(0)
    grid, _, _ = harness.kodak_like_grid(num_lods=8, max_grid_res=128)
    grid.multiscale_type = mtype
    with torch.no_grad():      # latents spread over several integers: a fresh grid's round to one value (a flat field)
        grid.codebook.copy_(torch.randn_like(grid.codebook) * 4)
    grid = grid.to(dev)
    x = (torch.rand(5, 40, 2, device=dev) * 2 - 1).requires_grad_(True)
    out = grid.interpolate(x, len(grid.resolutions) - 1)
    w = torch.randn_like(out)
    (out * w).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    # against autograd through the torch oracle on the same decoded table (F == 1 duplicated, as the module does)
    from oracle.hashgrid_torch import hashgrid_forward
    table = grid.latent_dec(grid.codebook).detach()
    if table.shape[1] == 1:
        table = table.repeat(1, 2)
    xc = x.detach().reshape(-1, 2).cpu().requires_grad_(True)
    feats = hashgrid_forward(xc, table.float().cpu(), grid.codebook_lod_first_idx.cpu(), grid.resolutions,
                             grid.codebook_bitwidth)
    if grid.feature_dim == 1:
        feats = feats[:, ::2]
    L = len(grid.resolutions)
    feats = feats.reshape(5, 40, -1)
    feats = feats if mtype == "cat" else feats.reshape(5, 40, L, -1).sum(-2)
    (feats * w.cpu()).sum().backward()
    np.testing.assert_allclose(x.grad.cpu().reshape(-1, 2).numpy(), xc.grad.numpy(), rtol=1e-4,
                               atol=1e-5 * float(xc.grad.abs().max()))


def test_graph_replay_of_forward_and_backward_with_coordinate_grad(dev):
    from shacira_amd.wisp.ops import grid
    dim, res, bw, tc, tt, tf, tg = _grid_inputs(dev, "D", 300_000)
    sizes = torch.zeros(len(res), dtype=torch.int32, device=dev)
    c = tc.clone().requires_grad_(True)
    cb = tt.clone().requires_grad_(True)

    def step():
        c.grad = None
        cb.grad = None
        grid.hashgrid(c, res, bw, len(res) - 1, cb, sizes, tf).backward(tg)
        return c.grad, cb.grad

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    eager_c, eager_cb = [t.clone() for t in step()]
    g = torch.cuda.CUDAGraph()
    c.grad = None
    cb.grad = None
    with torch.cuda.graph(g):
        out_c, out_cb = step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c, eager_c)
    _assert_codebook_grads_agree(out_cb, eager_cb, tf)     # (float atomics: see above)


# Registration, calibrated on the CPU oracle loop below: config B HashGrid (seed 0, feature_std 0.1), 32 x 32 pixel lattice,
# delta_true = (0.010, -0.006), Adam lr 1e-3, 150 steps, MSE of the 'cat' features. The CPU loop ends at
# (0.0100011, -0.0059995) (loss 6.5e-10); the two loops must agree to 5e-5 and both land within 1e-4 of delta_true.
REG_DELTA = (0.010, -0.006)
REG_STEPS, REG_LR, REG_TOL = 150, 1e-3, 5e-5


def _register(interp, coords, target):
    d = torch.zeros(2, device=coords.device, requires_grad=True)
    opt = torch.optim.Adam([d], lr=REG_LR)
    for _ in range(REG_STEPS):
        opt.zero_grad()
        loss = ((interp(coords + d) - target) ** 2).mean()
        loss.backward()
        opt.step()
    return d.detach().cpu().numpy()


def test_registration_matches_the_cpu_oracle_loop(dev):
    from shacira_amd.harness import image_coords
    from shacira_amd.wisp.models.grids.hash_grid import HashGrid
    from oracle.hashgrid_torch import hashgrid_forward
    torch.manual_seed(0)
    g = HashGrid.from_geometric(feature_dim=2, num_lods=16, multiscale_type="cat", resolution_dim=2, feature_std=0.1,
                                codebook_bitwidth=11, min_grid_res=16, max_grid_res=512, blas_level=3)
    g.freeze()
    coords = image_coords(32, 32)
    table, first, res = g.codebook.detach(), g.codebook_lod_first_idx, g.resolutions
    delta = torch.tensor(REG_DELTA)
    cpu_fn = lambda x: hashgrid_forward(x, table, first, res, 11)
    with torch.no_grad():
        target = cpu_fn(coords + delta)
    d_cpu = _register(cpu_fn, coords, target)
    g = g.to(dev)
    gpu_fn = lambda x: g.interpolate(x, len(res) - 1)
    d_gpu = _register(gpu_fn, coords.to(dev), target.to(dev))
    assert np.abs(d_cpu - np.array(REG_DELTA)).max() < 1e-4, d_cpu
    assert np.abs(d_gpu - d_cpu).max() < REG_TOL, (d_gpu, d_cpu)
