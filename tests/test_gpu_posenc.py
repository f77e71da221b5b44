"""The positional-encoding row kernels (shacira_amd/csrc/posenc.hip) on the MI355X against the fp64 oracle tests/posenc_ref.py,
at the smallest shapes that cross each of their edges: a tile of 256 rows and a block of 256 lanes (N = 0, 1, 63 .. 65, 257, 4099),
every coordinate count, 1 / 4 / 10 bands log and linear, the prefix widths that take the scalar and the 16-byte copy, row-strided
operands and a pointer that is 4-byte aligned only.

Bounds, in units of U = 2^-24 (tests/posenc_ref.py):
  forward     prefix and coordinates bit for bit; sin / cos within 4 U absolute: 4 ulp at [0.5, 1), OpenCL's limit for sin / cos,
              which the device library meets; NaN exactly where the oracle is
  backward    (2F + 8) U * magnitude: two roundings per product, a sequential fp32 sum of 2F + 1 terms, 4 ulp of the saved values
  backward2   3 U * |oracle| (two products), zeros exact
  chain       (4F + 32) U * magnitude
Worst observed figures are printed (``pytest -s``) for profiles/posenc.md."""
import numpy as np
import pytest
import torch

import posenc_ref as R
from shacira_amd import hip_ops
from shacira_amd.wisp.models.embedders import PositionalEmbedder

pytestmark = pytest.mark.gpu
U = R.U
SPECIAL = np.array([1.0, -1.0, 0.0, -0.0, 1e-30, 1e-40, 1e4, -1e4, np.nan, np.inf, -np.inf], np.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def make_coords(n, d, seed, special=True):
    """uniform in [-1, 1]; rows 0 .. 10 (when there are that many) hold one special value each, in column (row mod d)."""
    rng = np.random.default_rng([seed, n, d])
    c = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    if special:
        for i, v in enumerate(SPECIAL[:n]):
            c[i, i % d] = v
    return c


def embedder(dev, d, F, inc, log, fused=True):
    return PositionalEmbedder(F, F - 1, log_sampling=log, include_input=inc, input_dim=d, fused=fused).to(dev)


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (N, d, F, include_input, log bands, P)
N_SWEEP = [(n, 2, 4, True, True, 3) for n in (0, 1, 63, 64, 65, 257, 4099)]
SHAPE_SWEEP = [(257, d, F, inc, log, (0, 1, 3, 32)[(d + F + inc + 2 * log) % 4])
               for d in (2, 3) for F in (1, 4, 10) for inc in (True, False) for log in (True, False)]
EDGE = [(257, 1, 4, True, True, 3), (257, 4, 4, True, False, 32), (257, 4, 64, False, True, 0)]
P_SWEEP = [(4099, 2, 10, False, True, P) for P in (0, 1, 3, 32)] + [(4099, 3, 10, True, False, 32)]
FORWARD_CASES = N_SWEEP + SHAPE_SWEEP + EDGE + P_SWEEP
worst = {"fused": 0.0, "torch": 0.0}


def check_forward(row, coords, prefix, bands, inc, what):
    """The kernel's row [N, P + E] (a tensor) against the oracle. Returns the worst sin / cos error."""
    n, d = coords.shape
    P = 0 if prefix is None else prefix.shape[1]
    want = R.forward(coords, bands, inc, prefix)
    got = row.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, what
    if P:
        assert np.array_equal(bits(got[:, :P]), bits(prefix)), f"{what}: prefix columns"
    e = P
    if inc:
        assert np.array_equal(bits(got[:, P:P + d]), bits(coords)), f"{what}: coordinate columns"
        e += d
    enc, ref = got[:, e:].astype(np.float64), want[:, e:]
    assert np.array_equal(np.isnan(enc), np.isnan(ref)), f"{what}: NaN pattern"
    err = np.nanmax(np.abs(enc - ref)) if enc.size and not np.isnan(ref).all() else 0.0
    assert err <= 4 * U, f"{what}: sin / cos off by {err / U:.2f} U"
    return err


@pytest.mark.parametrize("n,d,F,inc,log,P", FORWARD_CASES)
def test_forward(dev, n, d, F, inc, log, P):
    emb = embedder(dev, d, F, inc, log)
    bands = emb.bands.cpu().numpy()
    coords = make_coords(n, d, 1)
    prefix = np.random.default_rng([2, n, P]).standard_normal((n, P)).astype(np.float32) if P else None
    if P and n:
        prefix.view(np.uint32)[0, 0] = 0x7FC01234          # a NaN payload survives the copy
    x = torch.from_numpy(coords).to(dev)
    what = f"N={n} d={d} F={F} inc={inc} log={log} P={P}"
    if P:
        p = torch.from_numpy(prefix).to(dev)
        row = emb.rows(p, x)
        again = emb.rows(p, x)
    else:
        row = emb(x)
        again = emb(x)
    assert row.shape == (n, P + emb.out_dim) and row.dtype == torch.float32
    assert torch.equal(row.view(torch.int32), again.view(torch.int32)), f"{what}: two calls differ"
    err = check_forward(row, coords, prefix, bands, inc, what)
    # torch's own device sin / cos on the same arguments, for the record
    comp = embedder(dev, d, F, inc, log, fused=False)(x).cpu().numpy().astype(np.float64)
    ref = R.forward(coords, bands, inc)
    with np.errstate(invalid="ignore"):
        terr = np.nanmax(np.abs(comp - ref)[:, (d if inc else 0):]) if n else 0.0
    worst["fused"], worst["torch"] = max(worst["fused"], err), max(worst["torch"], terr)
    print(f"posenc forward {what}: fused {err / U:.3f} U, torch composite {terr / U:.3f} U "
          f"(worst so far {worst['fused'] / U:.3f} / {worst['torch'] / U:.3f})")


def test_forward_strided_and_misaligned_operands(dev):
    n, d, F, P = 257, 3, 4, 32
    emb = embedder(dev, d, F, True, True)
    bands = emb.bands.cpu().numpy()
    coords = make_coords(n, d, 3)
    prefix = np.random.default_rng(4).standard_normal((n, P)).astype(np.float32)
    width = P + emb.out_dim
    wide = torch.from_numpy(np.concatenate([coords, np.full((n, 1), 7.0, np.float32)], 1)).to(dev)      # [N, 4]
    view = wide[:, :d]
    assert not view.is_contiguous()
    p = torch.from_numpy(prefix).to(dev)
    base = hip_ops.posenc_forward(view, emb.bands, p, True)
    check_forward(base, coords, prefix, bands, True, "row-strided coords")
    assert torch.equal(bits_t(emb.rows(p, view)), bits_t(base))
    # a prefix that is a row-strided view, and one whose last stride is not 1 (made contiguous by the binding)
    pwide = torch.cat([p, torch.full((n, 3), 9.0, device=dev)], 1)
    assert torch.equal(bits_t(hip_ops.posenc_forward(view, emb.bands, pwide[:, :P], True)), bits_t(base))
    pt = p.t().contiguous().t()
    assert pt.stride(1) != 1
    assert torch.equal(bits_t(hip_ops.posenc_forward(view, emb.bands, pt, True)), bits_t(base))
    # an output row stride above P + E: the padding columns keep what they held (multiple of 4: the 16-byte path; 5 more: not)
    for pad in (4, 5):
        store = torch.full((n, width + pad), -5.0, device=dev)
        out = hip_ops.posenc_forward(view, emb.bands, p, True, out=store[:, :width])
        assert out.data_ptr() == store.data_ptr()
        assert torch.equal(bits_t(store[:, :width]), bits_t(base)), f"pad {pad}"
        assert bool((store[:, width:] == -5.0).all()), f"pad {pad}: padding columns written"
    # an output that starts 4 bytes into an allocation: the scalar path, same bits; the floats around it untouched
    flat = torch.full((n * width + 2,), -5.0, device=dev)
    out = flat[1:1 + n * width].view(n, width)
    assert out.data_ptr() % 16 == 4
    hip_ops.posenc_forward(view, emb.bands, p, True, out=out)
    assert torch.equal(bits_t(out), bits_t(base)) and flat[0].item() == -5.0 and flat[-1].item() == -5.0
    # ... and a misaligned prefix
    pflat = torch.zeros(n * P + 1, device=dev)
    pmis = pflat[1:].view(n, P)
    pmis.copy_(p)
    assert pmis.data_ptr() % 16 == 4
    assert torch.equal(bits_t(hip_ops.posenc_forward(view, emb.bands, pmis, True)), bits_t(base))


def bits_t(t):
    return t.contiguous().view(torch.int32)


BACKWARD_CASES = [(1, 2, 4, True, True, 3), (65, 2, 4, False, True, 0), (257, 3, 10, True, True, 32),
                  (257, 3, 4, True, False, 1), (257, 2, 1, False, False, 3), (4099, 2, 10, True, True, 32),
                  (4099, 3, 4, False, False, 3), (257, 1, 4, True, True, 3), (257, 4, 10, True, False, 32)]


def _operands(dev, n, d, F, inc, log, P, seed):
    emb = embedder(dev, d, F, inc, log)
    coords = make_coords(n, d, seed)
    prefix = np.random.default_rng([seed, 5, n]).standard_normal((n, P)).astype(np.float32)
    go = np.random.default_rng([seed, 6, n]).standard_normal((n, P + emb.out_dim)).astype(np.float32)
    return emb, coords, prefix, go


@pytest.mark.parametrize("n,d,F,inc,log,P", BACKWARD_CASES)
def test_backward(dev, n, d, F, inc, log, P):
    emb, coords, prefix, go = _operands(dev, n, d, F, inc, log, P, 7)
    bands = emb.bands.cpu().numpy()
    x = torch.from_numpy(coords).to(dev).requires_grad_(True)
    p = torch.from_numpy(prefix).to(dev).requires_grad_(True)
    g = torch.from_numpy(go).to(dev)
    row = emb.rows(p, x)
    gp, gx = torch.autograd.grad(row, (p, x), g, retain_graph=True)
    gp2, gx2 = torch.autograd.grad(row, (p, x), g)
    assert torch.equal(bits_t(gx), bits_t(gx2)) and torch.equal(bits_t(gp), bits_t(gp2))      # repeatable
    assert np.array_equal(bits(gp), bits(go[:, :P])), "the prefix gradient is grad_out's first P columns"
    want, mag = R.backward(R.forward(coords, bands, inc, prefix), go, bands, d, inc, P)
    got = gx.cpu().numpy().astype(np.float64)
    # the non-finite pattern: the composite's autograd on this device
    xc = torch.from_numpy(coords).to(dev).requires_grad_(True)
    comp = torch.cat([p.detach(), embedder(dev, d, F, inc, log, fused=False)(xc)], -1)
    (gxc,) = torch.autograd.grad(comp, xc, g)
    assert np.array_equal(np.isfinite(got), np.isfinite(gxc.cpu().numpy())), "non-finite pattern"
    assert np.array_equal(np.isnan(got), np.isnan(gxc.cpu().numpy()))
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    ratio = np.abs(got - want)[fin] / np.maximum(mag[fin], 1e-300)
    print(f"posenc backward N={n} d={d} F={F} inc={inc} log={log} P={P}: worst {ratio.max() / U:.2f} U of the magnitude "
          f"(bound {2 * F + 8})")
    assert np.all(np.abs(got - want)[fin] <= (2 * F + 8) * U * mag[fin])
    # the kernel on its own, on a row-strided saved row and grad_out
    wide_row = torch.cat([row.detach(), torch.zeros(n, 3, device=dev)], 1)
    wide_g = torch.cat([g, torch.ones(n, 5, device=dev)], 1)
    alone = hip_ops.posenc_backward(wide_row[:, :row.shape[1]], wide_g[:, :row.shape[1]], emb.bands, d, inc, P)
    assert torch.equal(bits_t(alone), bits_t(gx))


@pytest.mark.parametrize("n,d,F,inc,log,P", BACKWARD_CASES)
def test_backward2_alone(dev, n, d, F, inc, log, P):
    emb, coords, prefix, go = _operands(dev, n, d, F, inc, log, P, 8)
    bands = emb.bands.cpu().numpy()
    gg = np.random.default_rng([8, 9, n]).standard_normal((n, d)).astype(np.float32)
    row = emb.rows(torch.from_numpy(prefix).to(dev), torch.from_numpy(coords).to(dev))
    g_row, g_go = hip_ops.posenc_backward2(torch.from_numpy(gg).to(dev), row, torch.from_numpy(go).to(dev), emb.bands, d, inc, P)
    again = hip_ops.posenc_backward2(torch.from_numpy(gg).to(dev), row, torch.from_numpy(go).to(dev), emb.bands, d, inc, P)
    assert torch.equal(bits_t(g_row), bits_t(again[0])) and torch.equal(bits_t(g_go), bits_t(again[1]))
    w_row, w_go = R.backward2(gg, row.cpu().numpy(), go, bands, d, inc, P)
    # An entry is (b * v) * gg_j, two fp32 roundings: 3 U of the oracle as long as both results are normal numbers. The row of the
    # denormal coordinate has sin = 1e-40: there fp32's spacing is 2^-149 whatever the magnitude, each rounding is off by up to
    # 2^-150, the first one scaled by |gg_j|. That absolute term is the number format's, and it is below 1e-43.
    floor = (1.0 + float(np.abs(gg).max())) * 2.0 ** -150
    for name, got, want in (("grad_row", g_row, w_row), ("grad_grad_out", g_go, w_go)):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        fin = np.isfinite(want)
        assert np.all(got[fin & (want == 0)] == 0), f"{name}: a zero is not exact"
        err = np.abs(got - want)[fin]
        normal = np.abs(want)[fin] >= 2.0 ** -120
        print(f"posenc backward2 N={n} d={d} F={F} inc={inc} log={log} P={P} {name}: worst "
              f"{(err[normal] / np.abs(want)[fin][normal]).max() / U:.2f} U of the oracle (bound 3), {int((~normal).sum())} "
              f"entries below 2^-120")
        assert np.all(err <= 3 * U * np.abs(want)[fin] + floor), name
    if inc:
        assert np.array_equal(bits(g_go[:, P:P + d]), bits(gg))


@pytest.mark.parametrize("n,d,F,inc,log,P", BACKWARD_CASES)
def test_chain_double_backward(dev, n, d, F, inc, log, P):
    emb, coords, prefix, _ = _operands(dev, n, d, F, inc, log, P, 10)
    bands = emb.bands.cpu().numpy()
    v = np.random.default_rng([10, 11]).standard_normal(P + emb.out_dim).astype(np.float32)
    x = torch.from_numpy(coords).to(dev).requires_grad_(True)
    p = torch.from_numpy(prefix).to(dev).requires_grad_(True)
    f = (emb.rows(p, x) * torch.from_numpy(v).to(dev)).sum()
    (fx,) = torch.autograd.grad(f, x, create_graph=True)
    L = fx.square().sum()
    grads = torch.autograd.grad(L, (x, p) if P else (x,))
    want, mag = R.chain(coords, bands, v, inc, P)
    got = grads[0].cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) or np.array_equal(np.isfinite(got), fin)
    ratio = np.abs(got - want)[fin] / np.maximum(mag[fin], 1e-300)
    print(f"posenc chain N={n} d={d} F={F} inc={inc} log={log} P={P}: worst {ratio.max() / U:.2f} U of the magnitude "
          f"(bound {4 * F + 32})")
    assert np.all(np.abs(got - want)[fin] <= (4 * F + 32) * U * mag[fin])
    if P:
        gp = grads[1].cpu().numpy()
        rows_fin = np.isfinite(coords).all(1)
        assert np.all(gp[rows_fin] == 0), "dL/dprefix is exactly zero"


def test_graph_capture_replays_the_eager_bits(dev):
    n, d, F, P = 4099, 2, 4, 32
    emb, coords, prefix, go = _operands(dev, n, d, F, False, True, P, 12)
    x = torch.from_numpy(coords).to(dev).requires_grad_(True)
    p = torch.from_numpy(prefix).to(dev).requires_grad_(True)
    g = torch.from_numpy(go).to(dev)

    def step(p, x):
        row = emb.rows(p, x)
        gp, gx = torch.autograd.grad(row, (p, x), g)
        return row.detach(), gp.clone(), gx

    # No autograd graph of p and x may outlive a step on another stream: the gradient accumulators of the two leaves belong to
    # the stream of the forward that created them, and a captured backward that feeds an accumulator made on the default stream
    # makes the default stream wait inside the capture. So the warm-up runs on a side stream and keeps nothing, and the eager
    # reference is taken after the replay, on leaves of its own.
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(p, x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(p, x)
    for t in captured:
        t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = step(p.detach().clone().requires_grad_(True), x.detach().clone().requires_grad_(True))
    for a, b in zip(captured, eager):
        assert torch.equal(bits_t(a), bits_t(b))


def test_autocast_with_a_half_prefix_gives_the_fp32_row(dev):
    n, d, F, P = 257, 2, 4, 32
    emb, coords, prefix, _ = _operands(dev, n, d, F, True, True, P, 13)
    x = torch.from_numpy(coords).to(dev)
    half = torch.from_numpy(prefix).to(dev).half()
    want = emb.rows(half.float(), x)
    with torch.autocast("cuda", dtype=torch.float16):
        got = emb.rows(half, x)
        alone = emb(x)
    assert got.dtype == torch.float32 and alone.dtype == torch.float32
    assert torch.equal(bits_t(got), bits_t(want)) and torch.equal(bits_t(alone), bits_t(want[:, P:]))
    # a half prefix that needs a gradient gets it in its own type
    h = half.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        emb.rows(h, x).sum().backward()
    assert h.grad.dtype == torch.float16 and bool((h.grad == 1).all())


def test_outside_the_kernels_limits_the_composite_runs(dev):
    """fp64 coordinates, five coordinates, bands elsewhere: the torch composite, bit for bit, with no warning or error."""
    rng = np.random.default_rng(14)
    emb = embedder(dev, 5, 3, True, True)
    plain = embedder(dev, 5, 3, True, True, fused=False)
    x5 = torch.from_numpy(rng.uniform(-1, 1, (33, 5)).astype(np.float32)).to(dev)
    assert torch.equal(emb(x5), plain(x5))
    emb3, plain3 = embedder(dev, 3, 3, True, True), embedder(dev, 3, 3, True, True, fused=False)
    x64 = torch.from_numpy(rng.uniform(-1, 1, (33, 3))).to(dev)
    assert emb3(x64).dtype == torch.float64 and torch.equal(emb3(x64), plain3(x64))
    pre = torch.randn(33, 4, device=dev, dtype=torch.float64)
    assert torch.equal(emb3.rows(pre, x64), torch.cat([pre, plain3(x64)], -1))
