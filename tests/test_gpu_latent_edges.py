"""latent.hip at its edges, against float64: the selector decoder (tests/latent_multi_ref.py), the plain and per-level
decoders and the SGA quantiser (oracle/latent.py), the entropy bottleneck per element (oracle/latent.py and the probe set of
tests/latent_entropy_probes.py) -- at the lane / wave / workgroup edges, above the grid cap (a thread adds several rows in
fp32), with a second trip of the finish kernels' loops, in every selector instantiation, and at NaN / tie / clamp / mask edges.

Every tolerance is a counted rounding bound (EPS = 2^-23, i.e. TWO units of round-to-nearest per counted rounding):

  reduced gradients   |got - ref| <= c EPS sum|term| + EPS |ref|      c = fp32 roundings that form one term + rows one thread
                                                                       adds in fp32 (the block partials are fp64)
  per-element outputs |got - ref| <= c_el EPS sum|products that form the element|

with ``ref`` the float64 sum and ``sum|term|`` its absolute counterpart from the restatement; the counts stand next to each
assertion. Where the SGA sample enters, its own (ill-conditioned) fp32 tolerance is carried to first order on top
(latent_multi_ref.sga_tolerances). The entropy elements use the measured-reference allowance of latent_entropy_probes.py.
Each check prints the worst error as a fraction of its bound before it asserts.
"""
import numpy as np
import pytest
import torch

import latent_entropy_probes as pr
import latent_multi_ref as mr
from oracle import latent as ol

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
TINY = float(np.finfo(np.float32).tiny)
BIG = 2048 * 256 + 257          # 524 545 rows: the grid is capped at 2048 workgroups and 257 threads take a second row
MULTI = [(1, 2), (2, 2), (1, 4), (2, 4), (4, 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ops():
    from shacira_amd import hip_ops
    return hip_ops


def _to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _rows_per_thread(rows, cap=2048):
    blocks = max(1, min((rows + 255) // 256, cap))
    return max(1, -(-rows // (blocks * 256)))


def _within(name, got, ref, tol):
    """|got - ref| <= tol everywhere; prints the worst fraction of the bound first."""
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.size == 0:
        return
    assert np.isfinite(got).all(), f"{name}: non-finite value"
    frac = np.abs(got - ref) / (tol + 1e-300)
    print(f"  {name}: worst error / bound = {float(frac.max()):.3f}")
    assert (np.abs(got - ref) <= tol).all(), f"{name}: {float(frac.max()):.3f} of the bound at {np.unravel_index(frac.argmax(), frac.shape)}"


def _reduced(name, got, ref, abs_sum, c, extra=0.0):
    _within(name, got, ref, c * EPS * np.asarray(abs_sum) + EPS * np.abs(ref) + extra + TINY)


def _elements(name, got, ref, scale, c_el, extra=0.0):
    _within(name, got, ref, c_el * EPS * np.asarray(scale) + extra + TINY)


# ======================================================================================================= a. selector decoder
def _multi_inputs(seed, rows, ld, F, dft, K, shift=True):
    """alpha on a grid of 1/64 (so that fp32 alpha / T cannot merge two different values into a tie the float64 argmax would
    not see) with exact ties between the two largest entries in two rows out of five: the first maximum must win."""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-6, 6, (rows, ld)).astype(np.float32)
    alpha = (np.rint(rng.standard_normal((K, rows)) * 64) / 64).astype(np.float32)
    if K >= 2 and rows:
        top = alpha.max(0) + np.float32(0.25)
        t0 = np.arange(rows) % 5 == 0
        alpha[K - 2, t0], alpha[K - 1, t0] = top[t0], top[t0]
        if K >= 3:
            t1 = np.arange(rows) % 5 == 1
            alpha[0, t1], alpha[2, t1] = top[t1], top[t1]
    S = 1 if dft else ld
    return dict(latent=lat, alpha=alpha, div=rng.uniform(0.5, 3, ld).astype(np.float32),
                scale=(rng.standard_normal((K, S, F)) * 0.2).astype(np.float32),
                dft=ol.dft_matrix(ld, F) if dft else None,
                shift=(rng.standard_normal((K, F)) * 0.05).astype(np.float32) if shift else None,
                grad_out=rng.standard_normal((rows, F)).astype(np.float32), rng=rng)


def _multi_counts(p, temperature, rows, straight_through=False):
    """Rounding counts of multi_decode_kernel (units of EPS), from its code:
    E_a, the relative error of a soft weight: alpha / T (1) and the subtraction of the maximum (1) are ABSOLUTE errors of
      the exponent, <= 2 amax EPS each side with amax = max|alpha| / T -> 4 amax; expf 2; the K-term denominator K; the
      division 1; the same again for the normalising sum's own terms, bounded with 3 more: 4 amax + K + 6.
    forward element: x = q / div 1, the fma chain over LD LD, * a_k 1 + E_a, the K-term sums K each ('sq' sums twice), the
      shift 1, * a_k 1 + E_a: LD + 2K + 4 + 2 E_a; straight-through: a is an exact one-hot, no E_a.
    reduced terms: x 1, g * asum * a_k 3 + K + 2 E_a, the product with x or zm (LD + 1): LD + K + 5 + 2 E_a, + the rows one
      thread adds.
    backward elements (grad_latent, grad_alpha): the F K fma terms of dx, da_k's F-term sum of (LD + 4)-rounding products, the
      dot over K (2K), asum (K + E_a), the softmax Jacobian (3 + E_a), / div * dq 2: LD + F K + 3K + 10 + 3 E_a."""
    K, _, F = p["scale"].shape
    ld = p["latent"].shape[1]
    amax = float(np.abs(p["alpha"]).max()) / temperature if p["alpha"].size else 0.0
    e_a = 4 * amax + K + 6
    return dict(fwd=ld + 2 * K + 4 + (0 if straight_through else 2 * e_a), red=ld + K + 5 + 2 * e_a + _rows_per_thread(rows),
                bwd=ld + F * K + 3 * K + 10 + 3 * e_a)


def _keep_off_the_clamp_edge(p, args_of, clampw, c_fwd):
    """Re-draws the latents of rows whose float64 output lies within the forward bound of +-clamp: there the fp32 kernel may
    legitimately mask the other way. (The exact-equality case is built separately, with outputs that ARE the clamp value.)"""
    for _ in range(8):
        fw = mr.forward(*args_of(p), clampw)
        near = (np.abs(np.abs(fw["y"]) - clampw) <= 4 * c_fwd * EPS * fw["y_abs"] + 1e-30).any(1)
        if not near.any():
            return
        p["latent"][near] = p["rng"].uniform(-6, 6, (int(near.sum()), p["latent"].shape[1])).astype(np.float32)
    raise AssertionError("could not move the rows off the clamp edge")


def _multi_check(dev, p, temperature=0.7, straight_through=True, clampw=0.0, sga=None, tag="", on_the_edge=False):
    """One forward and one backward of the selector decoder against the restatement. sga = None or diff_sampling (bool);
    on_the_edge: the outputs equal the clamp value by construction, exactly, in fp32 and fp64 alike."""
    ops = _ops()
    rows = p["latent"].shape[0]
    uni = None
    if sga is not None:
        uni = p["rng"].random((rows, p["latent"].shape[1], 2), dtype=np.float32)
    args_of = lambda q: (q["latent"], q["alpha"], uni, temperature, straight_through, bool(sga), q["div"], q["scale"],
                         q["dft"], q["shift"])
    c = _multi_counts(p, temperature, rows, straight_through)
    if clampw > 0 and not on_the_edge:
        _keep_off_the_clamp_edge(p, args_of, clampw, c["fwd"])
    q_tol = dq_tol = None
    if sga is not None:
        q_tol, dq_tol = mr.sga_tolerances(p["latent"], uni, temperature, bool(sga))
    t = {k: _to(dev, v) for k, v in p.items() if k != "rng"}
    tu = _to(dev, uni)
    out = ops.latent_multi_decode_forward(t["latent"], t["alpha"], tu, temperature, straight_through, bool(sga), t["div"],
                                          t["scale"], t["dft"], t["shift"], clampw)
    fw = mr.forward(*args_of(p), clampw, q_tol=q_tol)
    _elements(tag + " forward", _np(out), fw["out"], fw["y_abs"], c["fwd"], fw["y_qtol"])
    gl, ga, gs, gsh = ops.latent_multi_decode_backward(t["latent"], t["alpha"], tu, temperature, straight_through, bool(sga),
                                                       t["div"], t["scale"], t["dft"], t["shift"], clampw, t["grad_out"])
    bw = mr.backward(*args_of(p), clampw, p["grad_out"], q_tol=q_tol, dq_tol=dq_tol)
    _elements(tag + " grad_latent", _np(gl), bw["grad_latent"], bw["grad_latent_abs"], c["bwd"], bw["grad_latent_qtol"])
    _elements(tag + " grad_alpha", _np(ga), bw["grad_alpha"], bw["grad_alpha_abs"], c["bwd"], bw["grad_alpha_qtol"])
    _reduced(tag + " grad_scale", _np(gs), bw["grad_scale"], bw["grad_scale_abs"], c["red"], bw["grad_scale_qtol"])
    if p["shift"] is not None:
        _reduced(tag + " grad_shift", _np(gsh), bw["grad_shift"], bw["grad_shift_abs"], c["red"], bw["grad_shift_qtol"])
    else:
        assert gsh is None
    return fw, bw


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 70_001])
@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (1, 2, True)])
def test_selector_lane_wave_and_workgroup_edges(dev, rows, ld, F, dft):
    """1 / 255 / 256 / 257 rows: the lane and wave edges of one workgroup and the first row of a second; 70 001 rows: 274
    workgroups, so finish_partials_kernel's ``b += 256`` loop takes a second trip in both of its launches (scale part, and the
    shift part at ``partials + kMultiMaxK * SF`` with stride NRED). Straight-through on and off, ties included."""
    for st in (True, False):
        _multi_check(dev, _multi_inputs(rows + ld, rows, ld, F, dft, 3), straight_through=st, tag=f"st={st}")


@pytest.mark.parametrize("dft", [False, True])
@pytest.mark.parametrize("ld,F", MULTI)
def test_selector_every_instantiation_above_256_workgroups(dev, ld, F, dft):
    """All ten (LD, F, dft) instantiations at 70 001 rows (274 workgroups), K = 3, soft and straight-through selector."""
    for st in (True, False):
        fw, _ = _multi_check(dev, _multi_inputs(7 * ld + F, 70_001, ld, F, dft, 3), straight_through=st, tag=f"st={st}")
    assert fw["out"].shape == (70_001, F)


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (1, 2, True)])
def test_selector_decoder_counts(dev, K, ld, F, dft):
    """K = 1 and K = 8: where the loops padded to kMultiMaxK end (no padded lane may leak -inf / 0 into the softmax, the
    mixing or the partials; with K = 8 nothing is padded). 4 099 rows: 17 workgroups, the last one partly filled."""
    for st in (True, False):
        _multi_check(dev, _multi_inputs(K, 4_099, ld, F, dft, K), straight_through=st, tag=f"K={K} st={st}")


@pytest.mark.parametrize("st", [False, True])
@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (2, 4, True)])
def test_selector_above_the_grid_cap(dev, ld, F, dft, st):
    """524 545 rows: grid_for caps the grid at 2048 workgroups, 257 threads walk two rows and add them in fp32 (the +2 in c)."""
    _multi_check(dev, _multi_inputs(11 + st, BIG, ld, F, dft, 3), straight_through=st)


def test_selector_sga_above_the_grid_cap(dev):
    """The SGA instantiation of the reducing kernel at 524 545 rows ((2, 2, sq), soft selector, diff_sampling, T = 0.7)."""
    _multi_check(dev, _multi_inputs(13, BIG, 2, 2, False, 3), straight_through=False, sga=True)


@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (1, 2, True), (4, 2, True)])
def test_selector_without_shift(dev, ld, F, dft):
    """shift = NULL: the kernel reads zeros instead and the second finish launch is skipped."""
    _multi_check(dev, _multi_inputs(5, 4_099, ld, F, dft, 3, shift=False), straight_through=False)


@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (2, 4, True)])
def test_selector_clamp_and_its_closed_mask(dev, ld, F, dft):
    """clamp_weights at the 0.9 quantile of |y|: about a tenth of the outputs clamp and lose their gradient. Then scale = 0 and
    shift = +-clamp with the straight-through one-hot: every output EQUALS the clamp value (0 * x + shift, times exactly 1),
    and torch.clamp passes the gradient there -- a mask written with < instead of <= would return zero gradients."""
    p = _multi_inputs(21, 70_001, ld, F, dft, 3)
    for st in (True, False):
        y = mr.forward(p["latent"], p["alpha"], None, 0.7, st, False, p["div"], p["scale"], p["dft"], p["shift"], 0.0)["y"]
        clampw = float(np.float32(np.quantile(np.abs(y), 0.9)))
        fw, _ = _multi_check(dev, p, straight_through=st, clampw=clampw, tag=f"st={st}")
        share = float((np.abs(fw["y"]) > clampw).mean())
        assert 0.05 < share < 0.15, share
    p = _multi_inputs(22, 4_099, ld, F, dft, 3)
    clampw = 0.375
    p["scale"][:] = 0.0
    p["shift"][:] = clampw * np.where(np.arange(3 * F).reshape(3, F) % 2 == 0, 1.0, -1.0).astype(np.float32)
    fw, bw = _multi_check(dev, p, straight_through=True, clampw=clampw, tag="exact", on_the_edge=True)
    assert (np.abs(fw["y"]) == clampw).all() and (np.abs(bw["grad_shift"]) > 0).all()
    out = _ops().latent_multi_decode_forward(*[_to(dev, p[k]) for k in ("latent", "alpha")], None, 0.7, True, False,
                                             _to(dev, p["div"]), _to(dev, p["scale"]), _to(dev, p["dft"]),
                                             _to(dev, p["shift"]), clampw)
    assert np.array_equal(_np(out), fw["out"])


@pytest.mark.parametrize("temperature", [0.7, 0.05])
@pytest.mark.parametrize("diff", [True, False])
@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (1, 4, True)])
def test_selector_sga(dev, ld, F, dft, diff, temperature):
    """The SGA instantiations (the quantiser shares the selector's temperature), both values of diff_sampling."""
    _multi_check(dev, _multi_inputs(31, 4_099, ld, F, dft, 3), temperature=temperature, straight_through=False, sga=diff,
                 tag=f"T={temperature} diff={diff}")


@pytest.mark.parametrize("ld,F,dft", [(2, 2, False), (2, 4, True)])
def test_selector_backward_of_an_empty_table(dev, ld, F, dft):
    """rows = 0: one workgroup runs no row; every parameter gradient comes back exactly zero (not uninitialised memory)."""
    ops = _ops()
    p = _multi_inputs(1, 0, ld, F, dft, 3)
    t = {k: _to(dev, v) for k, v in p.items() if k != "rng"}
    gl, ga, gs, gsh = ops.latent_multi_decode_backward(t["latent"], t["alpha"], None, 0.7, True, False, t["div"], t["scale"],
                                                       t["dft"], t["shift"], 0.0, t["grad_out"])
    assert gl.shape == (0, ld) and ga.shape == (3, 0)
    assert gs.shape == p["scale"].shape and float(gs.abs().max()) == 0.0 and not torch.isnan(gs).any()
    assert gsh.shape == (3, F) and float(gsh.abs().max()) == 0.0 and not torch.isnan(gsh).any()


# ============================================================================================ b. plain and per-level decoders
def _decode_inputs(seed, rows, ld, F):
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-6, 6, (rows, ld)).astype(np.float32)
    if rows >= 9:
        lat[:9, 0] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 1e-9, -1e-9]
    return dict(latent=lat, div=rng.uniform(0.5, 3, ld).astype(np.float32),
                matrix=(rng.standard_normal((ld, F)) * 0.2).astype(np.float32),
                colscale=rng.uniform(0.5, 2, F).astype(np.float32), shift=(rng.standard_normal(F) * 0.05).astype(np.float32),
                grad_out=rng.standard_normal((rows, F)).astype(np.float32), rng=rng)


def _decode_reference(p, uni, temperature, diff, rows_per_thread):
    """float64 values, absolute counterparts, SGA carry-overs and the rounding counts of latent_decode_*_kernel:
    forward element: z = q / div 1, fma chain LD, * colscale 1, + shift 1 = LD + 3 (the oracle's own float32 forward, which
      rounds each product and sum, is NOT used for the value: it is recomputed here in float64);
    grad_latent: gs = g * cs 1, fma chain F, / div 1, * dq 1 = F + 3;
    grad_matrix term z_c * gs_j: 1 + 1 + 1 = 3;  grad_colscale term g * zm_j: LD + 1 + 1;  grad_shift term g: 0;
      each + the rows one thread adds in fp32."""
    lat, d = p["latent"], p["div"].astype(np.float64).reshape(1, -1)
    ld, F = p["matrix"].shape
    M, cs, sh = p["matrix"].astype(np.float64), p["colscale"].astype(np.float64), p["shift"].astype(np.float64)
    if uni is None:
        q, dq = np.rint(lat.astype(np.float64)), np.ones(lat.shape)
        q_tol, dq_tol = np.zeros(lat.shape), np.zeros(lat.shape)
    else:
        q, dq = mr.quantise(lat, uni, temperature, diff)
        q_tol, dq_tol = mr.sga_tolerances(lat, uni, temperature, diff)
    z, zt = q / d, q_tol / d
    zm, zma, zmt = z @ M, np.abs(z) @ np.abs(M), zt @ np.abs(M)
    g = p["grad_out"].astype(np.float64)
    gs = g * cs
    r = dict(out=zm * cs + sh, out_abs=zma * np.abs(cs) + np.abs(sh), out_qtol=zmt * np.abs(cs), c_out=ld + 3)
    dx_abs = (np.abs(gs) @ np.abs(M).T) / d
    r.update(latent=(gs @ M.T) / d * dq, latent_abs=dx_abs * np.abs(dq), latent_qtol=dx_abs * dq_tol, c_latent=F + 3)
    r.update(matrix=z.T @ gs, matrix_abs=np.abs(z).T @ np.abs(gs), matrix_qtol=zt.T @ np.abs(gs), c_matrix=3 + rows_per_thread)
    r.update(colscale=(g * zm).sum(0), colscale_abs=(np.abs(g) * zma).sum(0), colscale_qtol=(np.abs(g) * zmt).sum(0),
             c_colscale=ld + 2 + rows_per_thread)
    r.update(shift=g.sum(0), shift_abs=np.abs(g).sum(0), shift_qtol=0.0, c_shift=rows_per_thread)
    return r


def _decode_compare(tag, got_out, got_bw, r):
    if got_out is not None:
        _elements(tag + " forward", _np(got_out), r["out"], r["out_abs"], r["c_out"], r["out_qtol"])
    gl, gm, gc, gsh = got_bw
    _elements(tag + " grad_latent", _np(gl), r["latent"], r["latent_abs"], r["c_latent"], r["latent_qtol"])
    _reduced(tag + " grad_matrix", _np(gm), r["matrix"], r["matrix_abs"], r["c_matrix"], r["matrix_qtol"])
    _reduced(tag + " grad_colscale", _np(gc), r["colscale"], r["colscale_abs"], r["c_colscale"], r["colscale_qtol"])
    _reduced(tag + " grad_shift", _np(gsh), r["shift"], r["shift_abs"], r["c_shift"], r["shift_qtol"])


@pytest.mark.parametrize("ld,F,mode", [(2, 2, "round"), (2, 2, "sga diff"), (2, 2, "sga"), (8, 8, "round"), (8, 8, "sga diff")])
def test_decode_above_the_grid_cap(dev, ld, F, mode):
    """latent_decode_forward / _backward and the SGA pair at 524 545 rows ((8, 8): 80 reduced values, the widest): the
    grid-stride loop, two rows per thread in fp32, eight trips of the finish loop. The float64 reference agrees with
    oracle.latent.decode_* (asserted here at the oracle's own float32 rounding), which the golden vectors pin."""
    ops = _ops()
    p = _decode_inputs(ld * 10 + F, BIG, ld, F)
    t = {k: _to(dev, v) for k, v in p.items() if k != "rng"}
    n = _rows_per_thread(BIG)
    assert n == 2
    if mode == "round":
        out = ops.latent_decode_forward(t["latent"], t["div"], t["matrix"], t["colscale"], t["shift"], 0.0)
        bw = ops.latent_decode_backward(t["latent"], t["div"], t["matrix"], t["colscale"], t["shift"], 0.0, t["grad_out"], True)
        r = _decode_reference(p, None, 1.0, False, n)
        o_out, _ = ol.decode_forward(p["latent"], p["div"], p["matrix"], p["colscale"], p["shift"], 0.0)
        _elements("oracle forward", o_out, r["out"], r["out_abs"], 2 * (ld + 3))  # numpy float32: a rounding per product and sum
        o_bw = ol.decode_backward(p["latent"], p["div"], p["matrix"], p["colscale"], p["shift"], 0.0, p["grad_out"])
        for k in ("matrix", "colscale", "shift"):                                 # its z and zm are float32: 1 and LD + 1
            _reduced("oracle " + k, o_bw[k], r[k], r[k + "_abs"], ld + 2)
        _decode_compare("round", out, bw, r)
        return
    diff = mode == "sga diff"
    uni = p["rng"].random((BIG, ld, 2), dtype=np.float32)
    tu = _to(dev, uni)
    out = ops.latent_decode_sga_forward(t["latent"], tu, 0.7, diff, t["div"], t["matrix"], t["colscale"], t["shift"], 0.0)
    bw = ops.latent_decode_sga_backward(t["latent"], tu, 0.7, diff, t["div"], t["matrix"], t["colscale"], t["shift"], 0.0,
                                        t["grad_out"], True)
    _decode_compare(mode, out, bw, _decode_reference(p, uni, 0.7, diff, n))


LEVEL_LENGTHS = [0, 1, 255, 256, 257, 32_768, 32_769] + [301 + 7 * i for i in range(9)]


@pytest.mark.parametrize("sga", [None, True])
def test_per_level_decoders_at_their_grid_cap(dev, sga):
    """latent_decode_levels_*: 16 levels of 0, 1, 255, 256, 257, 32 768 and 32 769 rows (decode_launch caps the grid at
    2048 / 16 = 128 workgroups per level: 32 768 rows fill it, 32 769 make one thread take a second row), nine more of 301..357
    rows, and 33 rows no level owns. Each level's slice against the float64 reference of that slice with that level's
    parameters; the unowned tail is exactly zero each way."""
    ops = _ops()
    ld, F, L = 2, 4, 16
    offsets = np.concatenate([[0], np.cumsum(LEVEL_LENGTHS)]).astype(np.int64)
    T = int(offsets[-1]) + 33
    assert len(LEVEL_LENGTHS) == L and 2048 // L * 256 == 32_768
    rng = np.random.default_rng(3)
    lv = [_decode_inputs(100 + l, n, ld, F) for l, n in enumerate(LEVEL_LENGTHS)]
    tail = _decode_inputs(99, 33, ld, F)
    lat = np.concatenate([q["latent"] for q in lv] + [tail["latent"]])
    go = np.concatenate([q["grad_out"] for q in lv] + [tail["grad_out"]])
    stack = lambda k: np.stack([q[k] for q in lv])
    uni = rng.random((T, ld, 2), dtype=np.float32) if sga else None
    args = (_to(dev, lat), [int(o) for o in offsets], _to(dev, uni), 0.7, True, _to(dev, stack("div")),
            _to(dev, stack("matrix")), _to(dev, stack("colscale")), _to(dev, stack("shift")), 0.0)
    out = _np(ops.latent_decode_levels_forward(*args))
    gl, gm, gc, gsh = [_np(x) for x in ops.latent_decode_levels_backward(*args, _to(dev, go))]
    assert out.shape == (T, F) and gm.shape == (L, ld, F) and gc.shape == (L, F) and gsh.shape == (L, F)
    for l, q in enumerate(lv):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        r = _decode_reference(q, None if uni is None else uni[lo:hi], 0.7, True, _rows_per_thread(hi - lo, 2048 // L))
        back = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (gl[lo:hi], gm[l], gc[l], gsh[l]))
        _decode_compare(f"level {l} ({hi - lo} rows)", torch.from_numpy(out[lo:hi]), back, r)
    assert _rows_per_thread(32_769, 2048 // L) == 2 and _rows_per_thread(32_768, 2048 // L) == 1
    assert not out[offsets[-1]:].any() and not gl[offsets[-1]:].any()              # exact zeros, no NaN
    assert not gm[0].any() and not gc[0].any() and not gsh[0].any()                 # the empty level's gradients


@pytest.mark.parametrize("rows", [1, 257, BIG])
@pytest.mark.parametrize("ld,F", [(1, 1), (2, 2), (8, 8)])
def test_one_level_is_the_plain_decoder(dev, ld, F, rows):
    """The contract the shared row loops rest on (the plain backward enters them through a kernel entry of its own, the
    per-level one through LevelRows): latent_decode_levels_* with the one level [0, T] and parameters stacked
    to [1, ...] give, bit for bit, what latent_decode_* give, and with uniforms what latent_decode_sga_* give with the
    temperature on the host and in device memory. 1 row is a single lane, 257 one row past a workgroup, 524 545 above the
    grid cap (a thread takes two rows, the finish loop makes several trips)."""
    ops = _ops()
    p = _decode_inputs(ld * 10 + F, rows, ld, F)
    lat, go = _to(dev, p["latent"]), _to(dev, p["grad_out"])
    par = tuple(_to(dev, p[k]) for k in ("div", "matrix", "colscale", "shift"))
    stacked = tuple(x.unsqueeze(0).contiguous() for x in par)
    uni = _to(dev, p["rng"].random((rows, ld, 2), dtype=np.float32))

    def levels(u):
        a = (lat, [0, rows], u, 0.7, True, *stacked, 0.0)
        return (ops.latent_decode_levels_forward(*a),) + tuple(ops.latent_decode_levels_backward(*a, go))

    def sga(temperature):
        return (ops.latent_decode_sga_forward(lat, uni, temperature, True, *par, 0.0),) + tuple(
            ops.latent_decode_sga_backward(lat, uni, temperature, True, *par, 0.0, go, True))

    plain = (ops.latent_decode_forward(lat, *par, 0.0),) + tuple(ops.latent_decode_backward(lat, *par, 0.0, go, True))
    on_device = torch.full((1,), 0.7, dtype=torch.float32, device=dev)
    for tag, got, want in (("plain", levels(None), plain), ("sga", levels(uni), sga(0.7)), ("device T", levels(uni), sga(on_device))):
        for name, g, w in zip(("decoded", "grad_latent", "grad_matrix", "grad_colscale", "grad_shift"), got, want):
            assert g.numel() == w.numel() and torch.equal(g.reshape(w.shape), w), f"{tag}: {name} differs"


@pytest.mark.parametrize("temperature", [1.0, 0.05])
@pytest.mark.parametrize("diff", [True, False])
def test_sga_quantiser_edge_rows(dev, diff, temperature):
    """sga_quantise at its own edges, per element: q through the forward and dq through grad_latent of the (1, 1) decoder
    with div = matrix = 1 (y = q and grad_latent = g * dq, both exact in fp32 beyond the quantiser itself). Latents exactly
    integer (0, -3, 7), +-0.5, -0.999999 and 0.999999 (the distance to the far neighbour EQUALS the float32 clamp bound
    1 - 1e-6, where torch.clamp still hands the gradient on), 1e6 + 0.5; each with uniforms 0, 1, eps32 and 1 - eps32 in
    either slot; appended to a small random batch. The allowance is what fp32 can hold, and it is wide where the exponents
    are: q moves by 12 eps32 Z (|wf| s0 + |wc| s1), i.e. ~7e-4 |w| at T = 0.05 (Z ~ 470) and +-14..28 around q = 1e6 -- the two
    weights, each good to eps32 Z, no longer add up to one and multiply 1e6 -- so the 1e6 + 0.5 rows check the floor / ceiling
    arithmetic and dq, not which neighbour was drawn. (This test caught the kernel masking that gradient with < at the bound: dq
    of the +-0.999999 rows lacked the far neighbour's term, 27 000 times the bound at T = 1.)"""
    ops = _ops()
    rng = np.random.default_rng(17)
    edge_w = [0.0, -3.0, 7.0, 0.5, -0.5, -0.999999, 0.999999, 1e6 + 0.5]
    edge_u = [0.0, 1.0, EPS, 1.0 - EPS, 0.5]
    cases = [(w, u0, u1) for w in edge_w for u0 in edge_u for u1 in edge_u]
    lat = np.concatenate([rng.uniform(-6, 6, 300), [c[0] for c in cases]]).astype(np.float32).reshape(-1, 1)
    uni = rng.random((lat.shape[0], 1, 2), dtype=np.float32)
    uni[300:, 0, 0], uni[300:, 0, 1] = [c[1] for c in cases], [c[2] for c in cases]
    assert -lat[300 + 5 * 25, 0] == np.float32(1.0 - 1e-6)                          # -0.999999: wc - w is the bound itself
    one = np.ones((1,), np.float32)
    g = rng.standard_normal((lat.shape[0], 1)).astype(np.float32)
    t = [_to(dev, a) for a in (lat, uni, one, one.reshape(1, 1))]
    out = ops.latent_decode_sga_forward(t[0], t[1], temperature, diff, t[2], t[3], None, None, 0.0)
    gl, gm, _, gsh = ops.latent_decode_sga_backward(t[0], t[1], temperature, diff, t[2], t[3], None, None, 0.0, _to(dev, g),
                                                    False)
    q, dq = mr.quantise(lat, uni, temperature, diff)
    q_tol, dq_tol = mr.sga_tolerances(lat, uni, temperature, diff)
    _within("q", _np(out), q, q_tol + TINY)
    _within("dq", _np(gl), g * dq, np.abs(g) * dq_tol + EPS * np.abs(g * dq) + TINY)
    _reduced("grad_matrix", _np(gm), (q * g).sum(0).reshape(1, 1), (np.abs(q * g)).sum(0).reshape(1, 1), 3,
             (q_tol * np.abs(g)).sum())
    _reduced("grad_shift", _np(gsh), g.astype(np.float64).sum(0), np.abs(g).sum(0), 1)


@pytest.mark.parametrize("sga", [None, True])
@pytest.mark.parametrize("clampw", [0.0, 0.3])
def test_a_nan_latent_stays_in_its_row(dev, sga, clampw):
    """One NaN latent (row 700 of 1 031, column 1 of LD = 2, F = 4): the decoded row 700 is NaN, clamped or not (torch.clamp
    keeps NaN), and every other row equals the run without the NaN bit for bit. Backward: the row's z_1 and all its zm_j are
    NaN, so the reductions it feeds with a NaN are grad_matrix[1, :] (terms z_1 * gs_j) and grad_colscale[:] (terms
    g_j * zm_j) -- those are NaN and nothing else is. grad_matrix[0, :] (terms z_0 * gs_j, z_0 finite) and grad_shift (terms
    g_j) take from the row what they take from a finite one: they equal, bit for bit, the run in which the NaN is replaced by
    a finite value (same rows in the same lanes; with a clamp the row's grad_out is zeroed there, as torch.clamp masks a NaN),
    i.e. the row contributes as if it were removed apart from its own finite terms. grad_latent of the other rows is
    unchanged. A second pair of runs zeroes the row's grad_out on both sides: that IS the row removed for every reduction, so
    grad_matrix[0] and grad_shift equal the NaN-free run bit for bit while grad_matrix[1] and grad_colscale are NaN (0 * NaN)
    on the one side and finite on the other -- NaN only because of that row. (This test caught fminf(fmaxf(y, -c), c)
    turning the NaN row into -c in latent_decode_fwd_kernel; the same line of the per-level and selector kernels is held by
    test_a_nan_latent_under_a_clamp_in_the_per_level_and_selector_kernels.)"""
    ops = _ops()
    rows, ld, F, bad = 1_031, 2, 4, 700
    p = _decode_inputs(41, rows, ld, F)
    uni = p["rng"].random((rows, ld, 2), dtype=np.float32) if sga else None
    keep = np.arange(rows) != bad

    def run(lat, go):
        t = [_to(dev, a) for a in (lat, p["div"], p["matrix"], p["colscale"], p["shift"])]
        if uni is None:
            res = (ops.latent_decode_forward(*t, clampw),) + tuple(ops.latent_decode_backward(*t, clampw, _to(dev, go), True))
        else:
            tu = _to(dev, uni)
            res = (ops.latent_decode_sga_forward(t[0], tu, 0.7, True, *t[1:], clampw),) + tuple(
                ops.latent_decode_sga_backward(t[0], tu, 0.7, True, *t[1:], clampw, _to(dev, go), True))
        return [x.cpu().numpy() for x in res]

    go_clean = p["grad_out"].copy()
    if clampw > 0:
        go_clean[bad] = 0.0
    clean = run(p["latent"], go_clean)
    lat = p["latent"].copy()
    lat[bad, 1] = np.nan
    out, gl, gm, gc, gsh = run(lat, p["grad_out"])
    assert np.isnan(out[bad]).all(), out[bad]
    assert np.array_equal(out[keep], clean[0][keep]) and np.array_equal(gl[keep], clean[1][keep])
    assert np.isnan(gm[1]).all() and np.isnan(gc).all()
    assert np.isfinite(gm[0]).all() and np.isfinite(gsh).all()
    assert np.array_equal(gm[0], clean[2][0]) and np.array_equal(gsh, clean[4])
    go0 = p["grad_out"].copy()
    go0[bad] = 0.0
    removed, with_nan = run(p["latent"], go0), run(lat, go0)
    assert all(np.isfinite(x).all() for x in removed)
    assert np.isnan(with_nan[2][1]).all() and np.isnan(with_nan[3]).all()
    assert np.array_equal(with_nan[2][0], removed[2][0]) and np.array_equal(with_nan[4], removed[4])
    assert np.array_equal(with_nan[1][keep], removed[1][keep])


def test_a_nan_latent_under_a_clamp_in_the_per_level_and_selector_kernels(dev):
    """The NaN-keeping clamp of latent_decode_levels_fwd_kernel and multi_decode_kernel (clamp_weights = 0.3; the row's grad_out
    is zero on both sides, so the comparison run is the row removed for every reduction, same rows in the same lanes).
    Per level (levels of 300 and 400 rows, NaN in column 1 of row 350): decoded row 350 is NaN, every other row and all of
    level 0's gradients are bit-identical; of level 1, grad_matrix[1, :] and grad_colscale are NaN, grad_matrix[0, :] and
    grad_shift bit-identical. Selector ((2, 2, sq), K = 3, 600 rows, NaN in column 1 of row 350): decoded row 350 is NaN;
    grad_scale[:, 1, :] (terms x_1 * du) is NaN for every k (0 * NaN), grad_scale[:, 0, :] and grad_shift are bit-identical,
    grad_alpha is NaN in column 350 only (da_k = sum_j g_j (mixed_j + ...), 0 * NaN) and bit-identical elsewhere."""
    ops = _ops()
    ld, F, bad, clampw = 2, 4, 350, 0.3
    lv = [_decode_inputs(51, 300, ld, F), _decode_inputs(52, 400, ld, F)]
    lat = np.concatenate([q["latent"] for q in lv])
    go = np.concatenate([q["grad_out"] for q in lv])
    go[bad] = 0.0
    keep = np.arange(700) != bad
    stack = lambda k: _to(dev, np.stack([q[k] for q in lv]))

    def levels(l_):
        args = (_to(dev, l_), [0, 300, 700], None, 1.0, False, stack("div"), stack("matrix"), stack("colscale"), stack("shift"),
                clampw)
        return [x.cpu().numpy() for x in (ops.latent_decode_levels_forward(*args),) +
                tuple(ops.latent_decode_levels_backward(*args, _to(dev, go)))]

    clean = levels(lat)
    nan_lat = lat.copy()
    nan_lat[bad, 1] = np.nan
    out, gl, gm, gc, gsh = levels(nan_lat)
    assert all(np.isfinite(x).all() for x in clean) and (np.abs(clean[0]) == np.float32(clampw)).any()
    assert np.isnan(out[bad]).all(), out[bad]
    assert np.array_equal(out[keep], clean[0][keep]) and np.array_equal(gl[keep], clean[1][keep])
    assert np.array_equal(gm[0], clean[2][0]) and np.array_equal(gc[0], clean[3][0]) and np.array_equal(gsh[0], clean[4][0])
    assert np.isnan(gm[1][1]).all() and np.isnan(gc[1]).all()
    assert np.array_equal(gm[1][0], clean[2][1][0]) and np.array_equal(gsh[1], clean[4][1])

    p = _multi_inputs(53, 600, 2, 2, False, 3)
    p["scale"] *= 4.0                                       # so that some outputs clamp at 0.3
    p["grad_out"][bad] = 0.0
    keep = np.arange(600) != bad

    def multi(l_):
        t = {k: _to(dev, v) for k, v in p.items() if k != "rng"}
        a = (_to(dev, l_), t["alpha"], None, 0.7, True, False, t["div"], t["scale"], t["dft"], t["shift"], clampw)
        return [x.cpu().numpy() for x in (ops.latent_multi_decode_forward(*a),) +
                tuple(ops.latent_multi_decode_backward(*a, t["grad_out"]))]

    clean = multi(p["latent"])
    nan_lat = p["latent"].copy()
    nan_lat[bad, 1] = np.nan
    out, gl, ga, gs, gsh = multi(nan_lat)
    assert all(np.isfinite(x).all() for x in clean) and (np.abs(clean[0]) == np.float32(clampw)).any()
    assert np.isnan(out[bad]).all(), out[bad]
    assert np.array_equal(out[keep], clean[0][keep]) and np.array_equal(gl[keep], clean[1][keep])
    assert np.isnan(ga[:, bad]).all() and np.array_equal(ga[:, keep], clean[2][:, keep])
    assert np.isnan(gs[:, 1, :]).all() and np.array_equal(gs[:, 0, :], clean[3][:, 0, :])
    assert np.array_equal(gsh, clean[4])


# ================================================================================================= c. entropy per element
@pytest.mark.parametrize("ld", [1, 8])
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
def test_entropy_bits_per_element(dev, nl, ld):
    """Every probe of latent_entropy_probes.py (64 per (num_layers, LD)): the bits from ONE-ROW calls (the C-ABI returns the
    total only; with LD = 8 a row is eight probes, compared as the sum of their intervals plus the 8 fp32 additions), the
    gradient per element from grad_latent of one call with (zero) noise.

    Expectation: the float32 restatement oracle.latent.entropy_elements_f32. Allowance: its prob is known to +-delta,
    delta = 2 x M x eps32 (s_hi + s_lo), M = 6.25 / 14.44 / 26.99 / 26.34 for 1 / 2 / 3 / 4 layers MEASURED on the CPU as the
    float32 restatement's own largest error against float64 over these probes
    (test_oracle_golden.py::test_float32_entropy_restatement_against_fp64), and the factor 2 for __expf, __frcp_rn and
    __log2f, 1-2 ulp each. The bits must lie between the float64 bits at prob + delta and prob - delta; the gradient between
    the values 1 / q takes over that interval (latent_entropy_probes.grad_interval). No probe is left out of the comparison,
    but the issue's delta leaves some of them little to compare: where q - delta <= 0 (every w40 / first_prob0 / midtail
    probe of the steep sets, and the h-10 set at 3 and 4 layers, whose prob ~ 5e-6 is below delta) 1 / q is unbounded, the
    gradient interval is (-inf, inf) and only finiteness is asserted: 18 / 18 / 27 / 26 of the 64 probes for 1 / 2 / 3 / 4
    layers (VACUOUS, printed and pinned below); their bits interval is [~16, 50]. For the probes whose float32 prob is exactly
    0 the bits are held tighter than that, to the values fp32 can reach: both sigmoids are k 2^-24 away from their limit with k
    good to 2 (one ulp of __frcp_rn, one of the exponential under it), so prob is 0 .. 4 x 2^-24 and never negative, i.e.
    bits in [-log2(4 x 2^-24 + 1e-10), -log2(1e-10)] = [21.99, 33.22].
    With LD = 8 a call returns the sum of a row's eight probes and is held to the sum of their intervals: a wide probe in a
    row hides its seven neighbours to that width. Only the LD = 1 runs hold the bits per element (the gradient is per element
    for both). Where fp32 and
    fp64 legitimately part -- the upper tail (prob 0 or a few ulps of 1) and q = prob + 1e-10 == 1 (bits -0.0, gradient passed
    by the clamp) -- the float32 restatement is the expectation like everywhere else; those probes are printed by name.
    (This test caught tanhf_fast = 1 - 2 / (e + 1) near u = 0: probes h20.1/u~+-1e-4 at 3 and 4 layers were 3e-4 off in bits and
    gradient, 50 times the allowance, its absolute 1e-7 multiplied by softplus(20.1) per later layer.)"""
    ops = _ops()
    gt = 0.25
    vacuous = 0
    for names, lat, prm in pr.probes(nl, ld):
        z = np.zeros_like(lat)
        r32, el = ol.entropy_elements_f32(lat, z, prm, nl), ol.entropy_elements(lat, z, prm, nl)
        d = pr.delta(el["s_hi"], el["s_lo"], nl)
        lo, hi = pr.bits_interval(r32["prob"].astype(np.float64), d)
        zero = r32["prob"] == 0
        lo = np.where(zero, np.maximum(lo, pr.bits64(4 * 2.0 ** -24) * (1 - 4 * EPS)), lo)
        hi = np.where(zero, np.minimum(hi, pr.bits64(0.0) * (1 + 4 * EPS)), hi)
        tprm = _to(dev, prm)
        got = np.array([float(ops.entropy_bits_forward(_to(dev, lat[r:r + 1]), _to(dev, z[r:r + 1]), tprm, nl))
                        for r in range(lat.shape[0])])
        slack = ld * EPS * hi.sum(1)                                                  # the row's fp32 additions
        tail, one = pr.legit_differences(r32)
        print(f"  nl={nl} ld={ld}: fp32 != fp64 by right at", sorted({names[i][j] for i, j in zip(*np.nonzero(tail | one))}))
        for r in range(lat.shape[0]):
            print(f"  {names[r]}: bits {got[r]:.7g} in [{lo[r].sum():.7g}, {hi[r].sum():.7g}], float32 restatement "
                  f"{float(r32['bits'][r].astype(np.float64).sum()):.7g}")
        bad = ~((got >= lo.sum(1) - slack) & (got <= hi.sum(1) + slack))
        assert not bad.any(), [names[r] for r in np.nonzero(bad)[0]]
        gl, _ = ops.entropy_bits_backward(_to(dev, lat), _to(dev, z), tprm, nl, torch.full((), gt, device=dev))
        gl = _np(gl)
        glo, ghi = pr.grad_interval(r32["q"], d, el, nl, gt)
        assert np.isfinite(gl).all()
        vacuous += int(np.isinf(ghi).sum())
        bad = ~((gl >= glo - TINY) & (gl <= ghi + TINY))
        assert not bad.any(), [(names[i][j], gl[i, j], glo[i, j], ghi[i, j]) for i, j in zip(*np.nonzero(bad))]
        # validation mode on the same probes: round() has no gradient
        glv, _ = ops.entropy_bits_backward(_to(dev, lat), None, tprm, nl, torch.full((), gt, device=dev))
        assert float(glv.abs().max()) == 0.0 and not torch.isnan(glv).any()
    print(f"  nl={nl} ld={ld}: {vacuous} of 64 gradient probes are unbounded by the allowance")
    assert vacuous == VACUOUS[nl]


VACUOUS = {1: 18, 2: 18, 3: 27, 4: 26}      # probes with q - delta <= 0: computed on the CPU from the probe set and delta alone
HEAD = 2048 * 256                           # rows of the first trip of the grid-stride loop


@pytest.mark.parametrize("ld", [1, 8])
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
def test_entropy_totals_above_the_grid_cap(dev, nl, ld):
    """Total bits, parameter gradients and grad_latent at 524 545 rows (two rows per thread in fp32, grid-stride loop, eight
    trips of the finish loop, grad_total applied by the finish kernel).

    1. The second trip of the grid-stride loop, held tightly: the same call on rows [0, 524 288) (no thread takes two) and on
       the 257 rows past them must add up to the 524 545-row result. The per-row arithmetic is the same code on the same
       inputs, so the only differences are the one fp32 addition in each of the 257 two-row threads and the rounding of the
       three fp32 results: |big - (head + tail)| <= EPS sum|term| over those 514 rows + EPS (|big| + |head| + |tail|). A
       second row lost or counted twice is off by the tail's own sum, ~1e6 times that.
    2. grad_latent per element with grad_interval (as test_entropy_bits_per_element) on the first 257 rows, the 257 rows past
       2048 * 256 and 512 random ones.
    3. Against the float64 oracle. Total: the interval of the bits over prob +- delta summed over the rows, + (3 + n) EPS
       sum(bits) (__log2f 2, the result 1, n = 2 rows added in fp32): 4e-5 .. 2.4e-4 of the total for these inputs, wider than
       the 257 second rows weigh (5e-4 of it) only by a factor 2-11, which is why 1. exists. Parameter gradients:
       c EPS sum|term| + EPS |ref| with c = 12 per Bitparm layer (latent_entropy_probes.grad_interval) + 4 (the products of a
       term and the per-row softplus' / tanh' factor) + n, PLUS, stated separately as the SGA q_tol is, what the allowance on
       prob does to a term gp * s (1 - s) * chain * {x, 1, tanh u}: 1 / q moves by delta / (q - delta) relatively and
       s (1 - s) by (C + 2) EPS s absolutely (C = 2 M: s to C EPS s, hence 1 - s to the same absolute error). That extra is
       hundreds to tens of thousands of EPS sum|term| per entry here, printed below (1 / q is ill-conditioned in the tails): this part holds the per-row mathematics over a
       whole table, parts 1. and 2. the kernel's stride and reduction."""
    ops = _ops()
    rng = np.random.default_rng(nl * 7 + ld)
    lat = rng.uniform(-8, 8, (BIG, ld)).astype(np.float32)
    noise = rng.uniform(-0.5, 0.5, (BIG, ld)).astype(np.float32)
    params = (rng.standard_normal((4, 3, ld)) * 0.4).astype(np.float32)
    n, gt, C = _rows_per_thread(BIG), 0.25, pr.kernel_units(nl)
    el = ol.entropy_elements(lat, noise, params, nl)
    d = pr.delta(el["s_hi"], el["s_lo"], nl)
    q = el["prob"] + 1e-10
    assert (q - d > 0).all()
    gp_abs = gt / (q * pr.LN2)
    tl, tn, tp, tg = _to(dev, lat), _to(dev, noise), _to(dev, params), torch.full((), gt, device=dev)
    tot = float(ops.entropy_bits_forward(tl, tn, tp, nl))
    gl, gp = ops.entropy_bits_backward(tl, tn, tp, nl, tg)
    gp = _np(gp)

    # 1. head + tail = whole
    pair = np.r_[0:BIG - HEAD, HEAD:BIG]                                            # rows of the two-row threads
    tot_h = float(ops.entropy_bits_forward(tl[:HEAD], tn[:HEAD], tp, nl))
    tot_t = float(ops.entropy_bits_forward(tl[HEAD:], tn[HEAD:], tp, nl))
    tol = EPS * float(el["bits"][pair].sum()) + EPS * (abs(tot) + abs(tot_h) + abs(tot_t))
    print(f"  total: whole - (head + tail) = {tot - (tot_h + tot_t):.3g}, bound {tol:.3g}, tail alone {tot_t:.6g}")
    assert abs(tot - (tot_h + tot_t)) <= tol and tot_t > 1e3 * tol
    gp_h = _np(ops.entropy_bits_backward(tl[:HEAD], tn[:HEAD], tp, nl, tg, need_latent=False)[1])
    gp_t = _np(ops.entropy_bits_backward(tl[HEAD:], tn[HEAD:], tp, nl, tg, need_latent=False)[1])
    pe = ol.entropy_elements(lat[pair], noise[pair], params, nl)
    pair_abs = np.zeros(params.shape)
    for s_, tr in ((pe["s_hi"], pe["trace_hi"]), (pe["s_lo"], pe["trace_lo"])):
        pair_abs += ol._cdf_backward_abs(params, tr, gp_abs[pair] * s_ * (1.0 - s_))[1]
    _within("grad_params whole - (head + tail)", gp, gp_h + gp_t,
            EPS * pair_abs + EPS * (np.abs(gp) + np.abs(gp_h) + np.abs(gp_t)) + TINY)
    used = pair_abs > 0
    assert (np.abs(gp_t)[used] > 1e3 * EPS * pair_abs[used]).all()                   # the tail is far above that bound

    # 2. grad_latent per element, second-trip rows included
    idx = np.unique(np.r_[0:BIG - HEAD, HEAD:BIG, rng.integers(0, BIG, 512)])
    r32 = ol.entropy_elements_f32(lat[idx], noise[idx], params, nl)
    sub = ol.entropy_elements(lat[idx], noise[idx], params, nl)
    glo, ghi = pr.grad_interval(r32["q"], d[idx], sub, nl, gt)
    got = _np(gl)[idx]
    assert np.isfinite(_np(gl)).all() and np.isfinite(ghi).all() and (ghi - glo < 0.05 * np.abs(ghi + glo) + 1e-4).mean() > 0.9
    bad = ~((got >= glo - TINY) & (got <= ghi + TINY))
    assert not bad.any(), [(int(idx[i]), j, got[i, j], glo[i, j], ghi[i, j]) for i, j in zip(*np.nonzero(bad))][:8]

    # 3. against float64
    ref = float(el["bits"].sum())
    tol = float((pr.bits64(el["prob"] - d) - pr.bits64(el["prob"] + d)).sum() + (3 + n) * EPS * el["bits"].sum() + EPS * ref)
    print(f"  total bits {tot:.9g} vs {ref:.9g}: error / bound = {abs(tot - ref) / tol:.3f}, bound / total = {tol / ref:.2g}")
    assert abs(tot - ref) <= tol
    _, rp = ol.entropy_bits_backward(lat, noise, params, nl, gt)
    c = 12 * (nl - 1) + 4 + n
    abs_sum, extra = np.zeros(params.shape), np.zeros(params.shape)
    cond = d / (q - d) + np.where(q + d >= 1.0, 1.0, 0.0)            # 1 / q over its interval; the clamp's edge: the whole term
    for s_, tr in ((el["s_hi"], el["trace_hi"]), (el["s_lo"], el["trace_lo"])):
        abs_sum += ol._cdf_backward_abs(params, tr, gp_abs * s_ * (1.0 - s_))[1]
        extra += ol._cdf_backward_abs(params, tr, gp_abs * (s_ * (1.0 - s_) * cond + (C + 2) * EPS * s_))[1]
    used = np.abs(rp) > 0
    assert used.sum() == ld * (2 + 3 * (nl - 1)) and not gp[~used].any()            # unused layers: exact zeros
    print(f"  grad_params: prob allowance / (EPS sum|term|) = {float((extra[used] / (EPS * abs_sum[used])).max()):.0f} at most")
    _reduced("grad_params", gp, rp, abs_sum, c, extra)


def test_entropy_validation_mode_rounds_half_to_even(dev):
    """noise = None: w = round(latent), half to even; +-0.5 / +-1.5 / +-2.5 must give the bits of 0, -0, 2, -2, 2, -2 (the
    float32 restatement of the rounded values, same allowance as above) and grad_latent exactly zero."""
    ops = _ops()
    nl = 2
    prm = pr.set_params(6)
    lat = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], np.float32).reshape(-1, 1)
    want = np.array([0.0, -0.0, 2.0, -2.0, 2.0, -2.0], np.float32).reshape(-1, 1)
    assert np.array_equal(np.rint(lat), want)
    z = np.zeros_like(want)
    r32, el = ol.entropy_elements_f32(want, z, prm, nl), ol.entropy_elements(want, z, prm, nl)
    lo, hi = pr.bits_interval(r32["prob"].astype(np.float64), pr.delta(el["s_hi"], el["s_lo"], nl))
    other = ol.entropy_elements(np.array([[1.0], [-1.0], [3.0], [-3.0]], np.float32), np.zeros((4, 1), np.float32), prm, nl)
    assert np.abs(other["bits"][[0, 1, 0, 1, 2, 3]] - el["bits"][[0, 1, 2, 3, 4, 5]]).min() > 100 * (hi - lo).max()
    for r in range(6):
        got = float(ops.entropy_bits_forward(_to(dev, lat[r:r + 1]), None, _to(dev, prm), nl))
        assert lo[r, 0] <= got <= hi[r, 0], (float(lat[r, 0]), got, lo[r, 0], hi[r, 0])
    gl, _ = ops.entropy_bits_backward(_to(dev, lat), None, _to(dev, prm), nl, torch.ones((), device=dev))
    assert float(gl.abs().max()) == 0.0 and not torch.isnan(gl).any()


def _torch_entropy(lat, noise, params, nl):
    """BitEstimator.total_bits on the CPU in float32 (torch ops, autograd): sum clamp(-log2(prob + 1e-10), 0, 50) -> (total,
    grad_latent, grad_params [4, 3, LD])."""
    from shacira_amd.wisp.models.prob_models.bit_estimator import BitEstimator
    ld = lat.shape[1]
    be = BitEstimator(ld, num_layers=nl)
    fs = (be.f1, be.f2, be.f3, be.f4)
    with torch.no_grad():
        for k, f in enumerate(fs):
            f.h.copy_(torch.from_numpy(params[k, 0]).view(1, -1))
            f.b.copy_(torch.from_numpy(params[k, 1]).view(1, -1))
            if f.a is not None:
                f.a.copy_(torch.from_numpy(params[k, 2]).view(1, -1))
    l = torch.from_numpy(lat).requires_grad_(True)
    tot = be.total_bits(l, None if noise is None else torch.from_numpy(noise))
    tot.backward()
    gp = np.zeros((4, 3, ld), np.float32)
    for k, f in enumerate(fs):
        for s_, name in enumerate(("h", "b", "a")):
            prm = getattr(f, name)
            if prm is not None and prm.grad is not None:
                gp[k, s_] = prm.grad.numpy().reshape(-1)
    return float(tot.detach()), l.grad.numpy(), gp


@pytest.mark.parametrize("nl,ld,mode", [(2, 1, "latent"), (4, 8, "noise"), (3, 2, "validation")])
def test_a_nan_latent_or_noise_reaches_the_bits_and_the_gradients_it_feeds(dev, nl, ld, mode):
    """One NaN (row 255 of 300, the last channel) in the latent, in the noise, or in the latent in validation mode (round()).
    The policy is float32 torch's own for sum(clamp(-log2(prob + 1e-10), 0, 50)), evaluated here on the CPU and pinned:
    the total is NaN (torch.clamp keeps a NaN; fminf(fmaxf()) made it 0 bits); grad_latent is NaN at that element and nowhere
    else (the clamp masks the NaN's gradient to 0, and 0 / NaN in the logarithm's backward is NaN again) -- exactly 0 everywhere
    in validation mode; the parameter gradients are NaN in every slot of that channel the num_layers chain uses, and in the
    other channels they equal the run without the NaN bit for bit (each channel has its own accumulators) -- as does
    grad_latent in every other element."""
    ops = _ops()
    rng = np.random.default_rng(nl * 10 + ld)
    lat = rng.uniform(-8, 8, (300, ld)).astype(np.float32)
    noise = None if mode == "validation" else rng.uniform(-0.5, 0.5, (300, ld)).astype(np.float32)
    params = (rng.standard_normal((4, 3, ld)) * 0.4).astype(np.float32)
    bad_lat, bad_noise = lat.copy(), None if noise is None else noise.copy()
    (bad_noise if mode == "noise" else bad_lat)[255, ld - 1] = np.nan
    t_tot, t_gl, t_gp = _torch_entropy(bad_lat, bad_noise, params, nl)
    used = np.zeros((4, 3, ld), bool)                                   # pinned: what torch makes NaN
    for k in list(range(nl - 1)) + [3]:
        used[k, :2 if k == 3 else 3, ld - 1] = True
    at = np.zeros((300, ld), bool)
    at[255, ld - 1] = mode != "validation"
    assert np.isnan(t_tot) and np.array_equal(np.isnan(t_gl), at) and np.array_equal(np.isnan(t_gp), used)
    if mode == "validation":
        assert not t_gl.any()
    gt = torch.ones((), device=dev)
    run = lambda l_, n_: (float(ops.entropy_bits_forward(_to(dev, l_), _to(dev, n_), _to(dev, params), nl)),) + tuple(
        x.cpu().numpy() for x in ops.entropy_bits_backward(_to(dev, l_), _to(dev, n_), _to(dev, params), nl, gt))
    c_tot, c_gl, c_gp = run(lat, noise)
    tot, gl, gp = run(bad_lat, bad_noise)
    assert np.isfinite(c_tot) and np.isfinite(c_gl).all() and np.isfinite(c_gp).all()
    assert np.isnan(tot), tot
    assert np.array_equal(np.isnan(gl), at) and np.array_equal(gl[~at], c_gl[~at])
    assert np.array_equal(np.isnan(gp), used), np.argwhere(np.isnan(gp) != used)
    assert np.array_equal(gp[~used], c_gp[~used])
