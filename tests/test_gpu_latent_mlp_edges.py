"""latent_mlp.hip (the hidden-layer latent decoder, shacira_latent_mlp_forward / _backward) at its edges, against the float64
restatement tests/latent_mlp_ref.py: every instantiation (W = 4 / 8 / 16, rounding or SGA, each way) below, at and above the
grid cap of 512 workgroups, hidden widths that are not W, width-1 bottlenecks, each activation as the hidden and as the final
one, the clamp at 0 and at a value a third of the outputs exceed, tie / zero / clamp-bound / SGA-bound / saturation rows, the
NaN and inf policy of float32 torch, and the C-ABI's workspace contract.

Every element of every output is compared. Every bound comes from the restatement (EPS = 2^-23), none from the kernel:

  decoded      |got - ref| <= tol_y + TINY                      (tol_y: the forward tolerance carried layer by layer)
  grad_latent  |got - ref| <= grad_latent_tol + TINY            (the carried backward tolerance)
  grad_params  |got - ref| <= c EPS sum|term| + carried + EPS |ref| + TINY
               c = 1 (the fma that forms x * g and adds it) + 256 (the fp32 sum over a tile's rows in sw / sb)
                 + the tiles one workgroup adds in fp32 in accW / accB (1, or 2 above the cap); the block partials are fp64

Rows whose relu pre-activation or whose output lies within the restatement's own tolerance of the gate / the clamp bound
(latent_mlp_ref.safe_rows, .off_the_clamp_edge: they look at the reference only) keep their place in the batch with a zero
grad_out: their decoded values are still held (relu and the clamp are 1-Lipschitz), their grad_latent must be an exact 0.
Each test asserts, before it runs anything, that the filters take at most 5 % of the batch, and pins the count.
Each check prints its worst error as a fraction of its bound before it asserts; the worst per group is printed at the end.
"""
import ctypes

import numpy as np
import pytest
import torch

import latent_mlp_ref as lr
from oracle import latent as ol

pytestmark = pytest.mark.gpu
EPS = lr.EPS
TINY = float(np.finfo(np.float32).tiny)
CAP = 512                         # kLmlpMaxBlocks
B = CAP * 256                     # 131 072 rows fill the capped grid once
SMALL = [1, 255, 256, 257, 511]
AROUND = [B - 1, B, B + 1, B + 257]   # B + 1: one workgroup's second tile holds one live row; B + 257: one thread of the
                                       # forward adds two rows, and a second workgroup gets a second tile with one live row
ACTS = lr.ACTS
MULTI = {4: [(3, 4, 1), (4, 3, 4, 3, 4), (2, 3, 2)],                 # per W: a width-1 bottleneck / four layers / a hidden
         8: [(8, 1, 8), (2, 5, 8, 3), (2, 5, 3)],                    # width that is not W (all three in most of them)
         16: [(1, 2, 16), (3, 16, 9, 16, 2), (1, 16, 16, 16, 4)]}
SINGLE = {4: (1, 2), 8: (1, 8), 16: (16, 16)}
RATIOS = {}


def _configs():
    """Per W ten configurations: activation i as the hidden one of multi-layer shape i mod 3 with activation i + 1 as the final
    one, and activation i as the final one of the one-layer shape -- each activation is the hidden and the final one at each
    W. Odd ones run SGA (T and diff_sampling alternate), even ones rounding."""
    out = []
    for W in (4, 8, 16):
        for i, a in enumerate(ACTS):
            out.append((W, MULTI[W][i % 3], a, ACTS[(i + 1) % 5], i))
            out.append((W, SINGLE[W], "none", a, i + 1))
    return out


CONFIGS = _configs()
# by the configuration's last field. (T = 0.05, whose fp32 sample is only good to ~1e-3, does not meet the final sine: 30 times
# that tolerance would put more than 5 % of the rows within it of the clamp bound.)
SGA_OF = {0: None, 1: (0.05, True), 2: None, 3: (1.0, False), 4: None, 5: (0.4, True)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    print("\n  worst error / bound per group: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))


def _ops():
    from shacira_amd import hip_ops
    return hip_ops


def _to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _within(group, name, got, ref, tol, where=None):
    """|got - ref| <= tol on ``where`` (default: everywhere); prints the worst fraction of the bound first."""
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    assert got.shape == ref.shape == tol.shape, (name, got.shape, ref.shape, tol.shape)
    if where is not None:
        got, ref, tol = got[where], ref[where], tol[where]
    if got.size == 0:
        return
    assert np.isfinite(got).all() and np.isfinite(tol).all(), f"{name}: non-finite value or bound"
    frac = np.abs(got - ref) / (tol + 1e-300)
    worst = float(frac.max())
    RATIOS[group] = max(RATIOS.get(group, 0.0), worst)
    print(f"  {name}: worst error / bound = {worst:.3f}")
    assert (np.abs(got - ref) <= tol).all(), f"{name}: {worst:.3f} of the bound at flat index {int(frac.argmax())}"


def _tiles_per_workgroup(rows):
    tiles = max(1, -(-rows // 256))
    return -(-tiles // min(tiles, CAP))


def _prepare(p, T, diff, act, final_act, pinned=None, tag="", exact_clamp=False):
    """Filters (reference only), their 5 % cap, the pinned count; zeroes grad_out of the rejected rows; -> (bw, keep), the
    counts in bw["rejected"]. exact_clamp: the caller has proven that fp32 computes these outputs exactly, so none is on the
    wrong side of the clamp bound, and the clamp-edge filter is not applied."""
    fw = lr.forward(p["latent"], p["uniforms"], T, diff, p["div"], p["params"], p["widths"], act, final_act, p["clampw"])
    relu_ok, clamp_ok = lr.safe_rows(fw), lr.off_the_clamp_edge(fw, 0.0 if exact_clamp else p["clampw"])
    n = fw["y"].shape[0]
    counts = (int((~relu_ok).sum()), int((~clamp_ok).sum()))
    print(f"  {tag}: rejected rows (relu gate, clamp edge) = {counts} of {n}")
    assert counts[0] <= lr.MAX_REJECTED * n and counts[1] <= lr.MAX_REJECTED * n, (tag, counts, n)
    if pinned is not None:
        assert counts == tuple(pinned), (tag, counts, pinned)
    keep = relu_ok & clamp_ok
    p["grad_out"][~keep] = 0.0
    bw = lr.backward(p["latent"], p["uniforms"], T, diff, p["div"], p["params"], p["widths"], act, final_act, p["clampw"],
                     p["grad_out"])
    bw["rejected"] = counts
    return bw, keep


def _run(dev, p, T, diff, act, final_act):
    ops = _ops()
    t = [_to(dev, p[k]) for k in ("latent", "uniforms", "div", "params", "grad_out")]
    out = ops.latent_mlp_forward(t[0], t[1], T, diff, t[2], t[3], p["widths"], act, final_act, p["clampw"])
    gl, gp = ops.latent_mlp_backward(t[0], t[1], T, diff, t[2], t[3], p["widths"], act, final_act, p["clampw"], t[4])
    return [x.cpu().numpy().astype(np.float64) for x in (out, gl, gp)]


def _compare(group, tag, got, bw, keep, p, rows):
    out, gl, gp = got
    fw, c = bw["fw"], 1 + 256 + _tiles_per_workgroup(rows)
    _within(group, tag + " decoded", out, fw["out"], fw["tol_y"] + TINY)
    if p["clampw"] > 0:                                   # beyond the bound (by more than the tolerance): the bound itself
        over = (np.abs(fw["y"]) > p["clampw"]) & keep[:, None]
        assert np.array_equal(out[over], (np.sign(fw["y"]) * np.float32(p["clampw"]))[over]), tag
    _within(group, tag + " grad_latent", gl, bw["grad_latent"], bw["grad_latent_tol"] + TINY)
    dead = bw["grad_latent_abs"] == 0                      # every output masked by the clamp, every gate off, a rejected row
    assert not gl[dead].any(), f"{tag}: grad_latent is not an exact zero where nothing reaches the latent"
    _within(group, tag + " grad_params", gp, bw["grad_params"],
            c * EPS * bw["grad_params_abs"] + bw["grad_params_tol"] + EPS * np.abs(bw["grad_params"]) + TINY)


def _sine_note(tag, p, act, final_act, fw, T=1.0, diff=False):
    """What a plain fp32 numpy evaluation of the same inputs (rounding or SGA) uses of the forward bound; printed."""
    if "sine" in (act, final_act):
        y32 = lr.forward_f32(p["latent"], p["div"], p["params"], p["widths"], act, final_act, p["uniforms"], T, diff)
        frac = np.abs(y32 - fw["y"]) / (fw["tol_y"] + TINY)
        print(f"  {tag}: fp32 numpy restatement error / bound = {float(frac.max()):.3f}; largest bound "
              f"{float(fw['tol_y'].max()):.2e}")


def _take(p, n):
    q = {k: (v[:n].copy() if k in ("latent", "uniforms", "grad_out") and v is not None else v) for k, v in p.items()}
    return q


# ================================================================================================== a. shapes and row counts
# rejected rows (relu gate, clamp edge) of the ten batches (clamp off: 1 / 255 / 256 / 257 / 511 rows, then clamp on), per
# configuration: computed on the CPU from the inputs and the restatement alone
PINNED_SMALL = {(4, (1, 2), 'none', 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (1, 2), 'none', 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (1, 2), 'none', 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (1, 2), 'none', 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (1, 2), 'none', 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (2, 3, 2), 'tanh', 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (3, 4, 1), 'none', 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (3, 4, 1), 'relu', 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (4, 3, 4, 3, 4), 'sigmoid', 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (4, (4, 3, 4, 3, 4), 'sine', 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (1, 8), 'none', 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (1, 8), 'none', 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (1, 8), 'none', 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (1, 8), 'none', 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (1, 8), 'none', 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (2, 5, 3), 'tanh', 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (2, 5, 8, 3), 'sigmoid', 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (2, 5, 8, 3), 'sine', 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (8, 1, 8), 'none', 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (8, (8, 1, 8), 'relu', 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (16, (1, 2, 16), 'none', 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (16, (1, 2, 16), 'relu', 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (16, (1, 16, 16, 16, 4), 'tanh', 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (16, (3, 16, 9, 16, 2), 'sigmoid', 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 5), (0, 5), (0, 5),
                                              (0, 8)],
 (16, (3, 16, 9, 16, 2), 'sine', 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (16, (16, 16), 'none', 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 6), (0, 6), (0, 6), (0, 11)],
 (16, (16, 16), 'none', 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (2, 0), (0, 0), (0, 0), (0, 0), (0, 0), (2, 0)],
 (16, (16, 16), 'none', 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 (16, (16, 16), 'none', 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 1), (0, 1), (0, 1), (0, 1)],
 (16, (16, 16), 'none', 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)]}


@pytest.mark.parametrize("W,widths,act,final_act,kind", CONFIGS, ids=[f"W{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}"
                                                                       for c in CONFIGS])
def test_small_row_counts_in_every_shape(dev, W, widths, act, final_act, kind):
    """1 / 255 / 256 / 257 / 511 rows (one lane; a tile's last lane dead; a full tile; a second workgroup with one live row; two
    workgroups, the second partly dead -- never 512 partials: the finish kernel must read ``blocks`` of them, and the
    workspace the wrapper hands over is not cleared) in each of the thirty configurations, without a clamp and with one about
    a third of the outputs exceed. The batches of 16 rows and more carry the round-half ties +-0.5 / +-1.5 / +-2.5 and +-1e-9."""
    assert max(widths) <= W and (W == 4 or max(widths) > W // 2)
    sga = SGA_OF[kind]
    T, diff = sga if sga else (1.0, False)
    # a sine layer takes weights of the SIREN scale (30 z of a few radians), like the decoders that use it
    full = lr.make_inputs(100 * W + kind, 511, widths, sga=sga is not None, w_std=0.05 if "sine" in (act, final_act) else 0.5)
    assert np.array_equal(np.rint(full["latent"][:8, 0]), [0, -0.0, 2, -2, 2, -2, 0, -0.0])
    group = f"small W={W}"
    counts = []
    for clamp in (False, True):
        full["clampw"] = lr.clamp_at_quantile(full, T, diff, act, final_act) if clamp else 0.0
        for rows in SMALL:
            p = _take(full, rows)
            tag = f"{widths} {act}/{final_act} sga={sga} clamp={p['clampw']:.4g} rows={rows}"
            bw, keep = _prepare(p, T, diff, act, final_act, None, tag)
            counts.append(bw["rejected"])
            if clamp and rows == 511:
                share = float((np.abs(bw["fw"]["y"]) > p["clampw"]).mean())
                assert 0.25 < share < 0.42, share
            if rows == 511:
                _sine_note(tag, p, act, final_act, bw["fw"], T, diff)
            _compare(group, tag, _run(dev, p, T, diff, act, final_act), bw, keep, p, rows)
    assert counts == PINNED_SMALL[(W, widths, act, final_act)], counts


ABOVE = [(4, (4, 3, 4, 3, 4), "tanh", "relu", None), (4, (2, 3, 2), "relu", "sine", (0.4, True)),
         (8, (2, 5, 8, 3), "sigmoid", "tanh", None), (8, (2, 5, 3), "sine", "none", (1.0, False)),
         (16, (3, 16, 9, 16, 2), "relu", "sigmoid", None), (16, (1, 16, 16, 16, 4), "tanh", "none", (0.4, True))]
# rejected rows (relu gate, clamp edge) of the four row counts, per entry of ABOVE: CPU, inputs and restatement alone
PINNED_ABOVE = {(4, False): [(116, 0), (116, 0), (116, 0), (116, 0)],
 (4, True): [(118, 0), (118, 0), (118, 0), (118, 0)],
 (8, False): [(0, 0), (0, 0), (0, 0), (0, 0)],
 (8, True): [(0, 0), (0, 0), (0, 0), (0, 0)],
 (16, False): [(1081, 0), (1081, 0), (1081, 0), (1083, 0)],
 (16, True): [(0, 0), (0, 0), (0, 0), (0, 0)]}


@pytest.mark.parametrize("W,widths,act,final_act,sga", ABOVE, ids=[f"W{c[0]}-{'sga' if c[4] else 'round'}" for c in ABOVE])
def test_around_the_grid_cap_in_every_instantiation(dev, W, widths, act, final_act, sga):
    """B - 1, B, B + 1 and B + 257 rows (B = 512 * 256) in one rounding and one SGA shape per W: all six forward and all six
    backward instantiations at and above the cap, where a workgroup walks a second tile and adds it in fp32 (c grows by one).
    The clamp is on (a third of the outputs exceed it) in the rounding shapes."""
    T, diff = sga if sga else (1.0, False)
    full = lr.make_inputs(7 * W + (1 if sga else 0), B + 257, widths, sga=sga is not None, w_std=0.05 if "sine" in (act, final_act) else 0.5)
    if not sga:
        full["clampw"] = lr.clamp_at_quantile(full, T, diff, act, final_act)
    assert _tiles_per_workgroup(B) == 1 and _tiles_per_workgroup(B + 1) == 2
    for n, rows in enumerate(AROUND):
        p = _take(full, rows)
        tag = f"{widths} {act}/{final_act} sga={sga} rows={rows}"
        bw, keep = _prepare(p, T, diff, act, final_act, PINNED_ABOVE[(W, sga is not None)][n], tag)
        if rows == B + 257:
            _sine_note(tag, p, act, final_act, bw["fw"], T, diff)
        _compare(f"cap W={W} {'sga' if sga else 'round'}", tag, _run(dev, p, T, diff, act, final_act), bw, keep, p, rows)


@pytest.mark.parametrize("widths,final_act,sga", [((4, 3, 4, 3, 4), "none", None), ((2, 5, 3), "none", (0.4, True)),
                                                  ((3, 16, 2), "none", None), ((1, 8), "sine", (1.0, False))])
def test_sine_at_the_ordinary_weight_scale_without_a_clamp(dev, widths, final_act, sga):
    """sine as the hidden activation (and as the final one) with weights of std 0.5 / sqrt(fan_in), the scale of every other
    activation here, 511 rows, no clamp and no relu: neither filter applies, so nothing caps the bound. Every sine layer
    multiplies it by ~30 |W|: ~1e-4 after one hidden layer, 9e-2 after the three of (4, 3, 4, 3, 4) (of outputs of size 0.5:
    loose, honest, and it stays; deeper or doubly-sine shapes would reach the size of the output itself and hold nothing). The
    fp32 numpy evaluation's share of the bound is printed beside the kernel's."""
    T, diff = sga if sga else (1.0, False)
    p = lr.make_inputs(61 + len(widths), 511, widths, sga=sga is not None)
    tag = f"{widths} sine/{final_act} sga={sga} std 0.5"
    bw, keep = _prepare(p, T, diff, "sine", final_act, (0, 0), tag)
    _sine_note(tag, p, "sine", final_act, bw["fw"], T, diff)
    _compare("sine std 0.5", tag, _run(dev, p, T, diff, "sine", final_act), bw, keep, p, 511)


# rejected rows (relu gate, clamp edge) of golden cases 6 and 7: CPU, inputs and restatement alone
PINNED_GOLDEN = {6: (4, 0), 7: (0, 0)}


@pytest.mark.parametrize("ci", [6, 7])
def test_the_sga_reference_vectors_inputs_against_the_restatement(dev, golden, ci):
    """The inputs of the two SGA cases of latent_decoder_mlp.npz (6: diff_sampling, T = 0.4, relu, (2, 8, 8, 2); 7: T = 0.7,
    tanh, (1, 8, 2)) through the kernel, against the restatement with its own carried bounds and nothing on top. The CPU
    comparison of the restatement with those vectors' grad_latent needs an allowance for the cancellation in float32
    autograd of the sampler (test_latent_mlp_ref_cpu.py); the kernel, which forms the product s0 s1, needs none."""
    from conftest import npz_json
    from test_latent_mlp_ref_cpu import _golden_case
    g = golden("latent_decoder_mlp.npz")
    case = npz_json(g["cases_json"])[ci]
    assert case["use_sga"] and case["clamp_weights"] == 0.0
    pre = f"c{ci}_"
    widths, params, _ = _golden_case(g, ci, case)
    p = dict(latent=g[pre + "latent"].copy(), uniforms=g[pre + "uniforms"].copy(), div=g[pre + "div"].copy(),
             params=params.astype(np.float32), grad_out=g[pre + "grad_out"].copy(), widths=widths, clampw=0.0)
    assert np.array_equal(p["params"].astype(np.float64), params)
    T, diff, act, fin = case["temperature"], case["diff_sampling"], case["activation"], case["final_activation"]
    bw, keep = _prepare(p, T, diff, act, fin, PINNED_GOLDEN[ci], f"golden case {ci}")
    _compare("golden sga inputs", f"golden case {ci}", _run(dev, p, T, diff, act, fin), bw, keep, p, 700)


# ============================================================================================================== b. edge rows
def test_relu_pre_activations_of_exactly_zero(dev):
    """Zero latents (and +-0.4, which round to +-0) with zero biases, relu as the hidden and the final activation, widths
    (2, 5, 3): every pre-activation of those rows is an exact 0 in fp32 and fp64 alike -- forward 0, gates off, grad_latent an
    exact 0, and the rows add nothing to any parameter gradient (the other 300 rows do). Then three of those rows get a NaN, a
    +inf and a -inf grad_out."""
    widths = (2, 5, 3)
    p = lr.make_inputs(5, 320, widths)
    layers = [(W, np.zeros_like(b)) for W, b in lr.unpack(p["params"], widths)]
    p["params"] = lr.pack(layers).astype(np.float32)
    zero = np.arange(320) % 16 == 9
    p["latent"][zero] = np.resize(np.array([0.0, -0.0, 0.4, -0.4], np.float32), (int(zero.sum()), 2))
    bw, keep = _prepare(p, 1.0, False, "relu", "relu", (0, 0), "relu zeros")
    fw = bw["fw"]
    assert all((z[zero] == 0).all() for z in fw["zs"]) and keep[zero].all() and (bw["grad_latent_abs"][zero] == 0).all()
    got = _run(dev, p, 1.0, False, "relu", "relu")
    _compare("edge rows", "relu zeros", got, bw, keep, p, 320)
    assert not got[0][zero].any() and not got[1][zero].any()
    # the gate is a SELECT: under a NaN or infinite upstream gradient those rows (every unit off) still give an exact 0 to
    # grad_latent and add nothing to the gradients below the gate -- torch's relu backward, evaluated here in float32 on the
    # CPU; a product with a 0 / 1 mask would give NaN. Final relu: the final gate stops it, everything stays finite. Final none:
    # the second layer's own gradients take the NaN (b2 += NaN, W2 += 0 * NaN), as torch's do, the first layer's stay finite.
    bad = np.nonzero(zero)[0][:3]
    p["grad_out"][bad[0]], p["grad_out"][bad[1], 0], p["grad_out"][bad[2], 1] = np.nan, np.inf, -np.inf
    ok = np.ones(320, bool)
    ok[bad] = False
    for fin in ("relu", "none"):
        args = (p["latent"], None, 1.0, False, p["div"], p["params"], widths, "relu", fin, 0.0, p["grad_out"])
        _, t_gl, t_gp = lr.torch_eval(*args, torch.float32)
        assert not t_gl[bad].any() and np.isfinite(t_gl).all() and np.isfinite(t_gp[:15]).all()
        assert np.isnan(t_gp[15:]).all() if fin == "none" else np.isfinite(t_gp).all()
        ref = lr.backward(*args)
        assert lr.safe_rows(ref["fw"]).all()
        _, gl, gp = _run(dev, p, 1.0, False, "relu", fin)
        assert np.array_equal(lr.nonfinite_class(gl), lr.nonfinite_class(t_gl)) and not gl[bad].any(), fin
        assert np.array_equal(lr.nonfinite_class(gp), lr.nonfinite_class(t_gp)), (fin, lr.nonfinite_class(gp))
        _within("edge rows", f"relu zeros, non-finite grad_out, final {fin}: grad_latent", gl, ref["grad_latent"],
                ref["grad_latent_tol"] + TINY, ok)


def test_outputs_that_equal_the_clamp_bound(dev):
    """One layer, no activation, power-of-two weights and div, integer latents: y = (q0 / 2) / 2 + 1/4 and -q1 / 4 + 1/4 are
    exact in fp32 and fp64, and equal +-clamp_weights = +-0.75 for q0 = 2, -4 and q1 = -2, 4. The interval is closed: those
    outputs keep their gradient (a mask written with < would zero it); outputs beyond it lose theirs."""
    widths = (2, 2)
    p = lr.make_inputs(6, 600, widths)
    p["latent"] = np.random.default_rng(6).integers(-6, 7, (600, 2)).astype(np.float32)
    p["div"] = np.array([2.0, 1.0], np.float32)
    p["params"] = np.array([0.5, 0.0, 0.0, -0.25, 0.25, 0.25], np.float32)
    p["clampw"] = 0.75
    # proven here: a float32 evaluation, rounding after every product and sum, gives these outputs exactly
    y32 = lr.forward_f32(p["latent"], p["div"], p["params"], widths, "none", "none")
    bw, keep = _prepare(p, 1.0, False, "none", "none", (0, 0), "clamp bound", exact_clamp=True)
    y = bw["fw"]["y"]
    assert np.array_equal(y32, y)
    on = np.abs(y) == 0.75
    assert on[:, 0].sum() > 20 and on[:, 1].sum() > 20 and (np.abs(y) > 0.75).sum() > 100 and keep.all()
    got = _run(dev, p, 1.0, False, "none", "none")
    _compare("edge rows", "clamp bound", got, bw, keep, p, 600)
    assert np.array_equal(got[0], bw["fw"]["out"])
    g = p["grad_out"].astype(np.float64)
    want = np.where(np.abs(y) <= 0.75, g, 0.0) * np.array([0.5 / 2.0, -0.25])
    assert np.array_equal(got[1], want) and (got[1][on] != 0).all()


@pytest.mark.parametrize("T", [0.05, 0.4, 1.0])
@pytest.mark.parametrize("diff", [True, False])
def test_sga_bound_rows_and_uniform_edges(dev, diff, T):
    """The shared quantiser through this kernel, widths (1, 1) with W = 1, b = 0, div = 1 (decoded = q, grad_latent = g dq):
    fractional parts 0, lim = float32(1 - 1e-6) and its two fp32 neighbours, on either side of an integer, +-0.5, each with
    uniforms 0, 1, their fp32 neighbours and 0.5 in either slot, appended to 300 random rows. At lim the derivative is the
    closed-mask value of oracle.latent.sga_quantise (torch.clamp hands the gradient on at its bound); one ulp beyond it the
    far neighbour's term is gone. Tolerances: latent_multi_ref.sga_tolerances, as everywhere."""
    f = np.float32
    lim = f(1.0 - 1e-6)
    fracs = [f(0.0), f(0.5), lim, np.nextafter(lim, f(0)), np.nextafter(lim, f(1))]
    edge_w = [f(b) + fr for b in (0.0, -3.0, 2.0) for fr in fracs] + [-lim, -np.nextafter(lim, f(0)), -np.nextafter(lim, f(1))]
    edge_u = [f(0.0), f(1.0), f(EPS), f(1.0) - f(EPS / 2), np.nextafter(f(0), f(1)), f(0.5)]
    cases = [(w, u0, u1) for w in edge_w for u0 in edge_u for u1 in edge_u]
    p = lr.make_inputs(17, 300 + len(cases), (1, 1), sga=True)
    p["latent"][300:, 0] = [c[0] for c in cases]
    p["uniforms"][300:, 0, 0], p["uniforms"][300:, 0, 1] = [c[1] for c in cases], [c[2] for c in cases]
    p["div"], p["params"] = np.ones(1, f), np.array([1.0, 0.0], f)
    lat = p["latent"][:, 0].astype(np.float64)
    a, b = lat - np.floor(lat), np.floor(lat) + 1 - lat
    # proven on the CPU: w = lim and w = -lim have a distance that IS the bound (2 + lim and -3 + lim round away from it)
    at, beyond = (a == lim) | (b == lim), (a > lim) | (b > lim)
    assert at[300:].sum() == 2 * 36 and beyond[300:].sum() >= 5 * 36 and (a[300:] == 0).sum() == 3 * 36
    _, dq = ol.sga_quantise(p["latent"], p["uniforms"], T, diff)
    if diff:                                                  # the closed mask keeps the bound's own term: both terms count
        s0, s1 = lr.mr.sga_weights(p["latent"], p["uniforms"], T)
        both = s0 * s1 * ((1 - np.tanh(np.minimum(a, lim)[:, None]) ** 2) + (1 - np.tanh(np.minimum(b, lim)[:, None]) ** 2)) / T ** 2
        assert np.allclose(dq[at], both[at], rtol=1e-12, atol=0) and (dq[at] > 0).all()
    bw, keep = _prepare(p, T, diff, "none", "none", (0, 0), f"sga T={T} diff={diff}")
    assert np.array_equal(bw["fw"]["dq"], dq)
    _compare("edge rows", f"sga T={T} diff={diff}", _run(dev, p, T, diff, "none", "none"), bw, keep, p, p["latent"].shape[0])


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_saturated_sigmoid_and_tanh(dev, act):
    """Pre-activations of exactly +-0, +-20 and +-90 (expf(90) overflows float32: 1 / (1 + inf) must be 0, not NaN), as the
    final activation of (1, 1) and as the hidden one of (1, 1, 1), W = 1, b = 0, div = 1, among 256 random rows."""
    f = np.float32
    for widths, a, fa, prm in (((1, 1), "none", act, [1.0, 0.0]), ((1, 1, 1), act, "none", [1.0, 0.0, 0.5, 0.25])):
        p = lr.make_inputs(23, 262, widths)
        p["latent"][256:, 0] = [0.0, -0.0, 20.0, -20.0, 90.0, -90.0]
        p["div"], p["params"] = np.ones(1, f), np.array(prm, f)
        bw, keep = _prepare(p, 1.0, False, a, fa, (0, 0), f"saturated {act} {widths}")
        assert np.array_equal(bw["fw"]["zs"][0][256:, 0], [0.0, -0.0, 20.0, -20.0, 90.0, -90.0])
        got = _run(dev, p, 1.0, False, a, fa)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        _compare("edge rows", f"saturated {act} {widths}", got, bw, keep, p, 262)


POLICY_ROWS = [0, 255, 699]          # row 0, a tile's last lane, the last live row (700 rows: three tiles, the third partly dead)


@pytest.mark.parametrize("widths", [(2, 5, 3), (2, 3, 2)])
@pytest.mark.parametrize("act", ACTS)
def test_nan_inf_and_overflowing_latents_follow_float32_torch(dev, widths, act):
    """A NaN, a +inf, a -inf and an overflowing latent (+-3e38 with div 0.5), each in turn at rows 0, 255 and 699 of 700, with
    ``act`` as the hidden activation (final none) and as the final one (hidden tanh), hidden widths 5 (W = 8) and 3 (W = 4) so
    that padded lanes exist, with and without a clamp. The policy is float32 torch's, evaluated here on the same batch on the
    CPU (and pinned against the restatement by test_latent_mlp_ref_cpu.py): decoded, grad_latent and grad_params are NaN,
    +inf, -inf or finite exactly where torch's are. Every other row's decoded and grad_latent meet their bounds, and so do the
    parameter gradients the bad rows leave finite. (On the parent commit this failed three ways: a clamped NaN row decoded
    to -clamp_weights; relu turned a NaN into 0; and an infinite x = q / div made every padded lane NaN = fma(inf, 0, b), which
    the next layer's zero rows kept, so tanh / sigmoid rows decoded to NaN where torch gives tanh(+-inf) = +-1.)"""
    counts = []
    for hid, fin in ((act, "none"), ("tanh", act)):
        for name in lr.POLICY_LATENTS:
            for clamp in (False, True):
                p, where = lr.policy_batch(31, 700, widths, POLICY_ROWS, names=[name])
                if clamp:
                    p["clampw"] = lr.clamp_at_quantile(p, 1.0, False, hid, fin)
                tag = f"{widths} {hid}/{fin} {name} clamp={p['clampw']:.3g}"
                bw, keep = _prepare(p, 1.0, False, hid, fin, None, tag)
                counts.append(bw["rejected"])
                args = (p["latent"], None, 1.0, False, p["div"], p["params"], widths, hid, fin, p["clampw"], p["grad_out"])
                t_out, t_gl, t_gp = lr.torch_eval(*args, torch.float32)
                out, gl, gp = _run(dev, p, 1.0, False, hid, fin)
                for what, got, want in (("decoded", out, t_out), ("grad_latent", gl, t_gl), ("grad_params", gp, t_gp)):
                    cg, cw = lr.nonfinite_class(got), lr.nonfinite_class(want)
                    assert np.array_equal(cg, cw), (f"{tag}: {what} is (0 finite, 1 NaN, 2 +inf, 3 -inf) "
                                                    f"{cg[cg != cw][:8]} where torch is {cw[cg != cw][:8]}")
                good = np.ones(700, bool)
                good[list(where)] = False
                fw = bw["fw"]
                _within("policy", tag + " decoded", out, fw["out"], fw["tol_y"] + TINY, good)
                _within("policy", tag + " grad_latent", gl, bw["grad_latent"], bw["grad_latent_tol"] + TINY, good)
                fin_p = lr.nonfinite_class(t_gp) == 0
                tol = (1 + 256 + 1) * EPS * bw["grad_params_abs"] + bw["grad_params_tol"] + EPS * np.abs(bw["grad_params"]) + TINY
                _within("policy", tag + " grad_params", gp, bw["grad_params"], tol, fin_p & np.isfinite(tol))
    assert counts == PINNED_POLICY[(widths, act)], counts


# rejected rows (relu gate, clamp edge) of the twenty batches of each policy case, in the order they run: CPU, inputs and
# restatement alone
PINNED_POLICY = {((2, 3, 2), 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 3, 2), 'relu'): [(0, 0), (0, 0), (0, 0), (0, 3), (0, 0), (0, 0), (0, 0), (0, 3), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 3, 2), 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                          (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 3, 2), 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 3, 2), 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 5, 3), 'none'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 5, 3), 'relu'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 5, 3), 'sigmoid'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                          (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 5, 3), 'sine'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
 ((2, 5, 3), 'tanh'): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
                       (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)]}


# ================================================================================================== c. through the C-ABI
def _abi_call(dev, p, act, final_act, rows, ws, ws_bytes, want_latent=True, fill=None):
    """shacira_latent_mlp_backward on the first ``rows`` rows with the caller's workspace tensor; outputs pre-filled."""
    from shacira_amd import _lib
    ops = _ops()
    widths = p["widths"]
    wa = (ctypes.c_int32 * len(widths))(*widths)
    t = {k: _to(dev, p[k]) for k in ("latent", "div", "params", "grad_out")}
    gl = torch.full((max(rows, 1), widths[0]), 7.0 if fill is None else fill, device=dev)
    gp = torch.full((lr.num_params(widths),), 7.0 if fill is None else fill, device=dev)
    rc = _lib.lib().shacira_latent_mlp_backward(
        rows, len(widths) - 1, wa, ops._ptr(t["latent"]), None, 1.0, 0, ops._ptr(t["div"]), ops._ptr(t["params"]),
        ops.LATENT_ACTIVATIONS[act], ops.LATENT_ACTIVATIONS[final_act], float(p["clampw"]), ops._ptr(t["grad_out"]),
        ops._ptr(gl) if want_latent else None, ops._ptr(gp), ops._ptr(ws), ws_bytes, ops._stream(t["latent"]))
    torch.cuda.synchronize()
    return rc, gl.cpu().numpy(), gp.cpu().numpy()


@pytest.mark.parametrize("rows", [257, B + 1])
def test_a_dirty_workspace_of_the_exact_size(dev, rows):
    """A workspace of exactly shacira_latent_mlp_backward_workspace_bytes() + 256 guard bytes, all 0xFF (NaN as doubles), at 257
    rows (2 of the 512 block partials are written: the finish kernel must read those two) and at B + 1: the results equal, bit
    for bit, those of a zeroed workspace; the guard bytes are untouched; grad_latent = NULL gives the same grad_params bits;
    a second call gives identical bits."""
    from shacira_amd import _lib
    widths, act, fin = (2, 5, 8, 3), "tanh", "sigmoid"
    p = lr.make_inputs(41, rows, widths)
    wa = (ctypes.c_int32 * len(widths))(*widths)
    n = _lib.lib().shacira_latent_mlp_backward_workspace_bytes(len(widths) - 1, wa)
    assert n == CAP * lr.num_params(widths) * 8
    dirty = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device=dev)
    clean = torch.zeros((n + 256,), dtype=torch.uint8, device=dev)
    rc0, gl0, gp0 = _abi_call(dev, p, act, fin, rows, clean, n)
    rc1, gl1, gp1 = _abi_call(dev, p, act, fin, rows, dirty, n)
    assert rc0 == 0 and rc1 == 0 and np.isfinite(gp0).all() and np.isfinite(gl0).all()
    assert np.array_equal(gp0, gp1) and np.array_equal(gl0, gl1)
    assert bool((dirty[n:] == 0xFF).all()) and bool((clean[n:] == 0).all())
    rc2, gl2, gp2 = _abi_call(dev, p, act, fin, rows, dirty, n, want_latent=False)
    assert rc2 == 0 and np.array_equal(gp2, gp0) and (gl2 == 7.0).all()
    rc3, gl3, gp3 = _abi_call(dev, p, act, fin, rows, dirty, n)
    assert rc3 == 0 and np.array_equal(gp3, gp0) and np.array_equal(gl3, gl0)
    bw = lr.backward(p["latent"], None, 1.0, False, p["div"], p["params"], widths, act, fin, 0.0, p["grad_out"])
    _within("abi", f"rows={rows} grad_params", gp0, bw["grad_params"], (257 + _tiles_per_workgroup(rows)) * EPS
            * bw["grad_params_abs"] + bw["grad_params_tol"] + EPS * np.abs(bw["grad_params"]) + TINY)


def test_no_rows_and_a_workspace_one_byte_short(dev):
    """num_rows = 0: grad_params is exactly zero and decoded is untouched. A workspace one byte short: SHACIRA_EWORKSPACE, and
    nothing ran (the pre-filled outputs keep their values)."""
    from shacira_amd import _lib
    ops = _ops()
    widths, act, fin = (3, 4, 1), "relu", "none"
    p = lr.make_inputs(43, 300, widths)
    wa = (ctypes.c_int32 * len(widths))(*widths)
    n = _lib.lib().shacira_latent_mlp_backward_workspace_bytes(len(widths) - 1, wa)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    rc, gl, gp = _abi_call(dev, p, act, fin, 0, ws, n)
    assert rc == 0 and not gp.any() and (gl == 7.0).all()
    t = {k: _to(dev, p[k]) for k in ("latent", "div", "params")}
    dec = torch.full((300, 1), 7.0, device=dev)
    rc = _lib.lib().shacira_latent_mlp_forward(0, len(widths) - 1, wa, ops._ptr(t["latent"]), None, 1.0, 0, ops._ptr(t["div"]),
                                               ops._ptr(t["params"]), 3, 0, 0.0, ops._ptr(dec), ops._stream(dec))
    torch.cuda.synchronize()
    assert rc == 0 and bool((dec == 7.0).all())
    rc, gl, gp = _abi_call(dev, p, act, fin, 300, ws, n - 1)
    assert rc == _lib.EWORKSPACE and (gl == 7.0).all() and (gp == 7.0).all()
    rc, gl, gp = _abi_call(dev, p, act, fin, 300, ws, n)
    assert rc == 0 and np.isfinite(gp).all() and not (gp == 7.0).all()


def test_whole_equals_head_plus_tail_above_the_cap(dev):
    """grad_params of B + 257 rows against the float64 sum of the kernel's own results on rows [0, B) and [B, B + 257): the same
    rows in the same lanes, so the only differences are the one fp32 addition accW / accB make in the two workgroups that
    walk a second tile (EPS of the absolute terms of their rows: tiles 0, 1, 512 and 513) and the rounding of the three fp32
    results. A second tile lost, or a finish kernel reading partials it should not, is off by the tail's own sum."""
    widths, act, fin = (3, 16, 9, 16, 2), "tanh", "none"
    p = lr.make_inputs(47, B + 257, widths)
    ops = _ops()
    t = {k: _to(dev, p[k]) for k in ("latent", "div", "params", "grad_out")}
    run = lambda lo, hi: ops.latent_mlp_backward(t["latent"][lo:hi].contiguous(), None, 1.0, False, t["div"], t["params"], widths,
                                                 act, fin, 0.0, t["grad_out"][lo:hi].contiguous())[1].cpu().numpy().astype(np.float64)
    whole, head, tail = run(0, B + 257), run(0, B), run(B, B + 257)
    pair = np.r_[0:512, B:B + 257]
    sub = lr.backward(p["latent"][pair], None, 1.0, False, p["div"], p["params"], widths, act, fin, 0.0, p["grad_out"][pair])
    tol = EPS * sub["grad_params_abs"] + EPS * (np.abs(whole) + np.abs(head) + np.abs(tail)) + TINY
    _within("abi", "whole - (head + tail)", whole, head + tail, tol)
    assert (np.abs(tail) > 10 * tol).mean() > 0.9             # the tail is far above that bound
