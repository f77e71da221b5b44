"""tests/latent_mlp_ref.py (the float64 restatement the GPU tests of latent_mlp.hip compare with) held to three things, on the
CPU: the executed reference module's vectors, float64 torch autograd of the module's own path, and -- in float32 -- which
outputs and gradients torch makes NaN, +-inf or finite for a NaN, an infinite and an overflowing latent. That last table IS
the policy test_gpu_latent_mlp_edges.py asserts of the kernel; nothing in it was decided by hand."""
import numpy as np
import pytest
import torch

import latent_mlp_ref as lr
from conftest import npz_json
from shacira_amd.wisp.models.latent_decoders.decode_layer import get_dft_matrix

EPS = lr.EPS
TINY = float(np.finfo(np.float32).tiny)


def _golden_case(g, ci, case):
    """-> (widths, packed params, per layer a function packed-layout gradient -> the module's (grad_scale, grad_shift))."""
    p = f"c{ci}_"
    layers, back = [], []
    for k in range(case["num_layers"]):
        scale = g[p + f"scale{k}"].astype(np.float64)
        if "dft" in case["ldecode_matrix"]:
            out = scale.shape[1]
            fan_in = case["latent_dim"] if k == 0 else layers[-1][0].shape[1]
            dft32 = get_dft_matrix(fan_in, out).numpy()
            W = (dft32 * g[p + f"scale{k}"]).astype(np.float64)               # the module's effective matrix, formed in float32
            dft = dft32.astype(np.float64)
            # grad_scale = sum_i dft_ij gW_ij, formed by the module in float32: fan_in products and sums more
            back.append((lambda gW, dft=dft: (dft * gW).sum(0, keepdims=True),
                         lambda tW, aW, dft=dft: (np.abs(dft) * (tW + (dft.shape[0] + 1) * EPS * aW)).sum(0, keepdims=True)))
        else:
            W = scale
            back.append((lambda gW: gW, lambda tW, aW: tW))
        b = g[p + f"shift{k}"].astype(np.float64).reshape(-1) if case["use_shift"] else np.zeros(W.shape[1])
        layers.append((W, b))
    widths = tuple([layers[0][0].shape[0]] + [W.shape[1] for W, _ in layers])
    return widths, lr.pack(layers), back


def test_restatement_against_the_reference_modules_vectors(golden):
    """All eight cases of latent_decoder_mlp.npz (vectors of the executed reference module, float32), forward and every
    gradient, to the restatement's own carried tolerance + EPS |ref| -- i.e. to what a float32 evaluation of these inputs may
    differ from float64 by, no more. The reduced gradients were summed over 700 rows in float32 by the module; their bar
    is the carried tolerance alone all the same (it holds >= 2 EPS of every term). A 'dft' layer's effective matrix
    dft * scale is formed as the module forms it, in float32, and its grad_scale = sum_i dft_ij gW_ij takes the roundings of that
    float32 sum on top (fan_in + 1 EPS of its absolute terms): the one operation of the module outside the restated function."""
    g = golden("latent_decoder_mlp.npz")
    for ci, case in enumerate(npz_json(g["cases_json"])):
        p = f"c{ci}_"
        widths, params, back = _golden_case(g, ci, case)
        uni = g[p + "uniforms"] if case["use_sga"] else None
        args = (g[p + "latent"], uni, case["temperature"], case["diff_sampling"], g[p + "div"], params, widths,
                case["activation"], case["final_activation"], case["clamp_weights"])
        bw = lr.backward(*args, g[p + "grad_out"])
        fw = bw["fw"]
        keep = lr.safe_rows(fw) & lr.off_the_clamp_edge(fw, case["clamp_weights"])
        assert (~keep).mean() <= lr.MAX_REJECTED, (ci, int((~keep).sum()))
        worst = {}

        def within(name, got, ref, tol):
            frac = np.abs(got - ref) / (tol + 1e-300)
            worst[name] = float(frac.max())
            assert (np.abs(got - ref) <= tol).all(), (ci, name, float(frac.max()))

        within("out", g[p + "out"][keep], fw["out"][keep], (fw["tol_y"] + EPS * np.abs(fw["out"]) + TINY)[keep])
        autograd = 0.0
        if case["use_sga"] and case["diff_sampling"]:
            # The vectors' OWN noise, not the kernel's: autograd differentiates q = wf s0 + wc s1 through exp(z - lse(z)) as
            # s_i (w_i g - sum_j w_j s_j g), a difference of two numbers of size |w| s_i |g| (three roundings), times
            # |dz_i / dw| <= 1 / T^2 -- absolute 3 EPS max|w| / T^2 where dq = s0 s1 (...) / T^2 itself may be 1e-6. The kernel and
            # the restatement form the product s0 s1 and have no such cancellation.
            wmax = np.abs(np.floor(g[p + "latent"].astype(np.float64))) + 1.0
            autograd = 3 * EPS * wmax / case["temperature"] ** 2 * bw["grad_x_abs"]
        within("grad_latent", g[p + "grad_latent"][keep], bw["grad_latent"][keep],
               (bw["grad_latent_tol"] + autograd + EPS * np.abs(bw["grad_latent"]) + TINY)[keep])
        # the reduced gradients, in every case: rows the filters reject stay in these sums (the vectors hold them), and the
        # bar takes no allowance for them
        gp, gt = lr.unpack(bw["grad_params"], widths), lr.unpack(bw["grad_params_tol"], widths)
        ga = lr.unpack(bw["grad_params_abs"], widths)
        for k, ((gW, gb), (tW, tb), (aW, _)) in enumerate(zip(gp, gt, ga)):
            ref = back[k][0](gW)
            within(f"grad_scale{k}", g[p + f"grad_scale{k}"], ref, back[k][1](tW, aW) + EPS * np.abs(ref) + TINY)
            if case["use_shift"]:
                within(f"grad_shift{k}", g[p + f"grad_shift{k}"].reshape(-1), gb, tb + EPS * np.abs(gb) + TINY)
        if case["use_sga"]:
            # the quantiser in float32, in the product form the kernels use, against the UN-widened tolerances
            q32, dq32 = lr.sga_f32(g[p + "latent"], uni, case["temperature"], case["diff_sampling"])
            q64, dq64 = lr.mr.quantise(g[p + "latent"], uni, case["temperature"], case["diff_sampling"])
            q_tol, dq_tol = lr.mr.sga_tolerances(g[p + "latent"], uni, case["temperature"], case["diff_sampling"])
            within("q (fp32 product form)", q32, q64, q_tol + TINY)
            within("dq (fp32 product form)", dq32, dq64, dq_tol + TINY)
        print(f"  case {ci} {widths} rejected {int((~keep).sum())}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


RANDOM = [((3, 5, 2), "tanh", "none", None, 0.0), ((2, 7, 3, 6), "sigmoid", "sine", None, 0.4),
          ((1, 3), "none", "relu", None, 0.0), ((5, 1, 5), "relu", "tanh", None, 0.3),
          ((2, 11, 13, 9, 3), "sine", "sigmoid", None, 0.0), ((2, 6, 3), "tanh", "none", True, 0.0),
          ((3, 5, 2), "relu", "none", False, 0.5)]


@pytest.mark.parametrize("widths,act,final_act,sga,clampw", RANDOM)
def test_restatement_against_float64_autograd_of_the_module(widths, act, final_act, sga, clampw):
    """torch autograd in float64 through the module's own layers (LatentDecoder on the CPU evaluates
    final_activation(layers(q / div)) with torch ops), random shapes with widths that are no power of two, rounding and SGA.
    Two float64 evaluations: 1e-11 of the absolute scale."""
    p = lr.make_inputs(len(widths) * 7 + widths[1], 301, widths, sga=sga is not None)
    if sga is not None:
        # fractional parts beyond 1 - 1e-6 (the -1e-9 tie row) are clamped at float32(1 - 1e-6) by the restatement and the
        # kernels, as float32 torch does, and at the float64 value by this float64 module: keep them out of THIS comparison
        p["latent"][:8, 0] += 0.25
    args = (p["latent"], p["uniforms"], 0.4, bool(sga), p["div"], p["params"], widths, act, final_act, clampw)
    bw = lr.backward(*args, p["grad_out"])
    out, gl, gp = lr.torch_eval(*args, p["grad_out"], torch.float64)
    fw = bw["fw"]
    assert np.abs(out - fw["out"]).max() <= 1e-11 * (1 + np.abs(fw["out"]).max())
    assert np.abs(gl - bw["grad_latent"]).max() <= 1e-11 * (1 + bw["grad_latent_abs"].max())
    assert (np.abs(gp - bw["grad_params"]) <= 1e-11 * (1 + bw["grad_params_abs"])).all()
    assert (fw["tol_y"] >= 0).all() and np.isfinite(bw["grad_params_tol"]).all() and (bw["grad_latent_tol"] >= 0).all()
    # the fp32 numpy evaluation stays inside the forward tolerance (rounding path)
    if sga is None:
        y32 = lr.forward_f32(p["latent"], p["div"], p["params"], widths, act, final_act)
        assert (np.abs(y32 - fw["y"]) <= fw["tol_y"] + TINY).all()


@pytest.mark.parametrize("widths", [(2, 5, 3), (2, 3, 2), (1, 2)])
@pytest.mark.parametrize("act", lr.ACTS)
def test_the_nan_and_inf_policy_is_torchs_own_in_float32(widths, act):
    """A NaN, a +-inf and an overflowing (+-3e38 / 0.5) latent, one row each and all five in one batch, each activation as
    the hidden and as the final one, with and without a clamp: the restatement makes exactly the outputs and gradients NaN,
    +inf, -inf or finite that CPU torch makes in float32 (and the finite ones agree to the carried tolerance). Notable rows of
    that table: tanh / sigmoid of an infinite pre-activation are finite with a zero derivative, so the row's grad_latent is
    an exact 0 but its term inf * 0 makes grad_W1[0, :] NaN; sine of it is NaN; relu keeps NaN and +inf; a clamped NaN stays NaN
    and its gradient is masked, a clamped +-inf is +-clamp_weights."""
    for final_act in ("none", act):
        for clamp_q in (None, 0.67):
            for bad in ([3], [4], [5], [6], [7], [0, 9, 19, 29, 39]):
                p, where = lr.policy_batch(11, 40, widths, bad)
                if clamp_q is not None:
                    p["clampw"] = lr.clamp_at_quantile(p, 1.0, False, act, final_act, clamp_q)
                args = (p["latent"], None, 1.0, False, p["div"], p["params"], widths, act, final_act, p["clampw"])
                bw = lr.backward(*args, p["grad_out"])
                out, gl, gp = lr.torch_eval(*args, p["grad_out"], torch.float32)
                tag = (widths, act, final_act, p["clampw"], where)
                assert np.array_equal(lr.nonfinite_class(out), lr.nonfinite_class(bw["fw"]["out"])), tag
                assert np.array_equal(lr.nonfinite_class(gl), lr.nonfinite_class(bw["grad_latent"])), tag
                assert np.array_equal(lr.nonfinite_class(gp), lr.nonfinite_class(bw["grad_params"])), tag
                ok = np.ones(40, bool)
                ok[list(where)] = False
                ok &= lr.safe_rows(bw["fw"]) & lr.off_the_clamp_edge(bw["fw"], p["clampw"])
                with np.errstate(invalid="ignore"):
                    assert (np.abs(out - bw["fw"]["out"]) <= bw["fw"]["tol_y"] + TINY)[ok].all(), tag
                    assert (np.abs(gl - bw["grad_latent"]) <= bw["grad_latent_tol"] + TINY)[ok].all(), tag
                assert lr.nonfinite_class(out[list(where)]).any() or act in ("tanh", "sigmoid") or p["clampw"] > 0, tag
