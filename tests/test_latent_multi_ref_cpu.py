"""Pins tests/latent_multi_ref.py (the fp64 restatement of the selector decoder) to the vectors of the reference's executed
MultiLatentDecoder (tests/golden/multi_decoder.npz, all four cases), at the tolerances the GPU test of the fused kernel
(test_fused_multi_decoder_against_reference_vectors) uses against the same vectors."""
import numpy as np
import pytest

import latent_multi_ref as mr
from conftest import npz_json


@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_restatement_reproduces_the_reference_run(golden, ci):
    g = golden("multi_decoder.npz")
    case = npz_json(g["cases_json"])[ci]
    p = f"m{ci}_"
    dft = g[p + "p_layers.0.dft"] if "dft" in case["ldecode_matrix"] else None
    shift = g[p + "p_layers.0.use_shift"] if case["use_shift"] else None
    args = (g[p + "latent"], g[p + "p_alpha"], None, 0.7, case["straight_through"], False, g[p + "p_div"],
            g[p + "p_layers.0.scale"], dft, shift, 0.0)
    assert g[p + "p_layers.0.scale"].shape[1] == (1 if dft is not None else case["latent_dim"])
    fw = mr.forward(*args)
    np.testing.assert_allclose(fw["out"].astype(np.float32), g[p + "out"], rtol=1e-5, atol=1e-7)
    bw = mr.backward(*args, g[p + "grad_out"])
    np.testing.assert_allclose(bw["grad_latent"].astype(np.float32), g[p + "grad_latent"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(bw["grad_alpha"].astype(np.float32), g[p + "g_alpha"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(bw["grad_scale"].astype(np.float32), g[p + "g_layers.0.scale"], rtol=1e-4, atol=1e-6)
    if case["use_shift"]:
        np.testing.assert_allclose(bw["grad_shift"].astype(np.float32).reshape(g[p + "g_layers.0.use_shift"].shape),
                                   g[p + "g_layers.0.use_shift"], rtol=1e-4, atol=1e-6)
    # the absolute counterparts dominate the values they belong to
    for k in ("grad_latent", "grad_alpha", "grad_scale", "grad_shift"):
        assert (bw[k + "_abs"] >= np.abs(bw[k]) * (1 - 1e-12)).all(), k
    assert (fw["y_abs"] >= np.abs(fw["y"]) * (1 - 1e-12)).all()


def test_first_maximum_wins_a_tie():
    alpha = np.array([[1.0, 0.0], [1.0, 2.0], [0.5, 2.0]], np.float32)        # column 0: k=0 and 1 tie; column 1: k=1 and 2
    _, a = mr.selector(alpha, 0.7, True)
    assert a.T.tolist() == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
