"""Fused decoder MLP (row a14) against the same MLP evaluated with torch Linear layers (what the reference runs)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from shacira_amd.wisp.models.decoders import BasicDecoder


def _torch_mlp(dec, x):
    h = x
    for lin in dec.layers:
        h = torch.relu(lin(h))
    return dec.lout(h)


def test_basic_decoder_host_logic_and_names():
    torch.manual_seed(0)
    dec = BasicDecoder(32, 3, torch.relu, True, nn.Linear, 2, 16, [])
    assert [n for n, _ in dec.named_parameters()] == ["layers.0.weight", "layers.0.bias", "layers.1.weight",
                                                       "layers.1.bias", "lout.weight", "lout.bias"]
    x = torch.randn(10, 32)
    torch.testing.assert_close(dec(x), _torch_mlp(dec, x))          # CPU: plain torch layers
    out, h = dec(x, return_h=True)
    assert h.shape == (10, 16)
    assert dec.packed_params().numel() == 32 * 16 + 16 + 16 * 16 + 16 + 3 * 16 + 3
    skip = BasicDecoder(8, 2, torch.relu, True, nn.Linear, 3, 16, [1])    # construction rule of the reference (:58-66)
    assert [l.in_features for l in skip.layers] == [8, 24, 16]


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(32, 16, 2, 3), (24, 16, 2, 3), (16, 16, 2, 3), (48, 16, 2, 3), (32, 16, 1, 3),
                                  (32, 16, 3, 3), (32, 16, 2, 4),
                                  # hidden width 64: the fp32-MFMA kernels (NeRF density / colour decoders)
                                  (32, 64, 1, 16), (43, 64, 2, 3), (32, 64, 2, 3), (16, 64, 2, 3), (32, 64, 1, 3),
                                  # hidden width 128 (nerf_lego.yaml): weight gradients split over the workgroup's waves
                                  (96, 128, 1, 16), (43, 128, 2, 3)])
@pytest.mark.parametrize("n", [1, 255, 256, 70_001])
@pytest.mark.parametrize("variant", [-1, 0])
def test_fused_mlp_matches_torch_layers(dims, n, variant):
    """variant -1: the MFMA kernels wherever a shape has one (16x16x4 for width 16, 32x32x2 for width 64), 0: the VALU
    kernels (width 16 only)."""
    from shacira_amd import _lib, hip_ops
    dev = torch.device("cuda:0")
    IN, H, NH, OUT = dims
    if variant == 0 and H != 16:
        pytest.skip("width-64 / width-128 decoders exist as MFMA kernels only")
    _lib.set_option("mlp_variant", variant)
    try:
        _check_fused_mlp(dims, n, dev)
    finally:
        _lib.set_option("mlp_variant", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(32, 64, 1, 16), (43, 64, 2, 3), (96, 128, 1, 16), (43, 128, 2, 3)])
@pytest.mark.parametrize("n", [409_600, 1 << 20])
def test_wide_decoders_at_nerf_batch_sizes(dims, n):
    """The NeRF decoders (width 64: nerf_hash.yaml, width 128: nerf_lego.yaml) at the batch sizes nerf_lego.yaml runs (4 096
    rays x 100 steps = 409 600 samples) and at 2^20, against the same layers in float64 with the same bad-row accounting as
    the small cases: a handful of samples per million take the other ReLU branch than the fp64 evaluation (that is what the
    1e-2..9e-2 "max rel grad diff" of profiles/r03_mlp_mfma_util.md was: tools/attic/mlp128_check.py compared with torch's fp32
    layers without dropping those rows); every other row and every weight gradient holds 1e-5."""
    _check_fused_mlp(dims, n, torch.device("cuda:0"))


def _check_fused_mlp(dims, n, dev):
    from shacira_amd import hip_ops
    IN, H, NH, OUT = dims
    assert hip_ops.mlp_supported(*dims)
    torch.manual_seed(IN + NH + n % 7)
    dec = BasicDecoder(IN, OUT, torch.relu, True, nn.Linear, NH, H, []).to(dev)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(3.0 if H < 64 else 1.5)                # enough dynamic range for the ReLUs to gate both ways
    dec64 = BasicDecoder(IN, OUT, torch.relu, True, nn.Linear, NH, H, []).to(dev).double()
    dec64.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})

    def both(x0, gy):
        dec.zero_grad(); dec64.zero_grad()
        x = x0.clone().requires_grad_(True)
        y = dec(x)                                        # fused path
        y.backward(gy)
        got = [x.grad.clone()] + [p.grad.clone() for p in dec.parameters()]
        x64 = x0.double().requires_grad_(True)            # reference: the same layers in float64, same parameters
        y64 = _torch_mlp(dec64, x64)
        y64.backward(gy.double())
        return y, y64, got, [x64.grad] + [p.grad for p in dec64.parameters()]

    x0 = torch.randn(n, IN, device=dev)
    gy = torch.randn(n, OUT, device=dev)
    y, y64, got, want = both(x0, gy)
    torch.testing.assert_close(y.double(), y64, rtol=1e-5, atol=1e-5)
    # A sample whose pre-activation sits within rounding of 0 may take the other ReLU branch than the fp64 evaluation
    # (its input-gradient row and its contribution to every weight gradient then differ): at most a couple per 100 k
    # samples; they are dropped and the comparison repeated without them.
    gx, gx64 = got[0].double(), want[0]
    bad_rows = ((gx - gx64).abs() > 1e-5 * gx64.abs() + 1e-5 * float(gx64.abs().max()) + 1e-9).any(dim=1)
    assert int(bad_rows.sum()) <= n // 30_000, int(bad_rows.sum())
    if bad_rows.any():
        y, y64, got, want = both(x0[~bad_rows], gy[~bad_rows])
    for a, b in zip(got, want):
        torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-5 * float(b.abs().max()) + 1e-9)
