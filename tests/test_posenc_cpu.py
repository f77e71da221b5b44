"""Positional-encoding rows and ``wisp.models.nefs.NeuralImage`` without a GPU: the fp64 oracle (tests/posenc_ref.py) and the
mirror's torch composite against a recorded run of the reference's PositionalEmbedder (tests/golden/positional_embedder.npz,
written by tests/golden/make_posenc_golden.py), the argument checks of the three C entry points (they precede any HIP call), and
the module surface of NeuralImage with the grid operator swapped for the C oracle (test-only, as tests/test_harness.py does)."""
import ctypes
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import posenc_ref as R
from oracle import hashgrid_c as oc
from shacira_amd import _lib, codec, harness, hip_ops
from shacira_amd.wisp.models.activations import get_activation_class
from shacira_amd.wisp.models.embedders import PositionalEmbedder, get_positional_embedder
from shacira_amd.wisp.models.nefs import NeuralImage

CASES = ("d2_f4_in", "d2_f4_noin", "d3_f10", "d3_f5_lin")


def _case(golden, name):
    g = golden("positional_embedder.npz")
    d, F, inc, log = (int(v) for v in g[f"{name}.args"])
    return d, F, bool(inc), bool(log), g[f"{name}.coords"], g[f"{name}.bands"], g[f"{name}.out"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def oracle_op(monkeypatch):
    def fwd(coords, codebook, first_idx, resolution, bw):
        return torch.from_numpy(oc.forward(coords.detach().numpy(), codebook.detach().numpy(), first_idx.numpy(),
                                           list(resolution), bw))

    monkeypatch.setattr(hip_ops, "hashgrid_interpolate2d_cuda", fwd)


# ---- oracle and composite against the reference's recorded outputs -----------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_within_one_ulp(golden, name):
    d, F, inc, _, coords, bands, want = _case(golden, name)
    got = R.forward(coords, bands, inc)
    assert got.shape == want.shape == (coords.shape[0], R.widths(d, F, inc)[1])
    assert np.all(np.abs(got - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    if inc:
        assert np.array_equal(_bits(got[:, :d]), _bits(coords))


@pytest.mark.parametrize("name", CASES)
def test_composite_reproduces_the_reference_bit_for_bit(golden, name):
    d, F, inc, log, coords, bands, want = _case(golden, name)
    for fused in (False, True):        # fused=True on CPU tensors is the composite
        emb = PositionalEmbedder(F, F - 1, log_sampling=log, include_input=inc, input_dim=d, fused=fused)
        assert np.array_equal(emb.bands.numpy(), bands) and emb.out_dim == want.shape[1]
        assert list(emb.state_dict().keys()) == ["bands"]
        got = emb(torch.from_numpy(coords)).numpy()
        assert np.array_equal(_bits(got), _bits(want)), (name, fused)


def test_fused_flag_leaves_cpu_and_fp64_on_the_composite():
    torch.manual_seed(0)
    x = torch.rand(17, 3) * 2 - 1
    plain, _ = get_positional_embedder(5)
    fused, dim = get_positional_embedder(5, fused=True)
    assert dim == 3 + 30 and fused.fused and not plain.fused
    assert torch.equal(plain(x), fused(x))
    assert torch.equal(plain(x.double()), fused(x.double())) and fused(x.double()).dtype == torch.float64
    prefix = torch.randn(17, 5)
    for emb in (plain, fused):
        assert torch.equal(emb.rows(prefix, x), torch.cat([prefix, plain(x)], dim=-1))
    xg = x.clone().requires_grad_(True)
    fused.rows(prefix, xg).sum().backward()
    xr = x.clone().requires_grad_(True)
    torch.cat([prefix, plain(xr)], dim=-1).sum().backward()
    assert torch.equal(xg.grad, xr.grad)


def test_oracle_derivatives_match_autograd_in_fp64():
    """The oracle's backward, backward2 and chain against torch's double-precision autograd of the composite. Bands that are
    powers of two: the oracle's fp32 product is then exact, the same argument as the fp64 composite's."""
    rng = np.random.default_rng(1)
    d, F, P = 3, 4, 2
    coords = rng.uniform(-1, 1, (9, d)).astype(np.float32)
    bands = (2.0 ** np.arange(F)).astype(np.float32)
    for inc in (True, False):
        width = R.widths(d, F, inc, P)[1]
        go = rng.standard_normal((9, width)).astype(np.float32)
        gg = rng.standard_normal((9, d)).astype(np.float32)
        x = torch.from_numpy(coords).double().requires_grad_(True)
        pre = torch.zeros(9, P, dtype=torch.float64)
        b = torch.from_numpy(bands).double()

        def rows(x):
            w = (x[:, None] * b[None, :, None]).reshape(9, -1)
            return torch.cat([pre] + ([x] if inc else []) + [torch.sin(w), torch.cos(w)], -1)

        row = rows(x)
        g = torch.from_numpy(go).double().requires_grad_(True)
        gc, = torch.autograd.grad(row, x, g, create_graph=True)
        want, mag = R.backward(R.forward(coords, bands, inc, np.zeros((9, P), np.float32)), go, bands, d, inc, P)
        assert np.allclose(gc.detach().numpy(), want, rtol=1e-12, atol=1e-12) and np.all(mag >= np.abs(want) - 1e-12)
        # backward2: the row enters the coordinate gradient through its sin / cos columns
        row_leaf = row.detach().requires_grad_(True)
        bb = b.repeat_interleave(d)[None]
        e = P + (d if inc else 0)
        gc2 = (bb * (row_leaf[:, e + d * F:] * g[:, e:e + d * F] - row_leaf[:, e:e + d * F] * g[:, e + d * F:])
               ).reshape(9, F, d).sum(1) + (g[:, P:e] if inc else 0)
        d_row, d_go = torch.autograd.grad(gc2, (row_leaf, g), torch.from_numpy(gg).double())
        w_row, w_go = R.backward2(gg, row.detach().numpy(), go, bands, d, inc, P)
        assert np.allclose(d_row.numpy(), w_row, rtol=1e-12, atol=1e-12)
        assert np.allclose(d_go.numpy(), w_go, rtol=1e-12, atol=1e-12)
        # chain: L = sum |d(row . v)/dx|^2
        v = rng.standard_normal(width).astype(np.float32)
        x2 = torch.from_numpy(coords).double().requires_grad_(True)
        fx, = torch.autograd.grad((rows(x2) * torch.from_numpy(v).double()).sum(), x2, create_graph=True)
        dL, = torch.autograd.grad(fx.square().sum(), x2)
        want, mag = R.chain(coords, bands, v, inc, P)
        assert np.allclose(dL.numpy(), want, rtol=1e-11, atol=1e-11) and np.all(mag >= np.abs(want) - 1e-9)


# ---- the C entry points refuse bad arguments before any HIP call --------------------------------------------------------------
def test_entry_points_validate_their_arguments():
    L = _lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first or n == 0
    E = _lib.EINVAL
    fwd, bwd, bwd2 = L.shacira_posenc_forward, L.shacira_posenc_backward, L.shacira_posenc_backward2
    # n, d, F, include_input, P, coords, cs, prefix, ps, bands, out, os, stream   (d=2, F=4, input, P=3: 3 + 2 + 16 = 21)
    assert fwd(0, 2, 4, 1, 3, one, 2, one, 3, one, one, 21, None) == 0                 # n == 0: nothing to do
    assert fwd(0, 2, 4, 1, 0, None, 2, None, 0, None, None, 18, None) == 0             # ... whatever the pointers
    assert fwd(-1, 2, 4, 1, 3, one, 2, one, 3, one, one, 21, None) == E                # negative n
    assert fwd(5, 0, 4, 1, 3, one, 2, one, 3, one, one, 21, None) == E                 # d
    assert fwd(5, 5, 4, 1, 3, one, 5, one, 3, one, one, 64, None) == E
    assert fwd(5, 2, 0, 1, 3, one, 2, one, 3, one, one, 21, None) == E                 # F
    assert fwd(5, 2, 65, 1, 3, one, 2, one, 3, one, one, 512, None) == E
    assert fwd(5, 2, 4, 1, -1, one, 2, one, 3, one, one, 21, None) == E                # negative P
    assert fwd(5, 2, 4, 1, 3, None, 2, one, 3, one, one, 21, None) == E                # NULL coords
    assert fwd(5, 2, 4, 1, 3, one, 2, None, 3, one, one, 21, None) == E                # P > 0 with a NULL prefix
    assert fwd(5, 2, 4, 1, 3, one, 2, one, 3, None, one, 21, None) == E                # NULL bands
    assert fwd(5, 2, 4, 1, 3, one, 2, one, 3, one, None, 21, None) == E                # NULL out
    assert fwd(5, 2, 4, 1, 3, one, 2, one, 3, one, one, 20, None) == E                 # out stride < P + E
    assert fwd(5, 2, 4, 0, 3, one, 2, one, 3, one, one, 18, None) == E                 # ... without the input: 19
    assert fwd(5, 2, 4, 1, 3, one, 1, one, 3, one, one, 21, None) == E                 # coords stride < d
    assert fwd(5, 2, 4, 1, 3, one, 2, one, 2, one, one, 21, None) == E                 # prefix stride < P
    # n, d, F, include_input, P, row, rs, grad_out, gs, bands, grad_coords, stream
    assert bwd(0, 2, 4, 1, 3, one, 21, one, 21, one, one, None) == 0
    assert bwd(-1, 2, 4, 1, 3, one, 21, one, 21, one, one, None) == E
    assert bwd(5, 5, 4, 1, 3, one, 64, one, 64, one, one, None) == E
    assert bwd(5, 2, 65, 1, 3, one, 512, one, 512, one, one, None) == E
    assert bwd(5, 2, 4, 1, -1, one, 21, one, 21, one, one, None) == E
    assert bwd(5, 2, 4, 1, 3, one, 20, one, 21, one, one, None) == E                   # row stride
    assert bwd(5, 2, 4, 1, 3, one, 21, one, 20, one, one, None) == E                   # grad stride
    for hole in range(4):
        ptrs = [one] * 4
        ptrs[hole] = None
        assert bwd(5, 2, 4, 1, 3, ptrs[0], 21, ptrs[1], 21, ptrs[2], ptrs[3], None) == E
    # n, d, F, include_input, P, gg, row, rs, grad_out, gs, bands, grad_row, grad_grad_out, stream
    assert bwd2(0, 2, 4, 1, 3, one, one, 21, one, 21, one, one, one, None) == 0
    assert bwd2(-1, 2, 4, 1, 3, one, one, 21, one, 21, one, one, one, None) == E
    assert bwd2(5, 0, 4, 1, 3, one, one, 21, one, 21, one, one, one, None) == E
    assert bwd2(5, 2, 0, 1, 3, one, one, 21, one, 21, one, one, one, None) == E
    assert bwd2(5, 2, 4, 1, 3, one, one, 20, one, 21, one, one, one, None) == E
    assert bwd2(5, 2, 4, 1, 3, one, one, 21, one, 20, one, one, one, None) == E
    for hole in range(6):
        ptrs = [one] * 6
        ptrs[hole] = None
        assert bwd2(5, 2, 4, 1, 3, ptrs[0], ptrs[1], 21, ptrs[2], 21, ptrs[3], ptrs[4], ptrs[5], None) == E
    assert (_lib.POSENC_MAX_DIM, _lib.POSENC_MAX_BANDS) == (4, 64)


# ---- NeuralImage: the module surface -----------------------------------------------------------------------------------------
def _grid(num_lods=4):
    return harness.kodak_like_grid(num_lods=num_lods, max_grid_res=64)[0]


def test_neural_image_imports_under_the_reference_name():
    import shacira_amd.wisp as mirror
    saved = {k: v for k, v in sys.modules.items() if k == "wisp" or k.startswith("wisp.")}
    try:
        mirror.install_as_wisp(force=True)
        from wisp.models.activations import get_activation_class as gac
        from wisp.models.nefs import NeuralImage as N1
        from wisp.models.nefs.image import NeuralImage as N2
        assert N1 is N2 is NeuralImage and gac is get_activation_class
    finally:
        for k in [k for k in sys.modules if k == "wisp" or k.startswith("wisp.")]:
            del sys.modules[k]
        sys.modules.update(saved)


@pytest.mark.parametrize("embedder,position_input,embed_dim,kind", [
    ("none", False, 0, type(None)), ("none", True, 2, nn.Identity), ("identity", False, 2, nn.Identity),
    ("identity", True, 2, nn.Identity), ("positional", False, 2 * 2 * 4, PositionalEmbedder),
    ("positional", True, 2 + 2 * 2 * 4, PositionalEmbedder)])
def test_constructor_matrix(embedder, position_input, embed_dim, kind):
    grid = _grid()
    nef = NeuralImage(grid, pos_embedder=embedder, pos_multires=4, position_input=position_input, hidden_dim=8,
                      num_layers=2)
    assert isinstance(nef.pos_embedder, kind) and nef.pos_embed_dim == embed_dim
    assert nef.effective_feature_dim() == 8 and nef.color_net_input_dim() == 8 + embed_dim
    assert len(nef.decoder_color.layers) == 3 and nef.decoder_color.layers[0].in_features == 8 + embed_dim
    assert nef.decoder_color.lout.out_features == 3
    names = [n for n, _ in nef.named_parameters() if not n.startswith("grid.")]
    want = [f"decoder_color.layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")] + \
        ["decoder_color.lout.weight", "decoder_color.lout.bias"]
    assert names == (["pos_embedder.bands"] if kind is PositionalEmbedder else []) + want
    assert [n for n, _ in nef.named_parameters() if n.startswith("grid.")] == \
        ["grid." + n for n, _ in grid.named_parameters()]
    groups = {g["name"]: g["params"] for g in harness.param_groups(nef)}
    assert len(groups["decoder"]) == 8 and len(groups["rest"]) == (1 if kind is PositionalEmbedder else 0)
    assert nef.get_supported_channels() == {"rgb"}
    assert set(nef.public_properties()) == {"Grid", "Pos. Embedding", "Decoder (color)", "Final Activation"}
    if kind is PositionalEmbedder:
        assert nef.pos_embedder.fused and not NeuralImage(grid, pos_embedder="positional",
                                                          fused_embedder=False).pos_embedder.fused


def test_constructor_defaults_and_refusals():
    nef = NeuralImage(_grid())
    assert (nef.pos_embedder, nef.pos_embed_dim, nef.activation_type, nef.layer_type, nef.hidden_dim, nef.num_layers) == \
        (None, 0, "relu", "none", 128, 1)
    assert NeuralImage(_grid(), pos_embedder="positional").pos_embedder.num_freq == 10
    with pytest.raises(NotImplementedError):
        NeuralImage(_grid(), layer_type="spectral_norm")
    with pytest.raises(NotImplementedError):
        NeuralImage(_grid(), pos_embedder="fourier")
    with pytest.raises(TypeError):
        NeuralImage(_grid(), "none", 10, False, "relu", "none", "none", 128, 1, False)     # fused_embedder is keyword-only


def test_harness_state_dict_loads_and_gives_the_same_rgb(oracle_op):
    torch.manual_seed(2)
    grid = _grid()
    old = harness.NeuralImage(grid, hidden_dim=16, num_layers=1)
    new = NeuralImage(_grid(), pos_embedder="none", hidden_dim=16, num_layers=1)
    new.load_state_dict(old.state_dict())
    coords = torch.rand(64, 2) * 2 - 1
    with torch.no_grad():
        want, got = old.rgb(coords), new.rgb(coords)
    assert set(got) == {"rgb"} and torch.equal(got["rgb"], want)
    with torch.no_grad():
        assert torch.equal(new(channels="rgb", coords=coords), want)
        assert torch.equal(new(coords=coords)["rgb"], want) and torch.equal(new(channels=["rgb"], coords=coords)["rgb"], want)


DEFINITIONS = {
    "none": lambda x: x, "identity": lambda x: x, "relu": lambda x: x.clamp(min=0), "sin": torch.sin,
    "sinescaled": lambda x: torch.sin(30.0 * x), "sigmoid": lambda x: 1 / (1 + torch.exp(-x)),
    "fullsort": lambda x: x.sort(-1)[0],
    "minmax": lambda x: torch.stack([torch.minimum(x[:, 0::2], x[:, 1::2]), torch.maximum(x[:, 0::2], x[:, 1::2])],
                                    -1).reshape(x.shape),
}


@pytest.mark.parametrize("name", sorted(DEFINITIONS))
def test_activation_names(oracle_op, name):
    torch.manual_seed(3)
    x = torch.randn(12, 8)
    assert torch.allclose(get_activation_class(name)(x), DEFINITIONS[name](x), rtol=1e-6, atol=1e-7)
    coords = torch.rand(20, 2) * 2 - 1
    nef = NeuralImage(_grid(), pos_embedder="positional", pos_multires=2, activation_type=name, hidden_dim=8)
    out = nef.rgb(coords)["rgb"]
    x = torch.cat([nef.grid.interpolate(coords, 3).reshape(20, 8), nef.pos_embedder(coords)], -1)
    for lin in nef.decoder_color.layers:
        x = DEFINITIONS[name](lin(x))
    assert out.shape == (20, 3) and torch.allclose(out, nef.decoder_color.lout(x), rtol=1e-5, atol=1e-6)
    if name in ("none", "relu", "sigmoid"):
        fin = NeuralImage(_grid(), final_activation=name, hidden_dim=8)
        with torch.no_grad():
            raw = fin.decoder_color(fin.grid.interpolate(coords, 3).reshape(20, 8))
            assert torch.allclose(fin.rgb(coords)["rgb"], DEFINITIONS[name](raw), rtol=1e-6, atol=1e-7)


def test_unknown_activation_is_refused():
    with pytest.raises(AssertionError):
        get_activation_class("gelu")


def test_model_file_round_trips_a_positional_neural_image(oracle_op):
    torch.manual_seed(4)
    nef = NeuralImage(_grid(), pos_embedder="positional", pos_multires=4, position_input=True, hidden_dim=16).eval()
    with torch.no_grad():
        nef.grid.codebook.mul_(30).round_()
    coords = torch.rand(50, 2) * 2 - 1
    with torch.no_grad():
        want = nef.rgb(coords)["rgb"]
    data = codec.save_model(nef)
    torch.manual_seed(5)
    back = NeuralImage(_grid(), pos_embedder="positional", pos_multires=4, position_input=True, hidden_dim=16).eval()
    with torch.no_grad():
        back.pos_embedder.bands.zero_()
    codec.load_model(back, data)
    assert torch.equal(back.pos_embedder.bands, nef.pos_embedder.bands)
    with torch.no_grad():
        assert torch.equal(back.rgb(coords)["rgb"], want)
