"""``wisp.models.nefs.NeuralImage`` on the MI355X: a config-B-like 2-D LatentGrid (16 levels x 2 features), 4 099 pixels, a
4-band positional embedder without the raw position: 32 + 16 = a 48-wide decoder row, hidden width 16, two hidden layers -- the
shape for which the fused MFMA decoder is instantiated. The row written by the HIP kernel (``fused_embedder=True``) against the
torch composite (``fused_embedder=False``) on the same device, through the same fused decoder.

The bound. The two rows differ in their sin / cos columns by the few ulp that separate the device library's sincosf from torch's
sin and cos; the decoder and the grid's backward amplify that as they amplify any rounding. The yardstick for such noise is
a difference of the same kind that the project already accepts: the fused-MLP decoder against the plain ``nn.Linear`` chain on
IDENTICAL rows (both composites), same module, same seed. Per tensor, the relative difference is max |a - b| / max |b|; the
worst over rgb, the decoder gradients and grid.codebook.grad was measured on the MI355X (tools/posenc_ab.py --noise,
profiles/posenc.md) and the bound is twice that figure."""
import numpy as np
import pytest
import torch

from shacira_amd import harness
from shacira_amd.wisp.models.nefs import NeuralImage

pytestmark = pytest.mark.gpu

# worst relative difference, fused-MLP decoder against the Linear chain on identical composite rows (profiles/posenc.md)
DECODER_NOISE = 5.43e-07
BOUND = 2.0 * DECODER_NOISE
PIXELS = 4099


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def build(dev, fused_embedder, state=None):
    torch.manual_seed(0)
    grid, cdec, cent = harness.kodak_like_grid(num_lods=16, feature_dim=2)
    nef = NeuralImage(grid, pos_embedder="positional", pos_multires=4, position_input=False, hidden_dim=16, num_layers=1,
                      fused_embedder=fused_embedder).to(dev)
    if state is not None:
        nef.load_state_dict(state)
    return nef, cdec, cent


def evaluate(nef, coords, target):
    """rgb and the gradients of the MSE loss with respect to the decoder and the latent table, as {name: tensor}."""
    torch.manual_seed(1)            # the latent decoder draws its training noise from the global generator
    nef.zero_grad(set_to_none=True)
    rgb = nef.rgb(coords)["rgb"]
    ((rgb - target) ** 2).mean().backward()
    out = {"rgb": rgb.detach()}
    for name, p in nef.named_parameters():
        if name.startswith("decoder_color.") or name == "grid.codebook":
            out[name + ".grad"] = p.grad.detach().clone()
    return out


def relative_differences(a, b):
    return {k: float((a[k] - b[k]).abs().max() / b[k].abs().max()) for k in b}


def test_fused_row_feeds_the_fused_decoder_and_matches_the_composite(dev):
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(-1, 1, (PIXELS, 2)).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.uniform(0, 1, (PIXELS, 3)).astype(np.float32)).to(dev)
    fused, _, _ = build(dev, True)
    plain, _, _ = build(dev, False, fused.state_dict())
    assert fused.pos_embedder.fused and not plain.pos_embedder.fused
    assert fused.color_net_input_dim() == 48
    row = fused.pos_embedder.rows(torch.zeros(PIXELS, 32, device=dev), coords)
    assert row.shape == (PIXELS, 48) and fused.decoder_color._fused_dims(row) is not None      # the fused MLP takes the row
    assert fused.decoder_color._fused_dims(row) == (48, 16, 2, 3)
    got, want = evaluate(fused, coords, target), evaluate(plain, coords, target)
    assert set(got) == set(want) and len(want) == 1 + 6 + 1
    diffs = relative_differences(got, want)
    for name, v in sorted(diffs.items()):
        print(f"NeuralImage fused row vs composite row, {name}: {v:.3e} (bound {BOUND})")
    assert all(torch.isfinite(t).all() for t in got.values())
    assert float(want["grid.codebook.grad"].abs().max()) > 0
    assert max(diffs.values()) <= BOUND, diffs


def test_one_image_fitter_step(dev):
    nef, cdec, cent = build(dev, True)
    image = harness.make_test_image(48, 64, seed=2)
    coords = harness.image_coords(48, 64).to(dev)
    fitter = harness.ImageFitter(nef, coords, torch.from_numpy(image).reshape(-1, 3).to(dev), 10, cdec, cent)
    loss, psnr, bits = fitter.step()
    assert np.isfinite(loss) and np.isfinite(psnr) and np.isfinite(bits) and loss > 0 and bits > 0
    loss2, _, _ = fitter.step()
    assert np.isfinite(loss2)
