"""The pixel contracts on the host (no GPU): the restatement of tests/pixels_ref.py against the reference's own formulas -- its
index-to-coordinate rule, its lattice, ToTensor's division, the clamped-MSE chain -- and the entry points' validation codes,
which precede any HIP call."""
import ctypes

import pytest
import torch

import pixels_ref as R
from shacira_amd import _lib


@pytest.mark.parametrize("H,W", R.IMAGE_SIZES)
def test_integer_rule_equals_the_references_rules_for_every_pixel(H, W):
    """Up to 2^24 pixels the reference's fp32 division rule, its pregenerated lattice and the exact integer rule agree to the
    bit, for EVERY pixel of the image."""
    image = R.make_image(H, W)
    coords, rgb = R.pixel_batch_ref(image)
    idx = torch.arange(H * W, dtype=torch.int64).reshape(-1, 1)
    assert torch.equal(coords, R.reference_transform_coords(idx, H, W))
    assert torch.equal(coords, R.reference_lattice(H, W))
    assert torch.equal(rgb, R.to_tensor_division(image))
    assert coords.dtype == torch.float32 and rgb.dtype == torch.float32
    assert coords.min() >= -1 and coords.max() < 1


def test_references_rule_leaves_the_pixel_above_2_to_24():
    """The difference the dataset's docstring states: at the reference's own gigapixel size its rule returns another pixel's
    coordinate for most indices, the integer rule by construction does not."""
    H, W = 20000, 23466
    idx = torch.randint(0, H * W, (1 << 16, 1), generator=torch.Generator().manual_seed(0))
    y = idx // W
    exact = torch.cat([(y.float() / float(H) - 0.5) * 2, ((idx - y * W).float() / float(W) - 0.5) * 2], dim=1)
    wrong = (R.reference_transform_coords(idx, H, W) != exact).any(dim=1).float().mean().item()
    assert wrong > 0.5, wrong


def test_a_bytes_own_level_is_the_byte():
    """(clamp(b / 255, 0, 1) * 255).to(uint8) == b for all 256 values: the target's level in the clamped MSE is its byte."""
    b = torch.arange(256, dtype=torch.int64)
    assert torch.equal((torch.clamp(b.float() / 255.0, 0, 1) * 255).to(torch.uint8).to(torch.int64), b)


@pytest.mark.parametrize("H,W", R.IMAGE_SIZES[1:4])
def test_loss_restatement_equals_the_torch_chains(H, W):
    image = R.make_image(H, W)
    n = H * W
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    pred = R.pred_for(n, image, perm)
    target = R.to_tensor_division(image)[perm]
    r = R.pixel_loss_ref(pred, image, perm)
    assert r["lvl"] == R.clamped_level_sum(pred, target) and r["count"] == n
    assert r["sq"] == ((pred - target).double() ** 2).sum().item()
    assert torch.equal(r["levels"], (torch.clamp(pred, 0, 1) * 255).to(torch.uint8))
    leaf = pred.clone().requires_grad_(True)
    for k in (1.0, 1.0 / (3 * n)):
        leaf.grad = None
        (((leaf - target) ** 2).sum() * k).backward()
        assert torch.equal(R.pixel_grad_ref(pred, image, perm, 0, k), leaf.grad)
    # indices outside the image: NaN rows in the batch, skipped in the loss, zero in the gradient
    idx = torch.tensor([0, -1, n - 1, n])
    coords, rgb = R.pixel_batch_ref(image, idx)
    assert torch.isnan(coords[[1, 3]]).all() and torch.isnan(rgb[[1, 3]]).all() and not torch.isnan(coords[[0, 2]]).any()
    r = R.pixel_loss_ref(pred[:4], image, idx)
    assert r["count"] == 2 and (R.pixel_grad_ref(pred[:4], image, idx, 0, 1.0)[[1, 3]] == 0).all()
    # NaN predictions: level 0, NaN in the squared error
    bad = R.add_nonfinite(pred[:16]) if n >= 16 else None
    if bad is not None:
        r = R.pixel_loss_ref(bad, image, perm[:16])
        assert r["sq"] != r["sq"] and int(r["levels"][8, 0]) == 0 and int(r["levels"][5, 1]) == 255 and int(r["levels"][4, 2]) == 0


def test_pixel_entry_points_validate_their_arguments():
    """SHACIRA_EINVAL before anything is launched: pointers here are never dereferenced."""
    L = _lib.lib()
    one = ctypes.c_void_p(64)
    E = _lib.EINVAL
    batch, fwd, bwd = L.shacira_pixel_batch, L.shacira_pixel_loss_forward, L.shacira_pixel_loss_backward
    assert batch(one, 0, 4, None, 64, 0, 1, one, one, None) == E               # H <= 0
    assert batch(one, 4, 0, None, 64, 0, 1, one, one, None) == E               # W <= 0
    assert batch(one, 4, 1 << 31, None, 64, 0, 1, one, one, None) == E         # W beyond int32
    assert batch(one, 4, 4, None, 64, 0, -1, one, one, None) == E              # n < 0
    assert batch(one, 4, 4, one, 16, 0, 1, one, one, None) == E                # idx_bits
    assert batch(one, 4, 4, one, 0, 0, 1, one, one, None) == E
    assert batch(one, 4, 4, None, 64, -1, 1, one, one, None) == E              # range form: start < 0
    assert batch(one, 4, 4, None, 64, 15, 2, one, one, None) == E              # start + n > H W
    assert batch(one, 4, 4, None, 64, 16, 0, one, one, None) == 0              # empty range at the end
    assert batch(None, 4, 4, None, 0, 0, 0, None, None, None) == 0             # n == 0: nothing enqueued, whatever the pointers
    assert batch(None, 4, 4, None, 64, 0, 1, one, one, None) == E              # NULL image
    assert batch(one, 4, 4, None, 64, 0, 1, None, None, None) == E             # neither output
    ws = L.shacira_pixel_loss_workspace_bytes
    assert ws(0) == 0 and ws(-5) == 0 and ws(1) == _lib.PIXEL_PARTIAL_BYTES and ws(257) == 2 * _lib.PIXEL_PARTIAL_BYTES
    assert ws(1 << 40) == _lib.PIXEL_MAX_GRID * _lib.PIXEL_PARTIAL_BYTES
    assert ws(R.N_ABOVE_CAP) == R.MAX_GRID * _lib.PIXEL_PARTIAL_BYTES and R.MAX_GRID == _lib.PIXEL_MAX_GRID
    assert fwd(one, 2, one, 4, 4, None, 64, 0, 1, None, one, one, 24, None) == E      # row stride below 3
    assert fwd(one, 3, one, 4, 4, one, 33, 0, 1, None, one, one, 24, None) == E       # idx_bits
    assert fwd(one, 3, one, 4, 4, None, 64, 8, 9, None, one, one, 24, None) == E      # the range leaves the image
    assert fwd(one, 3, one, 4, 4, None, 64, 0, 0, None, None, None, 0, None) == 0     # n == 0
    assert fwd(None, 3, one, 4, 4, None, 64, 0, 1, None, one, one, 24, None) == E     # NULL pred
    assert fwd(one, 3, None, 4, 4, None, 64, 0, 1, None, one, one, 24, None) == E     # NULL image
    assert fwd(one, 3, one, 4, 4, None, 64, 0, 1, None, None, one, 24, None) == E     # NULL stats
    assert fwd(one, 3, one, 4, 4, None, 64, 0, 1, None, one, None, 24, None) == E     # missing workspace
    assert fwd(one, 3, one, 4, 4, None, 64, 0, 1, None, one, one, 23, None) == E      # short workspace
    assert fwd(one, 1 << 60, one, 4, 4, None, 64, 0, 16, None, one, one, 24, None) == E
    assert bwd(one, 2, one, 4, 4, None, 64, 0, 1, one, one, None) == E
    assert bwd(one, 3, one, 4, 4, one, 8, 0, 1, one, one, None) == E
    assert bwd(one, 3, one, 4, 4, None, 64, 0, 17, one, one, None) == E
    assert bwd(one, 3, one, 4, 4, None, 64, 0, 0, None, None, None) == 0
    assert bwd(one, 3, one, 4, 4, None, 64, 0, 1, None, one, None) == E               # NULL grad
    assert bwd(one, 3, one, 4, 4, None, 64, 0, 1, one, None, None) == E               # NULL grad_pred
    assert L.shacira_abi_version() == 11                                             # the additions do not move the ABI


def test_binding_refuses_host_and_malformed_operands():
    from shacira_amd import hip_ops
    image = R.make_image(5, 3)
    with pytest.raises(RuntimeError, match="HIP"):
        hip_ops.pixel_batch(image)
    with pytest.raises(RuntimeError, match="HIP"):
        hip_ops.pixel_loss(torch.zeros(15, 3), image)
