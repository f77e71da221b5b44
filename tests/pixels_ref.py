"""Restatement in torch ops (host, one rounding per operator) of the three contracts of shacira_amd/csrc/pixels.hip, as
include/shacira_hip.h words them: shacira_pixel_batch, shacira_pixel_loss_forward, shacira_pixel_loss_backward. Also the
reference's own formulas the contracts are held against in tests/test_pixels_cpu.py: its index-to-coordinate rule
(multi_image_dataset.py:232-242), its lattice (:148-153), ToTensor's division and the clamped-MSE chain (metrics.py:60-79)."""
import numpy as np
import torch

IMAGE_SIZES = ((1, 1), (1, 7), (5, 3), (37, 53), (512, 768))      # (H, W): the images every pixel test uses
N_LIST = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
MAX_GRID, BLOCK = 2048, 256                                        # SHACIRA_PIXEL_MAX_GRID and the kernels' workgroup
N_ABOVE_CAP = MAX_GRID * BLOCK + 257                               # the grid-stride loops turn twice


def make_image(H, W, seed=0):
    """A uint8 [H, W, 3] image with every byte value present when it is large enough."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    flat = img.reshape(-1)
    k = min(256, flat.numel())
    flat[:k] = torch.arange(k).to(torch.uint8)
    return img


def _indices(image, pixel_idx, start, n):
    hw = image.shape[0] * image.shape[1]
    if pixel_idx is None:
        n = hw - start if n is None else n
        assert 0 <= start and start + n <= hw
        return torch.arange(start, start + n, dtype=torch.int64)
    return pixel_idx.reshape(-1).to(torch.int64).cpu()


def pixel_batch_ref(image, pixel_idx=None, start=0, n=None):
    """(coords fp32 [n, 2], rgb fp32 [n, 3]); NaN rows for indices outside the image."""
    H, W = image.shape[:2]
    p = _indices(image, pixel_idx, start, n)
    ok = (p >= 0) & (p < H * W)
    q = torch.where(ok, p, torch.zeros_like(p))
    y = q // W
    x = q - y * W
    coords = torch.stack([(y.to(torch.float32) / np.float32(H) - 0.5) * 2.0, (x.to(torch.float32) / np.float32(W) - 0.5) * 2.0],
                         dim=-1)
    rgb = image.reshape(-1, 3)[q].to(torch.float32) / 255.0
    coords[~ok] = float("nan")
    rgb[~ok] = float("nan")
    return coords, rgb


def pixel_loss_ref(pred, image, pixel_idx=None, start=0):
    """dict(sq: fp64 sum of the squared fp32 differences, accumulated in fp64 by torch; lvl, count: Python ints; levels uint8
    [n, 3]; ok bool [n]; d fp32 [n, 3]) over the first three columns of ``pred``."""
    H, W = image.shape[:2]
    pred = pred[:, :3].to(torch.float32).cpu()
    p = _indices(image, pixel_idx, start, pred.shape[0])
    ok = (p >= 0) & (p < H * W)
    q = torch.where(ok, p, torch.zeros_like(p))
    byte = image.reshape(-1, 3)[q]
    d = pred - byte.to(torch.float32) / 255.0
    c = torch.where(pred > 0, pred, torch.zeros_like(pred))          # NaN -> 0, as the contract says
    c = torch.where(c < 1, c, torch.ones_like(c))
    levels = (c * 255.0).to(torch.int64)                             # truncation of a value in [0, 255]
    e = (levels - byte.to(torch.int64))[ok]
    return dict(sq=(d[ok].double() ** 2).sum().item(), lvl=int((e * e).sum().item()), count=int(ok.sum().item()),
                levels=levels.to(torch.uint8), ok=ok, d=d, pixels=p)


def pixel_grad_ref(pred, image, pixel_idx, start, g):
    """fp32 [n, 3]: g * (2 * d), zero rows for skipped pixels; g an fp32 scalar."""
    r = pixel_loss_ref(pred, image, pixel_idx, start)
    grad = torch.tensor(g, dtype=torch.float32) * (2.0 * r["d"])
    grad[~r["ok"]] = 0.0
    return grad


def pred_for(n, image, pixel_idx=None, start=0, seed=0, width=3):
    """Finite predictions [n, width] in [-0.3, 1.3] with rows of exact 0, 1 and k / 255 (the pixel's own colour among them)."""
    g = torch.Generator().manual_seed(77 + n + seed)
    pred = torch.rand((n, width), generator=g) * 1.6 - 0.3
    if n >= 8:
        _, rgb = pixel_batch_ref(image, pixel_idx, start, n)
        pred[0, :3] = 0.0
        pred[1, :3] = 1.0
        pred[2, :3] = torch.nan_to_num(rgb[2], nan=0.5)              # k / 255: the difference is exactly zero
        pred[3, :3] = torch.tensor([64 / 255, 128 / 255, 254 / 255])
        pred[4, :3] = torch.tensor([-0.0, 1.0 - 2 ** -24, 1.0 + 2 ** -23])
    return pred


def add_nonfinite(pred):
    """A copy of ``pred`` with a NaN row, a +Inf and a -Inf entry."""
    pred = pred.clone()
    n = pred.shape[0]
    pred[n // 2, 0] = float("nan")
    pred[n // 3, 1] = float("inf")
    pred[n // 4, 2] = float("-inf")
    return pred


# ---- the reference's own formulas -------------------------------------------------------------------------------------------
def reference_transform_coords(idx, H, W):
    """The reference's rule for [n, 1] int64 indices: floor-divide by the fp32 row (W, 1), take the remainder by (H, W),
    normalise by (H, W) to [-1, 1). The division happens in fp32: the index is rounded to 24 bits first."""
    cell = torch.div(idx, torch.tensor([[float(W), 1.0]]), rounding_mode="floor").long()
    cell = torch.remainder(cell, torch.tensor([[H, W]]))
    return (cell / torch.tensor([[H, W]]) - 0.5) * 2


def reference_lattice(H, W):
    """The reference's pregenerated grid [H W, 2], row first."""
    gy, gx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    gy, gx = (gy / H - 0.5) * 2, (gx / W - 0.5) * 2
    return torch.stack([gy.reshape(-1, 1), gx.reshape(-1, 1)], dim=-1).reshape(-1, 2)


def to_tensor_division(image):
    """torchvision's ToTensor on an 8-bit HWC image, as [H W, 3]: bytes as fp32, divided by 255."""
    return image.reshape(-1, 3).to(torch.float32).div(255)


def clamped_level_sum(pred, target):
    """The integer numerator of the clamped MSE: both sides clamped to [0, 1], times 255, truncated to uint8."""
    q = lambda t: (torch.clamp(t, 0, 1) * 255).to(torch.uint8).to(torch.int64)
    return int(((q(pred) - q(target)) ** 2).sum().item())
