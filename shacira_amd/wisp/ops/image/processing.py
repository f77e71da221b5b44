"""Colour-space helpers and ``resize_mip`` (reference wisp/ops/image/processing.py), in torch where the image lives.

The reference's ``resize_mip`` is a thin wrapper over ``cv2.resize`` by a factor 2^-mip. OpenCV is not a dependency here; at a
power-of-two factor on a size the factor divides, its three interpolation modes the reference uses have closed forms, restated
below. uint8 images do not go through here: their mip levels are exact integer sums made on the device
(``shacira_amd.hip_ops.image_mip``)."""
import numpy as np
import torch

# OpenCV's values, so that the reference's call sites read unchanged
INTER_NEAREST = 0
INTER_LINEAR = 1
INTER_AREA = 3


def srgb_to_linear(img):
    """sRGB -> linear: ``((x + 0.055) / 1.055) ** 2.4`` above 0.04045, ``x / 12.92`` at and below it. (The reference calls
    ``torch.power``, which does not exist; this is its formula with ``torch.pow``.)"""
    limit = 0.04045
    return torch.where(img > limit, torch.pow((img + 0.055) / 1.055, 2.4), img / 12.92)


def linear_to_srgb(img):
    """linear -> sRGB: ``1.055 x ** (1 / 2.4) - 0.055`` above 0.0031308, ``12.92 x`` at and below it, then capped at 1."""
    limit = 0.0031308
    img = torch.where(img > limit, 1.055 * (img ** (1.0 / 2.4)) - 0.055, 12.92 * img)
    img[img > 1] = 1
    return img


def resize_mip(img, mip, interpolation=INTER_LINEAR):
    """``img`` [H, W] or [H, W, C], a float tensor or numpy array, scaled down by f = 2^mip: the same kind of array,
    [H // f, W // f, ...]. What ``cv2.resize(img, (W // f, H // f), interpolation=...)`` computes when f divides H and W:

    * ``INTER_AREA``: the mean of each f x f block;
    * ``INTER_NEAREST``: ``img[::f, ::f]`` -- OpenCV's source index is floor(x * f);
    * ``INTER_LINEAR``: OpenCV samples at (x + 0.5) f - 0.5, for f >= 2 exactly half way between the two central pixels of the
      block along each axis: the mean of the block's central 2 x 2, as two passes with weights 0.5 / 0.5 (columns, then rows).

    ``mip = 0`` returns ``img`` itself. A size f does not divide raises ValueError (OpenCV's fractional-scale resampling is not
    restated); a uint8 image raises TypeError: the reference only passes floats, OpenCV's uint8 rounding differs between its
    code paths, and ``hip_ops.image_mip`` keeps a uint8 level exactly."""
    is_numpy = isinstance(img, np.ndarray)
    if not is_numpy and not torch.is_tensor(img):
        raise TypeError(f"resize_mip expects a float tensor or numpy array, got {type(img).__name__}")
    floating = np.issubdtype(img.dtype, np.floating) if is_numpy else img.dtype.is_floating_point
    if not floating:
        raise TypeError(f"resize_mip takes float images, got {img.dtype}: a uint8 image's mip level is made exactly, as integer "
                        "block sums, by shacira_amd.hip_ops.image_mip")
    if img.ndim not in (2, 3):
        raise ValueError(f"resize_mip expects [H, W] or [H, W, C], got {tuple(img.shape)}")
    if interpolation not in (INTER_NEAREST, INTER_LINEAR, INTER_AREA):
        raise ValueError(f"resize_mip: interpolation must be INTER_NEAREST, INTER_LINEAR or INTER_AREA, got {interpolation!r}")
    mip = int(mip)
    if mip < 0:
        raise ValueError(f"resize_mip: mip must be >= 0, got {mip}")
    if mip == 0:
        return img
    f = 1 << mip
    H, W = img.shape[:2]
    if H % f or W % f:
        raise ValueError(f"resize_mip: {H} x {W} is not divisible by 2^mip = {f}")
    if interpolation == INTER_NEAREST:
        return img[::f, ::f]
    blocks = img.reshape(H // f, f, W // f, f, *img.shape[2:])
    if interpolation == INTER_AREA:
        return blocks.mean(axis=(1, 3)) if is_numpy else blocks.mean(dim=(1, 3))
    m = f // 2
    cols = blocks[:, :, :, m - 1] * 0.5 + blocks[:, :, :, m] * 0.5
    return cols[:, m - 1] * 0.5 + cols[:, m] * 0.5
