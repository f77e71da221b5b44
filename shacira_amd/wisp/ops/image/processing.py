"""Colour-space helpers (reference wisp/ops/image/processing.py), in torch where the image lives. ``resize_mip`` is not
mirrored: it is a thin wrapper over OpenCV."""
import torch


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
