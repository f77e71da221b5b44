"""Reading and writing images (wisp/ops/image/io.py), on PIL alone: the reference decodes with PIL and converts with torchvision's
``ToTensor`` / ``read_image`` / ``write_png``; torchvision is not a dependency here, so the conversions are restated --
``ToTensor`` of an 8-bit RGB image is ``bytes.permute(2, 0, 1).float() / 255`` (one fp32 division per byte), which is also what
the pixel kernels compute. ``load_rgb_u8`` is an addition: the bytes themselves, which is all ``MultiImageDataset`` keeps.
``write_exr`` is not restated (pyexr is not a dependency)."""
import glob
import os

import numpy as np
import torch

MAX_IMAGE_PIXELS = 1216601101        # the reference raises PIL's limit to this for its gigapixel image (io.py:85)


def _open_rgb(path):
    import PIL.Image
    try:
        return PIL.Image.open(path).convert("RGB")
    except Exception:                # PIL refuses very large images as "decompression bombs"; the reference retries likewise
        PIL.Image.MAX_IMAGE_PIXELS = MAX_IMAGE_PIXELS
        return PIL.Image.open(path).convert("RGB")


def load_rgb_u8(path):
    """The image at ``path`` as a uint8 [H, W, 3] tensor on the host (any PIL mode is converted to RGB, as the reference does)."""
    return torch.from_numpy(np.array(_open_rgb(path), dtype=np.uint8))


def load_rgb_tensor(path, normalize=True):
    """The image as an fp32 [3, H, W] tensor in [0, 1] (``ToTensor`` of the RGB image; ``normalize`` is ignored, as in the
    reference)."""
    return hwc_to_chw(load_rgb_u8(path)).contiguous().float() / 255.0


def load_rgb(path, normalize=True):
    """The image as a numpy array [H, W, C] with the file's own channels: fp32 in [0, 1], or uint8 with ``normalize=False``."""
    import PIL.Image
    with PIL.Image.open(path) as im:
        if im.mode not in ("L", "LA", "RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        img = np.array(im, dtype=np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    return img.astype(np.float32) / np.float32(255.0) if normalize else img


def write_png(path, data):
    """Write an [H, W, C] uint8 image (tensor or array; C in 1, 3, 4) as a PNG."""
    import PIL.Image
    if torch.is_tensor(data):
        data = data.detach().cpu().numpy()
    data = np.ascontiguousarray(data)
    if data.dtype != np.uint8 or data.ndim != 3 or data.shape[2] not in (1, 3, 4):
        raise ValueError(f"write_png expects uint8 [H, W, 1 | 3 | 4], got {data.dtype} {data.shape}")
    PIL.Image.fromarray(data[..., 0] if data.shape[2] == 1 else data).save(path, format="PNG")


def glob_imgs(path, exts=("*.png", "*.PNG", "*.jpg", "*.jpeg", "*.JPG", "*.JPEG")):
    """The images in ``path`` with one of the extensions, in the order of the extensions."""
    imgs = []
    for ext in exts:
        imgs.extend(glob.glob(os.path.join(path, ext)))
    return imgs


def hwc_to_chw(img):
    """[H, W, C] -> [C, H, W] (a view)."""
    return img.permute(2, 0, 1)


def chw_to_hwc(img):
    """[C, H, W] -> [H, W, C] (a view)."""
    return img.permute(1, 2, 0)
