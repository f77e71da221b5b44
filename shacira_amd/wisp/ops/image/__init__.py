from .metrics import psnr, clamped_psnr
from .io import load_rgb, load_rgb_tensor, load_rgb_u8, write_png, glob_imgs, hwc_to_chw, chw_to_hwc  # noqa: F401
from .processing import srgb_to_linear, linear_to_srgb, resize_mip, INTER_NEAREST, INTER_LINEAR, INTER_AREA  # noqa: F401
