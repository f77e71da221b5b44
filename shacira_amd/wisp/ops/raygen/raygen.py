"""Ray generation with the reference's names (wisp/ops/raygen/raygen.py) and ``generate_rays``, the batched form the datasets
use: rays of arbitrary (view, pixel) pairs plus their composited target colours.

Two paths compute the same thing. Device tensors take the fused HIP kernel (``hip_ops.raygen``): fp32 arithmetic from fp32 camera
records. Host tensors -- and a ``coords_grid`` that is not the full-resolution centred grid, wherever it lives -- take the
composite: the reference's chain of torch operators in the camera's dtype, cast to fp32 at the end. Neither is differentiable
with respect to the camera: the reference does not optimise poses."""
import torch

from .... import _lib, hip_ops
from ...core import CameraFOV, Rays


def generate_2d_grid(width, height, device=None):
    """(pixel_y, pixel_x), both [height, width] integer grids."""
    h_coords = torch.arange(height, device=device)
    w_coords = torch.arange(width, device=device)
    return torch.meshgrid(h_coords, w_coords, indexing="ij")


def generate_centered_pixel_coords(img_width, img_height, res_x=None, res_y=None, device=None):
    """(pixel_y, pixel_x) of the centres of a res_y x res_x grid of pixels laid over an img_height x img_width image."""
    res_x = img_width if res_x is None else res_x
    res_y = img_height if res_y is None else res_y
    pixel_y, pixel_x = generate_2d_grid(res_x, res_y, device)
    pixel_x = pixel_x * (float(img_width) / res_x) + 0.5
    pixel_y = pixel_y * (float(img_height) / res_y) + 0.5
    if res_x == img_width and res_y == img_height:
        # the grid every dataset asks for: remembered on the tensors so that generate_*_rays can hand a device grid to the kernel
        # without comparing it against arange on the device. Any operator on the tensors drops the mark: then the composite runs.
        pixel_y._shacira_full_grid = pixel_x._shacira_full_grid = (int(img_width), int(img_height))
    return pixel_y, pixel_x


def camera_records(cameras):
    """fp32 [V, RAYGEN_RECORD_FLOATS] records of the kernel (layout: include/shacira_hip.h, shacira_raygen), rounded once from
    the camera's own dtype."""
    V = len(cameras)
    rec = torch.zeros((V, _lib.RAYGEN_RECORD_FLOATS), dtype=cameras.dtype, device=cameras.device)
    rec[:, 0:9] = cameras.view_matrix()[:, :3, :3].transpose(1, 2).reshape(V, 9)
    rec[:, 9:12] = cameras.cam_pos()
    rec[:, 12] = cameras.tan_half_fov(CameraFOV.HORIZONTAL)
    rec[:, 13] = cameras.tan_half_fov(CameraFOV.VERTICAL)
    rec[:, 14] = cameras.x0
    rec[:, 15] = cameras.y0
    if cameras.lens_type == "ortho":
        rec[:, 16] = 1.0
        rec[:, 17] = cameras.fov_distance * (cameras.width / cameras.height)
        rec[:, 18] = cameras.fov_distance
    return rec.to(torch.float32).contiguous()


def _camera_rays(cameras, view, px, py):
    """The composite: rays through the pixel-space points (px, py) -- pixel centres are x + 0.5 -- of cameras[view], in the
    camera's dtype. view int64 [n], px / py [n]. -> (origins, dirs) [n, 3]."""
    dtype = cameras.dtype
    px, py = px.to(dtype), py.to(dtype)
    rot = cameras.view_matrix()[:, :3, :3].transpose(1, 2)[view]        # [n, 3, 3] camera to world
    pos = cameras.cam_pos()[view]
    if cameras.lens_type == "pinhole":
        px = px - cameras.x0[view]
        py = py + cameras.y0[view]
    u = 2 * (px / cameras.width) - 1.0
    v = 2 * (py / cameras.height) - 1.0
    zeros = torch.zeros_like(u)
    if cameras.lens_type == "pinhole":
        d_cam = torch.stack((u * cameras.tan_half_fov(CameraFOV.HORIZONTAL)[view],
                             -v * cameras.tan_half_fov(CameraFOV.VERTICAL)[view], -torch.ones_like(u)), dim=-1)
        o_cam = torch.stack((zeros, zeros, zeros), dim=-1)
    else:
        fd = cameras.fov_distance[view]
        d_cam = torch.stack((zeros, zeros, -torch.ones_like(u)), dim=-1)
        o_cam = torch.stack((u * (fd * (cameras.width / cameras.height)), -v * fd, zeros), dim=-1)
    origins = (rot @ o_cam.unsqueeze(-1)).squeeze(-1) + pos
    dirs = (rot @ d_cam.unsqueeze(-1)).squeeze(-1)
    dirs = dirs / torch.linalg.norm(dirs, dim=-1, keepdim=True)
    return origins, dirs


def image_mip_torch(images, mip):
    """``hip_ops.image_mip`` as torch operators, on whatever device the images live: uint8 [..., H, W, C] -> the exact sums of
    the 2^mip x 2^mip blocks, int32 [..., H >> mip, W >> mip, C] (int32 because torch has few operators for uint16; every sum
    fits 16 bits for mip <= 4)."""
    f = 1 << int(mip)
    *lead, H, W, C = images.shape
    if H % f or W % f:
        raise ValueError(f"image_mip_torch: {H} x {W} is not divisible by 2^mip = {f}")
    return images.reshape(*lead, H // f, f, W // f, f, C).to(torch.int32).sum(dim=(-4, -2), dtype=torch.int32)


def composite_colors(pixels, bg_color="white", mip=0):
    """uint8 pixels [n, 3 or 4] -> (rgb fp32 [n, 3], mask bool [n, 1]) by the reference's fp32 chain (wisp/ops/image/io.py:106,
    nerf_standard_dataset.py:415-428). With ``mip`` > 0 the pixels are a mip level's integer block sums (uint16 or any wider
    integer type) and the divisor is 255 * 4^mip: the correctly rounded block mean."""
    # by a TENSOR 255: on the device torch turns a division by a Python scalar into a product with 1 / 255, which is not the
    # correctly rounded quotient the host (where the reference converts its images) and the kernel compute
    full = 255.0 * 4 ** int(mip or 0)
    if pixels.dtype == torch.uint16:
        pixels = pixels.to(torch.int32)
    img = pixels.to(torch.float32) / torch.full((1,), full, dtype=torch.float32, device=pixels.device)
    rgb, alpha = img[..., :3], img[..., 3:4]
    if alpha.numel() == 0 and img.shape[-1] == 3:
        return rgb.contiguous(), torch.ones_like(rgb[..., 0:1]).bool()
    mask = alpha > 0.5
    if bg_color == "black":
        rgb = rgb - (1 - alpha)
    else:
        rgb = rgb * alpha
        rgb = rgb + (1 - alpha)
    return rgb.clamp(0.0, 1.0), mask


def generate_rays(cameras, view_idx=None, pixel_idx=None, jitter=None, images=None, bg_color="white", mip=0):
    """(Rays, rgb, mask) of the pixels ``pixel_idx`` (y * W + x) of the views ``view_idx`` of ``cameras`` (one Camera of V views):
    fp32 origins and unit directions [n, 3], and -- with ``images`` uint8 [V, H, W, 3 or 4] -- the target colours composited over
    ``bg_color`` [n, 3] and the alpha mask [n, 1]; both None without images. Both indices None: every pixel of every view, view
    by view. ``jitter`` [n, 2]: a sub-pixel offset (jx, jy) added to the pixel centres. ``mip`` > 0: ``images`` are the uint16
    block sums of that mip level and the cameras have the level's size. Device tensors run the fused kernel, where an index out
    of range yields a NaN ray; host tensors run the composite in the camera's dtype."""
    if bg_color not in ("white", "black"):
        raise ValueError(f"bg_color must be 'white' or 'black', got {bg_color!r}")
    if cameras.device.type == "cuda":
        W, H = cameras.width, cameras.height
        as_i32 = lambda t: None if t is None else t.to(device=cameras.device, dtype=torch.int32)
        origins, dirs, rgb, mask = hip_ops.raygen(camera_records(cameras), W, H, as_i32(view_idx), as_i32(pixel_idx), jitter,
                                                  images, bg_color, mip=mip)
        return Rays(origins, dirs, dist_min=cameras.near, dist_max=cameras.far), rgb, mask
    return composite_rays(cameras, view_idx, pixel_idx, jitter, images, bg_color, mip=mip)


def composite_rays(cameras, view_idx=None, pixel_idx=None, jitter=None, images=None, bg_color="white", mip=0):
    """``generate_rays`` as a chain of torch operators in the camera's dtype, on whatever device the camera lives: the host path,
    and the yardstick the kernel is measured against (tools/raygen_ab.py)."""
    W, H, dev = cameras.width, cameras.height, cameras.device
    if view_idx is None:
        flat = torch.arange(len(cameras) * H * W, device=dev)
        view_idx, pixel_idx = flat // (H * W), flat % (H * W)
    view_idx, pixel_idx = view_idx.long(), pixel_idx.long()
    px = (pixel_idx % W).to(cameras.dtype) + 0.5
    py = (pixel_idx // W).to(cameras.dtype) + 0.5
    if jitter is not None:
        px, py = px + jitter[:, 0].to(cameras.dtype), py + jitter[:, 1].to(cameras.dtype)
    origins, dirs = _camera_rays(cameras, view_idx, px, py)
    rgb = mask = None
    if images is not None:
        if images.dtype == torch.uint16:                 # torch does not index uint16
            images = images.to(torch.int32)
        rgb, mask = composite_colors(images.reshape(len(cameras), H * W, -1)[view_idx, pixel_idx], bg_color, mip)
    rays = Rays(origins.to(torch.float32), dirs.to(torch.float32), dist_min=cameras.near, dist_max=cameras.far)
    return rays, rgb, mask


def _grid_rays(camera, coords_grid, lens):
    pixel_y, pixel_x = coords_grid
    if camera.device != pixel_y.device or camera.device != pixel_x.device:
        raise Exception(f"Expected camera and coords_grid to be on the same device, but found {camera.device}, "
                        f"{pixel_y.device} and {pixel_x.device}.")
    if camera.lens_type != lens:
        raise ValueError(f"generate_{lens}_rays got a camera with a {camera.lens_type} lens")
    if len(camera) != 1:
        raise ValueError("generate_*_rays takes a single camera; generate_rays takes a batch")
    full = (camera.width, camera.height)
    if (camera.device.type == "cuda" and getattr(pixel_y, "_shacira_full_grid", None) == full
            and getattr(pixel_x, "_shacira_full_grid", None) == full):
        return generate_rays(camera)[0]
    view = torch.zeros(pixel_x.numel(), dtype=torch.long, device=camera.device)
    origins, dirs = _camera_rays(camera, view, pixel_x.reshape(-1), pixel_y.reshape(-1))
    return Rays(origins.to(torch.float32), dirs.to(torch.float32), dist_min=camera.near, dist_max=camera.far)


def generate_pinhole_rays(camera, coords_grid):
    """Rays of a pinhole camera through ``coords_grid`` = (pixel_y, pixel_x), flattened row by row. The principal point is the
    displacement (camera.x0, camera.y0) in pixels from the image centre."""
    return _grid_rays(camera, coords_grid, "pinhole")


def generate_ortho_rays(camera, coords_grid):
    """Parallel rays of an orthographic camera through ``coords_grid``; the principal point is not used."""
    return _grid_rays(camera, coords_grid, "ortho")
