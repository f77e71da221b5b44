"""Image metrics with the reference's definitions (wisp/ops/image/metrics.py): PSNR (:19-58), the clamped MSE (:60-79), LPIPS
(:81-108, which needs weights this project does not ship) and SSIM (:111-132).

The reference computes SSIM on the host with ``skimage.metrics.structural_similarity(..., data_range=1, gaussian_weights=True,
sigma=1.5, channel_axis=2)``. Here it is a fused HIP kernel on device tensors (``hip_ops.ssim_forward``) and ``ssim_torch``, the
same definition in torch ops, on host tensors and as the fp64 oracle. Parity with skimage is by restatement of its definition
(tests/ssim_ref.py on scipy's ``gaussian_filter``), not by a recorded run of it. ``ssim_loss`` is an addition: the reference has
no differentiable SSIM."""
import math

import torch


def psnr(rgb, gts):
    """10*log10(1/MSE) for images in [0, 1], shape [..., 3]."""
    assert rgb.max() <= 1.05 and rgb.min() >= -0.05
    assert gts.max() <= 1.05 and gts.min() >= -0.05
    assert rgb.shape[-1] == 3 and gts.shape[-1] == 3
    mse = torch.mean((rgb[..., :3] - gts[..., :3]) ** 2).item()
    return 10 * math.log10(1.0 / mse)


def clamped_psnr(rgb, gts):
    """PSNR after clamping to [0,1] and truncating to uint8 levels, as the image trainer reports it."""
    assert gts.max() <= 1.05 and gts.min() >= -0.05
    assert rgb.shape[-1] == 3 and gts.shape[-1] == 3
    q = lambda t: (torch.clamp(t, 0, 1) * 255).to(torch.uint8)[..., :3].float()
    mse = torch.mean((q(rgb) - q(gts)) ** 2).item()
    return 20 * math.log10(255.0) - 10 * math.log10(mse)


def clamped_mse(rgb, gts):
    """MSE after clamping to [0,1] and truncating to uint8 levels (in levels squared)."""
    assert gts.max() <= 1.05 and gts.min() >= -0.05
    assert rgb.shape[-1] == 3 and gts.shape[-1] == 3
    q = lambda t: (torch.clamp(t, 0, 1) * 255).to(torch.uint8)[..., :3].float()
    return torch.mean((q(rgb) - q(gts)) ** 2).item()


def lpips(rgb, gts, lpips_model=None):
    """The reference's LPIPS needs the ``lpips`` package and its VGG weights; neither ships with this project."""
    try:
        from lpips import LPIPS
    except ImportError:
        raise Exception("Module lpips not available. To install, run `pip install lpips`")
    assert rgb.max() <= 1.05 and rgb.min() >= -0.05
    assert gts.max() <= 1.05 and gts.min() >= -0.05
    assert rgb.shape[-1] == 3 and gts.shape[-1] == 3
    if lpips_model is None:
        lpips_model = LPIPS(net="vgg").to(rgb.device)
    return lpips_model((2.0 * rgb[..., :3] - 1.0).permute(2, 0, 1), (2.0 * gts[..., :3] - 1.0).permute(2, 0, 1)).mean().item()


SSIM_SIGMA, SSIM_RADIUS = 1.5, 5        # radius = int(3.5 * sigma + 0.5): skimage's 11-tap window
SSIM_WINDOW = 2 * SSIM_RADIUS + 1


def ssim_window(dtype=torch.float64, device=None):
    """The normalised Gaussian window [11], computed in fp64 as scipy does and then cast."""
    k = torch.arange(-SSIM_RADIUS, SSIM_RADIUS + 1, dtype=torch.float64)
    w = torch.exp(-0.5 / (SSIM_SIGMA * SSIM_SIGMA) * k * k)
    return (w / w.sum()).to(dtype=dtype, device=device)


def _check_ssim_shapes(rgb, gts):
    if rgb.dim() != 3 or gts.dim() != 3 or rgb.shape[:2] != gts.shape[:2]:
        raise RuntimeError(f"ssim expects two [H, W, C] images of one size, got {tuple(rgb.shape)} and {tuple(gts.shape)}")
    if rgb.shape[0] < SSIM_WINDOW or rgb.shape[1] < SSIM_WINDOW:
        raise ValueError(f"win_size exceeds image extent: the {SSIM_WINDOW}-pixel window does not fit a "
                         f"{rgb.shape[0]} x {rgb.shape[1]} image")


def ssim_torch(rgb, gts, data_range=1.0, full=False):
    """SSIM of ``rgb[..., :3]`` against ``gts[..., :3]`` ([H, W, C] tensors) in torch ops, in the dtype of ``rgb``: the definition
    the HIP kernel implements, differentiable, and in fp64 its oracle. Returns the value as a 0-dim fp64 tensor (the valid pixels
    are averaged in fp64, as skimage does); with ``full`` also the per-pixel map [H, W, C] with scipy's 'reflect' borders."""
    import torch.nn.functional as F
    _check_ssim_shapes(rgb, gts)
    x = rgb[..., :3].permute(2, 0, 1).unsqueeze(1)                # [C, 1, H, W]
    y = gts[..., :3].to(dtype=x.dtype, device=x.device).permute(2, 0, 1).unsqueeze(1)
    if x.shape != y.shape:
        raise RuntimeError(f"ssim: channel counts differ: {tuple(rgb.shape)} and {tuple(gts.shape)}")
    r = SSIM_RADIUS
    w = ssim_window(x.dtype, x.device)

    def G(p):   # 'reflect' of scipy (d c b a | a b c d) is numpy's 'symmetric': the border pixel is repeated
        p = torch.cat([p[:, :, :r].flip(2), p, p[:, :, -r:].flip(2)], dim=2)
        p = torch.cat([p[:, :, :, :r].flip(3), p, p[:, :, :, -r:].flip(3)], dim=3)
        return F.conv2d(F.conv2d(p, w.view(1, 1, -1, 1)), w.view(1, 1, 1, -1))

    ux, uy, uxx, uyy, uxy = G(x), G(y), G(x * x), G(y * y), G(x * y)
    cov = SSIM_WINDOW ** 2 / (SSIM_WINDOW ** 2 - 1.0)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    S = S[:, 0]                                                    # [C, H, W]
    value = S[:, r:-r, r:-r].double().mean(dim=(1, 2)).mean()
    return (value, S.permute(1, 2, 0)) if full else value


def _device_pair(rgb, gts):
    """The two images as the kernel reads them and the channel count: buffers of one shape go through as they are (the kernel
    takes the pixel stride, so an RGBA buffer is not copied), otherwise their ``[..., :3]`` copies."""
    _check_ssim_shapes(rgb, gts)
    if rgb.shape != gts.shape or not (rgb.is_contiguous() and gts.is_contiguous()):
        rgb, gts = rgb[..., :3].contiguous(), gts[..., :3].contiguous()
    return rgb.float(), gts.float(), min(3, rgb.shape[-1])


def ssim(rgb, gts):
    """SSIM of two [H, W, 3+] images in [0, 1] over ``[..., :3]`` as a float: the fused HIP kernel on device tensors, ``ssim_torch``
    on host tensors."""
    assert rgb.max() <= 1.05 and rgb.min() >= -0.05
    assert gts.max() <= 1.05 and gts.min() >= -0.05
    if not rgb.is_cuda:
        return ssim_torch(rgb, gts).item()
    from .... import hip_ops
    a, b, c = _device_pair(rgb, gts.to(rgb.device))
    return hip_ops.ssim_forward(a, b, channels=c)[0].item()


def ssim_map(rgb, gts):
    """The per-pixel SSIM [H, W, C] of ``[..., :3]``, borders by reflection (skimage's ``full=True``)."""
    if not rgb.is_cuda:
        return ssim_torch(rgb, gts, full=True)[1]
    from .... import hip_ops
    a, b, c = _device_pair(rgb, gts.to(rgb.device))
    return hip_ops.ssim_forward(a, b, channels=c, with_map=True)[1]


class _SSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, data_range):
        from .... import hip_ops
        pred, target = pred.contiguous(), target.contiguous()
        ctx.save_for_backward(pred, target)
        ctx.data_range = data_range
        value, _ = hip_ops.ssim_forward(pred, target, data_range=data_range)
        return (1.0 - value).to(pred.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        from .... import hip_ops
        pred, target = ctx.saved_tensors
        return hip_ops.ssim_backward(pred, target, -grad_output, data_range=ctx.data_range), None, None


def ssim_loss(pred, target, data_range=1.0):
    """``1 - SSIM`` over all channels of two fp32 [H, W, C] device images as a differentiable 0-dim tensor (gradient with respect
    to ``pred`` only). Two fused kernels forward, two backward; no range asserts and no host read-back, so a training step that
    uses it can be captured into a graph. Not in the reference."""
    return _SSIMLoss.apply(pred, target.detach(), float(data_range))
