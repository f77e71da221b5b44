"""NeRF positional encoding (reference wisp/models/embedders/positional_embedder.py:15-100).

``fused=True`` (an addition; the default is the reference's chain of torch ops) writes the encoding -- and, through ``rows``, the
whole decoder input ``[prefix | encoding]`` -- with ONE HIP kernel (``shacira_posenc_forward``) when the operands are fp32 on the
device and within the kernel's limits; its backward reads the saved sin / cos columns, and is differentiable once more."""
import torch
import torch.nn as nn
from torch.amp import custom_bwd, custom_fwd
from torch.autograd.function import once_differentiable

from .... import _lib, hip_ops


class _PosEncCoordGrad(torch.autograd.Function):
    """grad_coords of the row kernel from its saved row and grad_out; its own backward is ``shacira_posenc_backward2``."""

    @staticmethod
    def forward(ctx, row, grad_out, bands, d, include_input, prefix_width):
        ctx.save_for_backward(row, grad_out, bands)
        ctx.meta = (d, include_input, prefix_width)
        return hip_ops.posenc_backward(row, grad_out, bands, d, include_input, prefix_width)

    @staticmethod
    @once_differentiable
    def backward(ctx, gg):
        row, grad_out, bands = ctx.saved_tensors
        grad_row, grad_grad = hip_ops.posenc_backward2(gg, row, grad_out, bands, *ctx.meta)
        return (grad_row if ctx.needs_input_grad[0] else None, grad_grad if ctx.needs_input_grad[1] else None, None, None,
                None, None)


class _PosEncRows(torch.autograd.Function):
    """[prefix | coords | sin | cos] in one kernel. Saves its OUTPUT: the backward needs the sin / cos columns only."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, prefix, coords, bands, include_input):
        row = hip_ops.posenc_forward(coords, bands, prefix, include_input)
        ctx.save_for_backward(row, bands)
        ctx.meta = (coords.shape[1], include_input, 0 if prefix is None else prefix.shape[1])
        return row

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad):
        row, bands = ctx.saved_tensors
        d, include_input, P = ctx.meta
        g_prefix = grad[:, :P] if ctx.needs_input_grad[0] else None       # the view itself: no kernel
        g_coords = _PosEncCoordGrad.apply(row, grad, bands, d, include_input, P) if ctx.needs_input_grad[1] else None
        return g_prefix, g_coords, None, None


class PositionalEmbedder(nn.Module):
    """coords [N, d] -> [coords,] sin(coords * 2^k), cos(coords * 2^k) for k log-spaced in [0, max_freq_log2]: all
    sines first, then all cosines, frequency-major inside each (the reference's layout)."""

    def __init__(self, num_freq, max_freq_log2, log_sampling=True, include_input=True, input_dim=3, fused=False):
        super().__init__()
        self.num_freq, self.max_freq_log2 = num_freq, max_freq_log2
        self.log_sampling, self.include_input = log_sampling, include_input
        self.fused = fused
        bands = 2.0 ** torch.linspace(0.0, max_freq_log2, steps=num_freq) if log_sampling \
            else torch.linspace(1, 2.0 ** max_freq_log2, steps=num_freq)
        self.out_dim = (input_dim if include_input else 0) + bands.shape[0] * input_dim * 2
        self.bands = nn.Parameter(bands).requires_grad_(False)

    def _takes_kernel(self, coords, prefix=None):
        """The row kernel's operands: fp32 coords [N, 1..4] and the bands on one device, at most 64 bands; a prefix [N, P] on
        that device, fp32 (any float type under autocast, which hands the kernel an fp32 copy)."""
        if not (self.fused and coords.is_cuda and coords.dtype == torch.float32 and coords.dim() == 2):
            return False
        if not (1 <= coords.shape[1] <= _lib.POSENC_MAX_DIM and 1 <= self.bands.numel() <= _lib.POSENC_MAX_BANDS
                and self.bands.device == coords.device and self.bands.dtype == torch.float32):
            return False
        if prefix is None:
            return True
        if not (prefix.is_cuda and prefix.device == coords.device and prefix.dim() == 2 and prefix.shape[0] == coords.shape[0]
                and prefix.shape[1] <= _lib.POSENC_MAX_PREFIX and prefix.is_floating_point()):
            return False
        return prefix.dtype == torch.float32 or (torch.is_autocast_enabled("cuda") and prefix.dtype != torch.float64)

    def forward(self, coords):
        if self._takes_kernel(coords):
            return _PosEncRows.apply(None, coords, self.bands, self.include_input)
        n = coords.shape[0]
        winded = (coords[:, None] * self.bands[None, :, None]).reshape(n, coords.shape[1] * self.num_freq)
        encoded = torch.cat([torch.sin(winded), torch.cos(winded)], dim=-1)
        return torch.cat([coords, encoded], dim=-1) if self.include_input else encoded

    def rows(self, prefix, coords):
        """``[prefix | self(coords)]`` [N, P + out_dim]: the decoder's input row."""
        if self._takes_kernel(coords, prefix):
            return _PosEncRows.apply(prefix, coords, self.bands, self.include_input)
        return torch.cat([prefix, self(coords)], dim=-1)


def get_positional_embedder(frequencies, input_dim=3, include_input=True, fused=False):
    encoder = PositionalEmbedder(frequencies, frequencies - 1, input_dim=input_dim, include_input=include_input, fused=fused)
    return encoder, encoder.out_dim
