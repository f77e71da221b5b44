"""``WispModule``: nn.Module plus ``name()`` / ``public_properties()`` (reference wisp/core/wisp_module.py:14-46)."""
from abc import ABC, abstractmethod
from typing import Any, Dict

import torch
import torch.nn as nn


class WispModule(nn.Module, ABC):
    def __init__(self):
        super().__init__()

    def name(self) -> str:
        return type(self).__name__

    @abstractmethod
    def public_properties(self) -> Dict[str, Any]:
        raise NotImplementedError("Wisp modules should implement the `public_properties` method")


class Rays:
    """Ray batch: ``origins`` / ``dirs`` [N, 3] and the scalar marching interval (reference wisp/core/rays.py:18-35;
    only what the tracers, the acceleration structure and the offline renderer read)."""

    def __init__(self, origins, dirs, dist_min=0.0, dist_max=float("inf")):
        self.origins, self.dirs, self.dist_min, self.dist_max = origins, dirs, dist_min, dist_max

    @property
    def shape(self):
        return self.origins.shape[:-1]

    def __len__(self):
        return self.origins.shape[0]

    def __getitem__(self, idx):
        return Rays(self.origins[idx], self.dirs[idx], self.dist_min, self.dist_max)

    def to(self, *args, **kwargs):
        return Rays(self.origins.to(*args, **kwargs), self.dirs.to(*args, **kwargs), self.dist_min, self.dist_max)

    def split(self, split_size):
        """Batches of ``split_size`` rays in order; the last one holds the remainder."""
        return [Rays(o, d, self.dist_min, self.dist_max)
                for o, d in zip(torch.split(self.origins, split_size), torch.split(self.dirs, split_size))]

    def reshape(self, *dims):
        return Rays(self.origins.reshape(*dims), self.dirs.reshape(*dims), self.dist_min, self.dist_max)


class RenderBuffer:
    """Multi-channel pixel buffer (reference wisp/core/render_buffer.py): ``rgb``, ``alpha``, ``depth``, ``hit`` and any further
    channel given by keyword or set as an attribute (``xyz``, ``normal``, ``shadow``, ``ao``, ``dirs`` read as None until then).
    The spatial dimensions are free: flat [N, C] while rays are traced in batches, [H, W, C] as an image. A plain attribute bag:
    every method returns a new buffer."""

    xyz = normal = shadow = ao = dirs = None

    def __init__(self, rgb=None, alpha=None, depth=None, hit=None, **extra):
        self.rgb, self.alpha, self.depth, self.hit = rgb, alpha, depth, hit
        for k, v in extra.items():
            setattr(self, k, v)

    @property
    def channels(self):
        """The names of the channels this buffer carries (None-valued ones included)."""
        return {k for k in vars(self) if not k.startswith("_")}

    def __iter__(self):
        return iter((k, v) for k, v in vars(self).items() if not k.startswith("_"))

    @property
    def rgba(self):
        if self.alpha is None or self.rgb is None:
            return None
        return torch.cat((self.rgb, self.alpha), dim=-1)

    def _apply(self, fn):
        return RenderBuffer(**{k: None if v is None else fn(v) for k, v in self})

    @staticmethod
    def _apply_on_pair(rb1, rb2, fn):
        names = list(dict.fromkeys([k for k, _ in rb1] + [k for k, _ in rb2]))
        return RenderBuffer(**{k: fn((getattr(rb1, k, None), getattr(rb2, k, None))) for k in names})

    def __add__(self, other):
        """Concatenation over the first dimension, channel by channel."""
        return self.cat(other)

    def cat(self, other, dim=0):
        """Channel-wise concatenation; a channel that is None (or absent) on one side is taken from the other. A [N] channel
        meets a [N, 1] one as [N, 1]."""
        def _cat(pair):
            a, b = pair
            if a is None or b is None:
                return a if b is None else b
            if a.ndim == b.ndim + 1 and a.shape[-1] == 1:
                b = b.unsqueeze(-1)
            elif b.ndim == a.ndim + 1 and b.shape[-1] == 1:
                a = a.unsqueeze(-1)
            return torch.cat((a, b), dim=dim)
        return RenderBuffer._apply_on_pair(self, other, _cat)

    @staticmethod
    def mean(*rblst):
        """The channel-wise sum over the buffers divided by their number; a None channel counts as zero."""
        def _sum(pair):
            a, b = pair
            if a is None or b is None:
                return a if b is None else b
            return a + b
        rb = RenderBuffer()
        for item in rblst:
            rb = RenderBuffer._apply_on_pair(rb, item, _sum)
        n = float(len(rblst))
        return rb._apply(lambda x: torch.div(x, n))

    def reshape(self, *dims):
        return self._apply(lambda x: x.reshape(*dims))

    def transpose(self):
        """Swaps dimensions 0 and 1 of every channel."""
        return self._apply(lambda x: x.permute(1, 0, *range(2, x.ndim)))

    def to(self, *args, **kwargs):
        return self._apply(lambda x: x.to(*args, **kwargs))

    def cuda(self):
        return self._apply(lambda x: x.cuda())

    def cpu(self):
        return self._apply(lambda x: x.cpu())

    def detach(self):
        return self._apply(lambda x: x.detach())

    def byte(self):
        return self._apply(lambda x: x.byte())

    def float(self):
        return self._apply(lambda x: x.float())

    def numpy_dict(self):
        return {k: v.numpy() for k, v in self if v is not None}

    def image(self):
        """A copy scaled for 8-bit output (call ``.byte()`` on it): rgb and alpha times 255, depth over its maximum (+ 1e-8) as
        grey, hit as black / white, normal mapped from [-1, 1]; hit and normal are present (None) even when the buffer has
        none, every other channel is dropped."""
        def grey(x):
            return torch.cat([x] * 3, dim=-1)
        out = dict()
        if self.rgb is not None:
            out["rgb"] = self.rgb * 255.0
        if self.alpha is not None:
            out["alpha"] = self.alpha * 255.0
        if self.depth is not None:
            out["depth"] = grey(self.depth / (torch.max(self.depth) + 1e-8)) * 255.0
        out["hit"] = grey(self.hit) * 255.0 if self.hit is not None else None
        out["normal"] = ((self.normal + 1.0) / 2.0) * 255.0 if self.normal is not None else None
        return RenderBuffer(**out)


from .camera import Camera, CameraFOV, blender_coords  # noqa: E402,F401
