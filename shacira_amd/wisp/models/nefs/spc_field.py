"""``SPCField``: a structured point cloud rendered with its own per-cell colours -- no embedder, no decoder (reference
wisp/models/nefs/spc_field.py). The topology is a ``StructuredPointCloud`` (``wisp.ops.spc``; its colours come with it) or an
``OctreeAS`` with ``features_dict``:
    'colors'   uint8 [cells, 4] in the Morton order of ``OctreeAS.points`` -> colour = byte / 255
    'normals'  float [cells, 3]                                             -> colour = 0.5 (n + 1)
    neither                                                                  -> the cell's coordinates / 2^L, as the reference
``rgba(ridx_hit)`` takes Morton indices of the finest level's cells as this package's tracers write them (``pidx``): they
carry no pyramid offset, where the reference subtracts the finest level's offset in kaolin's point hierarchy."""
import torch
import torch.nn as nn

from ...accelstructs import OctreeAS, _morton_index
from ...ops.spc.structured import StructuredPointCloud
from ..grids.blas_grid import BLASGrid


class _TopologyGrid(BLASGrid):
    """A grid with an acceleration structure and no features: SPC fields keep their features themselves."""

    def interpolate(self, coords, lod_idx):
        raise NotImplementedError("an SPCField has no interpolated features: its colours are per cell (rgba)")


class SPCField(nn.Module):
    def __init__(self, spc, features_dict=None, device=None):
        super().__init__()
        self.features_dict = dict(features_dict) if features_dict is not None else dict()
        self.spc = spc if isinstance(spc, StructuredPointCloud) else None
        if self.spc is not None:
            blas = spc.to_octree_as()
            if spc.colors is not None and "colors" not in self.features_dict:
                self.features_dict["colors"] = spc.colors_morton()
        elif isinstance(spc, OctreeAS):
            blas = spc
        else:
            raise TypeError(f"SPCField takes a StructuredPointCloud or an OctreeAS, got {type(spc).__name__}")
        self.spc_device = torch.device(device) if device is not None else blas.occupancy_grid.device
        cells = blas.points.shape[0]
        self.normals = None
        if "normals" in self.features_dict:
            self.normals = self.features_dict["normals"].reshape(-1, 3).to(self.spc_device)
        if "colors" in self.features_dict:
            # by a TENSOR 255: on the device torch turns a division by a Python scalar into a product with 1 / 255, which is
            # not the correctly rounded quotient the first-hit kernel writes
            colors = self.features_dict["colors"].reshape(-1, 4).to(self.spc_device).float()
            colors = colors / torch.full((1,), 255.0, device=colors.device)
        elif self.normals is not None:
            colors = 0.5 * (self.normals.float() + 1.0)
        else:
            colors = blas.points.to(self.spc_device).float() / float(1 << blas.max_level)
        if colors.shape[0] != cells:
            raise ValueError(f"SPCField: {colors.shape[0]} feature rows for {cells} cells")
        self.colors = colors
        self._codes = _morton_index(blas.points.to(self.spc_device), blas.max_level)      # ascending: points are in Morton order
        self.grid = _TopologyGrid(blas)
        self._forward_functions = {"rgb": self.rgba}

    @property
    def device(self):
        return self.spc_device

    def get_supported_channels(self):
        return set(self._forward_functions)

    def get_forward_function(self, channel):
        if channel not in self._forward_functions:
            raise Exception(f"Channel {channel} is not supported in {self.__class__.__name__}")
        fn = self._forward_functions[channel]
        return lambda *args, **kwargs: fn(*args, **kwargs)[channel]

    def forward(self, channels=None, **kwargs):
        """Dict of the requested channels; a single channel name returns its tensor, as the other fields do."""
        requested = {channels} if isinstance(channels, str) else set(self._forward_functions if channels is None else channels)
        unsupported = requested - self.get_supported_channels()
        if unsupported:
            raise Exception(f"Channels {unsupported} are not supported in {self.__class__.__name__}")
        out = self.rgba(**kwargs)
        if isinstance(channels, str):
            return out[channels]
        return out if channels is None else {c: out[c] for c in channels}

    def rgba(self, ridx_hit=None):
        """ridx_hit: Morton indices [B] of occupied cells of the finest level -> dict(rgb=[B, 1, 3])."""
        rows = torch.searchsorted(self._codes, ridx_hit.long().to(self._codes.device))
        rows = rows.clamp(max=max(self._codes.shape[0] - 1, 0))
        return dict(rgb=self.colors[rows, :3].unsqueeze(1))

    def public_properties(self):
        return {"Grid": self.grid}
