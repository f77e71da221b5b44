"""``TriplanarGrid``: a pyramid of triplanes (three orthogonal feature planes per LOD) behind the ``BLASGrid`` interface.

Mirror of reference wisp/models/grids/triplanar_grid.py: the same constructor, attributes (``feature_dim`` = 3 x the
argument, ``active_lods``, ``max_lod``, ``num_lods``, the reference's ``num_feat`` count), ``features`` ModuleList of
``TriplanarFeatureVolume`` with parameters ``fmx`` / ``fmy`` / ``fmz`` [1, F, 2^lod + 1, 2^lod + 1] drawn in that order per
LOD (state_dict keys, shapes and RNG draws match: a reference checkpoint loads unchanged), and the same ``interpolate``
output shapes, the [B, 3] 'cat' case's [B, 1, K] included. The sampling runs in the HIP kernels of ``wisp.ops.triplane``;
like ``HashGrid``, the module builds and loads on the host, and ``interpolate`` on host tensors raises.

One deviation: the reference's ``TriplanarFeatureVolume.forward`` raises ``TypeError`` on an [N, 3] input (a misspelt
``padding_modes`` keyword); the mirror returns the intended [N, 3, F].
"""
import logging as log
from typing import Any, Dict, Set, Type

import torch
import torch.nn as nn

from ...accelstructs import ASRaymarchResults, ASRaytraceResults, AxisAlignedBBoxAS, BaseAS
from ...core import WispModule
from ...ops import triplane as triplane_ops
from .blas_grid import BLASGrid


class TriplanarGrid(BLASGrid):
    def __init__(self, feature_dim: int, base_lod: int, num_lods: int = 1, interpolation_type: str = "linear",
                 multiscale_type: str = "sum", feature_std: float = 0.0, feature_bias: float = 0.0):
        super().__init__(blas=AxisAlignedBBoxAS())
        self.feature_dim = feature_dim * 3          # three planes per LOD
        self.base_lod = base_lod
        self.num_lods = num_lods
        self.interpolation_type = interpolation_type
        self.multiscale_type = multiscale_type
        self.feature_std = feature_std
        self.feature_bias = feature_bias
        self.active_lods = [self.base_lod + x for x in range(self.num_lods)]
        self.max_lod = self.num_lods + self.base_lod - 1
        log.info(f"Active LODs: {self.active_lods}")
        self.num_feat = 0
        self.init_feature_structure()

    def init_feature_structure(self):
        self.features = nn.ModuleList([])
        self.num_feat = 0
        for lod in self.active_lods:
            self.features.append(TriplanarFeatureVolume(self.feature_dim // 3, 2 ** lod, self.feature_std,
                                                        self.feature_bias))
            self.num_feat += ((2 ** lod + 1) ** 2) * self.feature_dim * 3   # the reference's count (3F counted 3 times)
        log.info(f"# Feature Vectors: {self.num_feat}")

    def freeze(self):
        self.features.requires_grad_(False)

    def interpolate(self, coords, lod_idx):
        """coords [B, S, 3] or [B, 3], LODs 0..lod_idx -> 'sum': [B, S, 3F] / [B, 3F]; 'cat': [B, S, (lod_idx+1) * 3F] and,
        for [B, 3] input, [B, 1, (lod_idx+1) * 3F] (the reference's shapes)."""
        if self.interpolation_type != "linear":
            raise ValueError(f"Interpolation mode '{self.interpolation_type}' is not supported")
        output_shape = coords.shape[:-1]
        if coords.ndim < 3:
            coords = coords[:, None]
        batch, num_samples = coords.shape[:2]
        vols = list(self.features)[:lod_idx + 1]
        planes = [t for v in vols for t in (v.fmx, v.fmy, v.fmz)]
        lods = [self.active_lods[i] for i in range(len(vols))]
        summed = self.multiscale_type == "sum"
        feats = triplane_ops.triplane_interpolate(coords.reshape(batch * num_samples, 3), lods, planes, summed)
        if summed:
            return feats.reshape(*output_shape, feats.shape[-1])
        return feats.reshape(batch, num_samples, feats.shape[-1])

    def raymarch(self, rays, raymarch_type, num_samples, level=None, seed=None, step=0) -> ASRaymarchResults:
        return self.blas.raymarch(rays, raymarch_type=raymarch_type, num_samples=num_samples, level=0, seed=seed,
                                  step=step)

    def raytrace(self, rays, level=None, with_exit=False) -> ASRaytraceResults:
        return self.blas.raytrace(rays, level=0, with_exit=with_exit)

    def supported_blas(self) -> Set[Type[BaseAS]]:
        return {AxisAlignedBBoxAS}

    def name(self) -> str:
        return "Triplanar Grid"

    def public_properties(self) -> Dict[str, Any]:
        properties = {
            "Feature Dims": self.feature_dim,
            "Total LODs": self.max_lod,
            "Active feature LODs": [str(x) for x in self.active_lods],
            "Interpolation": self.interpolation_type,
            "Multiscale aggregation": self.multiscale_type,
        }
        for idx, module in enumerate(self.features):
            properties[f"Pyramid Layer #{idx + 1}"] = module
        return {**super().public_properties(), **properties}


class TriplanarFeatureVolume(WispModule):
    """One LOD: planes fmx (read at y, z), fmy (x, z), fmz (x, y), each [1, fdim, fsize + 1, fsize + 1]."""

    def __init__(self, fdim, fsize, std, bias):
        super().__init__()
        self.fsize = fsize
        self.fdim = fdim
        self.fmx = nn.Parameter(torch.randn(1, fdim, fsize + 1, fsize + 1) * std + bias)
        self.fmy = nn.Parameter(torch.randn(1, fdim, fsize + 1, fsize + 1) * std + bias)
        self.fmz = nn.Parameter(torch.randn(1, fdim, fsize + 1, fsize + 1) * std + bias)
        self.padding_mode = "reflection"

    def forward(self, x):
        """x [B, S, 3] -> [B, S, 3, fdim]; x [N, 3] -> [N, 3, fdim]."""
        lod = self.fsize.bit_length() - 1
        flat = x.reshape(-1, 3)
        feats = triplane_ops.triplane_interpolate(flat, [lod], [self.fmx, self.fmy, self.fmz], True)
        return feats.reshape(*x.shape[:-1], 3, self.fdim)

    def name(self) -> str:
        return "TriplanarFeatureVolume"

    def public_properties(self) -> Dict[str, Any]:
        return {"Resolution": f"3x{self.fsize}x{self.fsize}"}
