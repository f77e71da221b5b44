"""``OctreeGrid``: a multiscale feature grid whose features sit on the corners of the occupied cells of an octree.

Mirror of reference wisp/models/grids/octree_grid.py: the same constructor arguments and attributes (``feature_dim``,
``base_lod``, ``num_lods``, ``active_lods``, ``max_lod``, ``interpolation_type``, ``multiscale_type``, ``feature_std``,
``feature_bias``, ``num_feat``), ``features`` as a ``ParameterList`` of [C_l + 1, F] tables drawn as ``zeros + bias`` then
``+= randn * std`` in level order, the same classmethods and the same ``interpolate`` shapes. The lookup runs in the HIP
kernels of ``wisp.ops.octree``; like ``HashGrid``, the module builds and loads on the host, and ``interpolate`` on host
tensors raises.

Differences, all stated:
  * the occupied set is ``OctreeAS``'s dense bit grid, not kaolin's point hierarchy. ``points_dual`` and ``trinkets`` are
    dictionaries keyed by the active level (the reference holds one tensor over its whole pyramid), and the rows of a table
    follow ``points_dual[l]``: ascending linear key (x * S + y) * S + z (``wisp.ops.octree``). That is not kaolin's order, so
    a reference checkpoint does not load;
  * the reference casts the table to fp16 for kaolin's kernel; the lookup here is fp32;
  * ``interpolation_type='closest'``, ``from_mesh`` and ``from_spc`` raise ``NotImplementedError``; a mesh comes in
    through ``from_triangles`` (``load_obj`` -> ``normalize(..., 'sphere')`` -> ``from_triangles``), rasterised exactly
    where the reference samples;
  * when ``self.blas`` is replaced (``OctreeAS.from_quantized_points`` on a new cell set), the next ``interpolate``
    rebuilds the index and carries every surviving corner's row over into new tables; corners that were not there before
    start at ``feature_bias``. The ``Parameter`` objects are replaced, so an optimizer has to be rebuilt after that (a
    warning is logged). Only a replaced ``self.blas`` object is noticed: after writing into its ``occupancy_grid`` in
    place, call ``blas.occupancy_changed()`` and ``grid.refresh_index(force=True)``.
"""
import logging as log
from typing import Any, Dict, Set, Type

import torch
import torch.nn as nn

from ...accelstructs import ASRaymarchResults, ASRaytraceResults, BaseAS, OctreeAS
from ...ops import octree as octree_ops
from .blas_grid import BLASGrid


class OctreeGrid(BLASGrid):
    def __init__(self, accelstruct: OctreeAS, feature_dim: int, base_lod: int, num_lods: int = 1,
                 interpolation_type: str = "linear", multiscale_type: str = "cat", feature_std: float = 0.0,
                 feature_bias: float = 0.0):
        super().__init__(accelstruct)
        self.feature_dim = feature_dim
        self.base_lod = base_lod
        self.num_lods = num_lods
        self.interpolation_type = interpolation_type
        self.multiscale_type = multiscale_type
        self.feature_std = feature_std
        self.feature_bias = feature_bias
        self.active_lods = [self.base_lod + x for x in range(self.num_lods)]
        self.max_lod = OctreeGrid.max_octree_lod(self.base_lod, self.num_lods)
        log.info(f"Active LODs: {self.active_lods}")
        self.num_feat = 0
        self.index = None
        if self.interpolation_type == "closest":
            raise NotImplementedError("interpolation_type='closest' is not implemented: no shipped configuration uses it")
        if self.interpolation_type != "linear":
            raise Exception(f"Interpolation mode {self.interpolation_type} is not supported.")
        if self.max_lod > self.blas.max_level:
            raise ValueError(f"the acceleration structure has {self.blas.max_level} levels, the grid needs {self.max_lod}")
        if self.num_lods > 0:
            self.init_feature_structure()

    @staticmethod
    def max_octree_lod(base_lod, num_lods) -> int:
        return base_lod + num_lods - 1

    @classmethod
    def make_dense(cls, feature_dim: int, base_lod: int, num_lods: int = 1, **kwargs):
        """A fully occupied grid with ``base_lod + num_lods - 1`` levels."""
        blas = OctreeAS.make_dense(level=OctreeGrid.max_octree_lod(base_lod, num_lods))
        return cls(accelstruct=blas, feature_dim=feature_dim, base_lod=base_lod, num_lods=num_lods, **kwargs)

    @classmethod
    def from_pointcloud(cls, pointcloud: torch.Tensor, feature_dim: int, base_lod: int, num_lods: int = 1, **kwargs):
        """Occupied cells = the cells of the finest level that hold a point of ``pointcloud`` [N, 3] in [-1, 1]^3."""
        blas = OctreeAS.from_pointcloud(pointcloud, level=OctreeGrid.max_octree_lod(base_lod, num_lods))
        return cls(accelstruct=blas, feature_dim=feature_dim, base_lod=base_lod, num_lods=num_lods, **kwargs)

    @classmethod
    def from_quantized_points(cls, quantized_points: torch.Tensor, feature_dim: int, base_lod: int, num_lods: int = 1,
                              **kwargs):
        """Occupied cells = the integer cells [N, 3] of the finest level."""
        blas = OctreeAS.from_quantized_points(quantized_points, level=OctreeGrid.max_octree_lod(base_lod, num_lods))
        return cls(accelstruct=blas, feature_dim=feature_dim, base_lod=base_lod, num_lods=num_lods, **kwargs)

    @classmethod
    def from_triangles(cls, vertices: torch.Tensor, faces: torch.Tensor, feature_dim: int, base_lod: int, num_lods: int = 1,
                       margin: float = 0.5, **kwargs):
        """Occupied cells = the cells of the finest level that the mesh touches (``OctreeAS.from_triangles``; GPU tensors)."""
        blas = OctreeAS.from_triangles(vertices, faces, level=OctreeGrid.max_octree_lod(base_lod, num_lods), margin=margin)
        return cls(accelstruct=blas, feature_dim=feature_dim, base_lod=base_lod, num_lods=num_lods, **kwargs)

    @classmethod
    def from_mesh(cls, *args, **kwargs):
        return OctreeAS.from_mesh(*args, **kwargs)     # raises, naming the way: load_obj, normalize, from_triangles

    @classmethod
    def from_spc(cls, *args, **kwargs):
        return OctreeAS.from_spc(*args, **kwargs)      # raises, naming the reason

    # ---- the corner index -------------------------------------------------------------------------------------------------
    @property
    def points_dual(self) -> Dict[int, torch.Tensor]:
        return {l: self.index[l].points_dual for l in self.active_lods}

    @property
    def trinkets(self) -> Dict[int, torch.Tensor]:
        return {l: self.index[l].trinkets for l in self.active_lods}

    def _new_row_value(self) -> float:
        return self.feature_bias

    def _draw_tables(self, rows):
        self.features = nn.ParameterList([])
        for n in rows:
            fts = torch.zeros(n, self.feature_dim) + self.feature_bias
            fts += torch.randn_like(fts) * self.feature_std
            self.features.append(nn.Parameter(fts))

    def init_feature_structure(self):
        self.index = octree_ops.build_octree_index(self.blas, self.active_lods)
        log.info("Built the corner index")
        fpyramid = [self.index[l].rows + 1 for l in self.active_lods]
        self.num_feat = sum(fpyramid)
        log.info(f"# Feature Vectors: {self.num_feat}")
        self._draw_tables(fpyramid)

    def refresh_index(self, force: bool = False):
        """After ``self.blas`` was replaced (or with ``force``): a new index, and tables that keep the rows of the surviving
        corners."""
        if self.index.source is self.blas and not force:
            return
        log.warning("OctreeGrid: the occupancy changed, the corner index was rebuilt and the feature tables were replaced "
                    "by new Parameters: rebuild any optimizer that holds the old ones")
        old, new = self.index, octree_ops.build_octree_index(self.blas, self.active_lods)
        with torch.no_grad():
            for i, l in enumerate(self.active_lods):
                param = self.features[i]
                ok, nk = old[l].corner_keys().to(param.device), new[l].corner_keys().to(param.device)
                table = torch.full((nk.shape[0] + 1, param.shape[1]), float(self._new_row_value()), dtype=param.dtype,
                                   device=param.device)
                table[-1] = param[-1]
                if ok.shape[0] > 0 and nk.shape[0] > 0:
                    pos = torch.searchsorted(ok, nk).clamp(max=ok.shape[0] - 1)
                    found = ok[pos] == nk
                    table[:-1][found] = param[pos[found]]
                self.features[i] = nn.Parameter(table, requires_grad=param.requires_grad)
        self.index = new
        self.num_feat = sum(new[l].rows + 1 for l in self.active_lods)

    def freeze(self):
        for lod_idx in range(self.num_lods):
            self.features[lod_idx].requires_grad_(False)

    def _tables(self, num_feats):
        """The [C_l + 1, F] tables of levels 0..num_feats-1 handed to the lookup."""
        return [self.features[i] for i in range(num_feats)]

    def interpolate(self, coords, lod_idx):
        """coords [B, S, 3] or [B, 3], levels 0..lod_idx of ``active_lods`` -> [B, S, K] / [B, K] with K = F for 'sum' and
        for lod_idx == 0, (lod_idx + 1) * F for 'cat'."""
        output_shape = coords.shape[:-1]
        self.refresh_index()
        num_feats = lod_idx + 1
        lods = self.active_lods[:num_feats]
        summed = self.multiscale_type == "sum"
        feats = octree_ops.octree_interpolate(coords.reshape(-1, 3), lods, self._tables(num_feats), self.index, summed)
        return feats.reshape(*output_shape, feats.shape[-1])

    def raymarch(self, rays, raymarch_type, num_samples, level=None, seed=None, step=0) -> ASRaymarchResults:
        """Samples over the coarsest level that has features, as the reference does."""
        return self.blas.raymarch(rays, raymarch_type=raymarch_type, num_samples=num_samples, level=self.base_lod, seed=seed,
                                  step=step)

    def raytrace(self, rays, level=None, with_exit=False) -> ASRaytraceResults:
        return self.blas.raytrace(rays, level=level, with_exit=with_exit)

    def supported_blas(self) -> Set[Type[BaseAS]]:
        return {OctreeAS}

    def name(self) -> str:
        return "Octree Grid"

    def public_properties(self) -> Dict[str, Any]:
        properties = {
            "Feature Dims": self.feature_dim,
            "Total LODs": self.max_lod,
            "Active feature LODs": [str(x) for x in self.active_lods],
            "Interpolation": self.interpolation_type,
            "Multiscale aggregation": self.multiscale_type,
        }
        return {**super().public_properties(), **properties}
