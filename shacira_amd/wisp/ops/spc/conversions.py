"""Meshes and point clouds to occupancy (reference wisp/ops/spc/conversions.py)."""
import torch

from ...accelstructs import OctreeAS
from .processing import dilate_points, morton_sorted_unique


def mesh_to_octree(vertices: torch.Tensor, faces: torch.Tensor, level: int, num_samples: int = None,
                   margin: float = 0.5) -> OctreeAS:
    """The ``OctreeAS`` of the cells of ``level`` that the mesh touches (``OctreeAS.from_triangles``; GPU tensors).

    The reference throws ``num_samples`` random surface samples plus a copy jittered by +-1 / 2^(level + 1) in cube
    coordinates -- a quarter of a cell -- and quantises them; here every triangle is rasterised against the cells with an
    exact overlap test: a cell is set iff a triangle overlaps the closed cube of half-extent ``0.5 + margin`` cells around
    its centre. The reference's sampling converges to the set of ``margin = 0.25``; the default 0.5 is a superset of it, about
    a third larger (more cells to trace, more corner rows): pass ``margin=0.25`` for the reference's band, 0 for the cells the
    surface touches. ``num_samples`` is accepted and ignored. Deviations: the return is an ``OctreeAS``, not kaolin's byte tensor, and
    geometry outside [-1, 1]^3 marks nothing (the reference clamps outside samples into the border cells)."""
    return OctreeAS.from_triangles(vertices, faces, level, margin=margin)


def pointcloud_to_octree(pointcloud: torch.Tensor, level: int, attributes: torch.Tensor = None, dilate: int = 0):
    """The ``OctreeAS`` of the cells of ``level`` holding a point of ``pointcloud`` [N, 3] in [-1, 1]^3 (quantised by
    ``OctreeAS.quantize_pointcloud``, as ``from_pointcloud`` does; points that are not finite are dropped), grown ``dilate`` times by
    ``dilate_points``. With ``attributes`` [N, F]: also their per-cell means, float [cells, F] in the Morton order of
    ``OctreeAS.points``; as in the reference, the means are those of the cells BEFORE dilation."""
    points, keep = OctreeAS.quantize_pointcloud(pointcloud, level)
    cells, inverse = morton_sorted_unique(points, level)
    grown = cells
    for _ in range(dilate):
        grown = dilate_points(grown, level)
    blas = OctreeAS.from_quantized_points(grown, level)
    if attributes is None:
        return blas
    att = attributes[keep].float()
    sums = torch.zeros((cells.shape[0], att.shape[1]), dtype=torch.float32, device=att.device).index_add_(0, inverse, att)
    counts = torch.bincount(inverse, minlength=cells.shape[0]).to(torch.float32)
    return blas, sums / counts[:, None]
