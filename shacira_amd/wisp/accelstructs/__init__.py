"""Kaolin-free stand-in for the occupancy structure the grids carry (reference: wisp/accelstructs/octree_as.py,
used by hash_grid.py:60-66 / latent_grid.py:70-76 through ``OctreeAS.make_dense``).

One dense occupancy level with Morton-ordered cell coordinates (``points``) so that ``dense_points`` / ``num_cells``
/ ``occupancy`` have the reference's shapes, plus -- SURVEY.md section 8 "next" row f2 -- the queries the NeRF pipeline
makes of it: ``query``, ``raytrace``, ``raymarch`` ('ray' and 'voxel', octree_as.py:129-307) and
``from_quantized_points`` (pruning, nerf.py:150-185), and ``from_triangles``, the mesh rasterised by mesh_voxelize.hip. The reference answers them with kaolin's sparse-octree CUDA
(un-vendored); here the occupied set is a dense [G, G, G] bit grid walked by the HIP kernels of render.hip.
``pidx`` values are Morton indices of the level's cells (the reference's index into its SPC point hierarchy).

Coarser levels (the octree feature grids ask for them): a cell of level l < ``max_level`` is occupied if any cell of
``max_level`` inside it is. The reduced grids are OR-reductions of the bit grid, cached per level and per device. The cache
is dropped when ``occupancy_grid`` is replaced by another tensor (a new structure from ``from_quantized_points``, a move to
another device); code that writes INTO the tensor in place must call ``occupancy_changed()`` itself, as
``harness.GraphedNerfFitter.after_prune`` does; ``query`` / ``raytrace`` / ``raymarch`` / ``level_points`` take any level in
0..max_level with the same conventions (``pidx``: Morton index of the cell at that level, -1 if unoccupied or outside).
``points`` and ``pyramid`` keep describing ``max_level`` only.
"""
from collections import namedtuple

import torch

ASQueryResults = namedtuple("ASQueryResults", ["pidx"])
ASRaytraceResults = namedtuple("ASRaytraceResults", ["ridx", "pidx", "depth"])
ASRaymarchResults = namedtuple("ASRaymarchResults", ["ridx", "samples", "depth_samples", "deltas", "boundary",
                                                     "ray_offsets"], defaults=[None])


def _morton_points(level: int) -> torch.Tensor:
    """All (x, y, z) cells of a 2^level cube in Morton order (x is the most significant of each bit triple)."""
    n = 1 << (3 * level)
    code = torch.arange(n, dtype=torch.int64)
    xyz = torch.zeros(n, 3, dtype=torch.int64)
    for b in range(level):
        xyz[:, 0] |= ((code >> (3 * b + 2)) & 1) << b
        xyz[:, 1] |= ((code >> (3 * b + 1)) & 1) << b
        xyz[:, 2] |= ((code >> (3 * b + 0)) & 1) << b
    return xyz.to(torch.int16)


def _morton_index(q: torch.Tensor, level: int) -> torch.Tensor:
    """int cells [N, 3] -> Morton index (x most significant of each bit triple), the row of ``_morton_points``."""
    q = q.long()
    m = torch.zeros(q.shape[0], dtype=torch.int64, device=q.device)
    for b in range(level):
        m |= (((q[:, 0] >> b) & 1) << (3 * b + 2)) | (((q[:, 1] >> b) & 1) << (3 * b + 1)) | (((q[:, 2] >> b) & 1) << (3 * b))
    return m


class BaseAS:
    def raymarch(self, *args, **kwargs):
        raise NotImplementedError

    def raytrace(self, *args, **kwargs):
        raise NotImplementedError

    def query(self, *args, **kwargs):
        raise NotImplementedError


class OctreeAS(BaseAS):
    """Occupancy at one level. ``points`` holds the occupied cells of ``level`` in Morton order (the reference's SPC
    holds the whole pyramid; the grids only ever ask for the cells of ``blas_level``); ``occupancy_grid`` is the same
    set as a dense bool [G, G, G] indexed [x][y][z]."""

    def __init__(self, level: int, occupancy_grid: torch.Tensor = None):
        self.max_level = level
        G = 1 << level
        if occupancy_grid is None:
            self.points = _morton_points(level)
            self.occupancy_grid = torch.ones((G, G, G), dtype=torch.bool)
        else:
            self.occupancy_grid = occupancy_grid.bool()
            cells = torch.nonzero(self.occupancy_grid)
            order = torch.argsort(_morton_index(cells, level))
            self.points = cells[order].to(torch.int16)
        self.pyramid = torch.tensor([[self.points.shape[0]], [0]], dtype=torch.int32)
        self.extent = dict()

    @classmethod
    def make_dense(cls, level: int):
        return cls(level)

    @classmethod
    def from_quantized_points(cls, quantized_points: torch.Tensor, level: int):
        """Occupied set = the given integer cells [N, 3] (reference octree_as.py `from_quantized_points`)."""
        G = 1 << level
        grid = torch.zeros((G, G, G), dtype=torch.bool, device=quantized_points.device)
        q = quantized_points.long()
        grid[q[:, 0], q[:, 1], q[:, 2]] = True
        return cls(level, grid)

    @staticmethod
    def quantize_pointcloud(pointcloud: torch.Tensor, level: int):
        """(cells int64 [M, 3], keep bool [N]): the cell of ``level`` of every finite point of ``pointcloud`` [N, 3] in
        [-1, 1]^3, ``query``'s floor(G * (x + 1) / 2) clamped into the grid as kaolin's ``quantize_points`` does (a point on a
        far face, x = 1, falls into the last cell); ``keep`` marks the points that are finite, the rows of ``cells``."""
        G = 1 << level
        cell = torch.floor(G * (pointcloud.float() + 1.0) / 2.0)
        keep = torch.isfinite(cell).all(dim=-1)
        return cell[keep].clamp(0, G - 1).long(), keep

    @classmethod
    def from_pointcloud(cls, pointcloud: torch.Tensor, level: int):
        """Occupied set = the cells of ``level`` holding a point of ``pointcloud`` [N, 3] in [-1, 1]^3
        (``quantize_pointcloud``). Points that are not finite are dropped."""
        return cls.from_quantized_points(cls.quantize_pointcloud(pointcloud, level)[0], level)

    @classmethod
    def from_triangles(cls, vertices: torch.Tensor, faces: torch.Tensor, level: int, margin: float = 0.5):
        """Occupied set = the cells of ``level`` that the mesh (``vertices`` [V, 3] in [-1, 1]^3, ``faces`` [F, 3]) touches:
        a cell is set iff a non-degenerate triangle overlaps the closed cube of half-extent ``0.5 + margin`` cells around
        its centre (the HIP rasteriser of mesh_voxelize.hip; contract: include/shacira_hip.h, shacira_mesh_voxelize).
        Deterministic and free of holes. The reference's ``from_mesh`` samples instead: surface samples plus a copy jittered
        by +-1 / 2^(level + 1) in cube coordinates, a QUARTER of a cell, whose limit is the set of ``margin = 0.25``; the
        default ``margin = 0.5`` is a superset of it, about a third larger. Geometry outside the cube marks nothing where
        the reference clamps it into the border cells. ``vertices`` and ``faces`` are kept in ``extent``, as the reference's
        ``from_mesh`` keeps them; the tensors must be on the GPU."""
        from ... import hip_ops
        hip_ops._need_gpu(vertices, faces)
        words, grid = hip_ops.mesh_voxelize(vertices[faces.long()], level, margin)
        blas = cls(level, grid)
        blas._packed = (blas.occupancy_grid, words)
        blas.extent["vertices"] = vertices
        blas.extent["faces"] = faces
        return blas

    @classmethod
    def from_mesh(cls, *args, **kwargs):
        raise NotImplementedError("OctreeAS.from_mesh(path) is not implemented: load the mesh with wisp.ops.mesh.load_obj, "
                                  "normalize(vertices, faces, 'sphere') it, move it to the GPU and call "
                                  "OctreeAS.from_triangles(vertices, faces, level)")

    @classmethod
    def from_spc(cls, *args, **kwargs):
        raise NotImplementedError("OctreeAS.from_spc reads kaolin's byte octree, which this dense bit grid does not "
                                  "hold: use from_quantized_points with the cells of the finest level")

    def _grid_on(self, device):
        if self.occupancy_grid.device != device:
            self.occupancy_grid = self.occupancy_grid.to(device)
        return self.occupancy_grid

    def _level(self, level):
        if level is None:
            return self.max_level
        level = int(level)
        if not 0 <= level <= self.max_level:
            raise ValueError(f"level {level} is outside 0..{self.max_level}")
        return level

    def occupancy_changed(self):
        """Drop the cached coarser levels: to be called after ``occupancy_grid`` was written in place."""
        self.__dict__.pop("_coarse", None)
        self.__dict__.pop("_packed", None)

    def packed_occupancy(self, level: int):
        """The occupancy of ``level`` as packed int32 words (bit ``key & 31`` of word ``key >> 5``, key = (x * G + y) * G
        + z) when the structure already holds them -- ``from_triangles`` keeps what the rasteriser wrote for ``max_level``
        -- else None. Dropped with the grid they describe (a replaced or moved ``occupancy_grid``, ``occupancy_changed``)."""
        packed = self.__dict__.get("_packed")
        if packed is None or level != self.max_level or packed[0] is not self.occupancy_grid:
            return None
        return packed[1]

    def occupancy_at(self, level: int, device=None) -> torch.Tensor:
        """Dense bool [G, G, G] of ``level`` (G = 2^level) on ``device`` (default: where the grid lives)."""
        level = self._level(level)
        grid = self._grid_on(device) if device is not None else self.occupancy_grid
        if level == self.max_level:
            return grid
        cache = self.__dict__.get("_coarse")
        if cache is None or cache[0] is not grid:      # the occupancy was replaced or moved: drop the reductions
            cache = self._coarse = (grid, {})
        if level not in cache[1]:
            G, s = 1 << level, 1 << (self.max_level - level)
            cache[1][level] = grid.reshape(G, s, G, s, G, s).permute(0, 2, 4, 1, 3, 5).reshape(G, G, G, s * s * s).any(-1)
        return cache[1][level]

    def query(self, coords, level=None, with_parents=False) -> ASQueryResults:
        """pidx [N]: Morton index of the cell holding each point, -1 if that cell is unoccupied or the point lies outside
        the cube (kaolin's float query: cell = floor(G * (x + 1) / 2), out of bounds -> -1)."""
        level = self._level(level)
        if with_parents:   # [N, level + 1]: column l answers level l (reference octree_grid.py:370)
            return ASQueryResults(pidx=torch.stack([self.query(coords, l).pidx for l in range(level + 1)], dim=-1))
        G = 1 << level
        cell = torch.floor(G * (coords + 1.0) / 2.0)
        inside = ((cell >= 0) & (cell < G)).all(dim=-1)
        q = torch.nan_to_num(cell, nan=0.0).clamp(0, G - 1).long()
        occ = inside & self.occupancy_at(level, coords.device)[q[:, 0], q[:, 1], q[:, 2]]
        pidx = torch.where(occ, _morton_index(q, level), torch.full_like(q[:, 0], -1))
        return ASQueryResults(pidx=pidx)

    def raytrace(self, rays, level=None, with_exit=False) -> ASRaytraceResults:
        from ... import render
        level = self._level(level)
        ridx, pidx, depth = render.raytrace_dense(rays.origins, rays.dirs, self.occupancy_at(level, rays.origins.device),
                                                  level)
        return ASRaytraceResults(ridx=ridx, pidx=pidx, depth=depth if with_exit else depth[:, 0:1])

    def first_hit(self, rays, level=None):
        """(hit bool [N], pidx int32 [N], depth fp32 [N]): the first occupied cell of ``level`` along every ray -- the first
        nugget of ``raytrace`` per ray (same ``pidx``, entry depth bit for bit) -- in ONE launch that writes one row per ray
        (spc.hip, shacira_spc_first_hit) instead of every crossing. A miss gives False / -1 / 0. The kernel reads the packed
        words: the structure's own for ``max_level`` (packed once from the bool grid and kept when it has none)."""
        from ... import hip_ops
        from ..ops.spc.structured import pack_occupancy
        level = self._level(level)
        if level < 1:
            raise ValueError("first_hit needs a level >= 1")
        dev = rays.origins.device
        grid = self.occupancy_at(level, dev)
        words = self.packed_occupancy(level)
        if words is None or words.device != dev:
            words = pack_occupancy(grid)
            if level == self.max_level:
                self._packed = (self.occupancy_grid, words)
        depth, hit, pidx, _ = hip_ops.spc_first_hit(rays.origins, rays.dirs, level, words)
        return hit, pidx, depth

    def _raymarch_voxel(self, rays, num_samples, level=None) -> ASRaymarchResults:
        """num_samples jittered samples inside every intersected cell (reference octree_as.py:171-233)."""
        from ... import render
        res = self.raytrace(rays, level, with_exit=True)
        ridx, depth = res.ridx.long(), res.depth
        K = ridx.shape[0]
        steps = torch.arange(num_samples, device=depth.device)[None].float().repeat([K, 1])
        steps += torch.rand_like(steps)
        steps *= (1.0 / num_samples)
        depth_samples = (depth[..., 0:1] + (depth[..., 1:2] - depth[..., 0:1]) * steps)[..., None]
        deltas = depth_samples[..., 0].diff(dim=-1, prepend=depth[..., 0:1]).reshape(K * num_samples, 1)
        samples = torch.addcmul(rays.origins.index_select(0, ridx)[:, None], rays.dirs.index_select(0, ridx)[:, None],
                                depth_samples)
        boundary = torch.zeros(K * num_samples, dtype=torch.bool, device=depth.device)
        boundary[torch.nonzero(render.mark_pack_boundaries(ridx)).flatten() * num_samples] = True
        ridx = ridx[:, None].expand(K, num_samples).reshape(K * num_samples)
        return ASRaymarchResults(ridx=ridx, samples=samples.reshape(K * num_samples, 3),
                                 depth_samples=depth_samples.reshape(K * num_samples, 1), deltas=deltas,
                                 boundary=boundary)

    def _raymarch_ray(self, rays, num_samples, level=None) -> ASRaymarchResults:
        """num_samples stratified samples per ray between dist_min and dist_max, kept where occupied (reference
        octree_as.py:235-290): generation, occupancy filter and compaction in two HIP launches."""
        from ... import render
        level = self._level(level)
        capacity = getattr(self, "sample_capacity", None)
        if capacity is not None:
            # fixed-size outputs for a step captured into a HIP graph (harness.GraphedNerfFitter): no count read-back;
            # `last_sample_count` keeps the true count on the device so that the owner can watch for dropped samples
            ridx, samples, depth, deltas, boundary, offsets, self.last_sample_count = render.raymarch_ray(
                rays.origins, rays.dirs, rays.dist_min, rays.dist_max, self.occupancy_at(level, rays.origins.device), level,
                num_samples, capacity=capacity)
        else:
            ridx, samples, depth, deltas, boundary, offsets = render.raymarch_ray(
                rays.origins, rays.dirs, rays.dist_min, rays.dist_max, self.occupancy_at(level, rays.origins.device), level,
                num_samples)
        return ASRaymarchResults(ridx=ridx, samples=samples, depth_samples=depth, deltas=deltas, boundary=boundary,
                                 ray_offsets=offsets)

    def _raymarch_voxel_seeded(self, rays, num_samples, level, seed, step) -> ASRaymarchResults:
        """`_raymarch_voxel` as the fused HIP march of render.raymarch_voxel: jitter restated from ``(seed, step)``, per-ray
        pack offsets, and ``sample_capacity`` / ``last_sample_count`` honoured as `_raymarch_ray` does."""
        from ... import render
        level = self._level(level)
        occ = self.occupancy_at(level, rays.origins.device)
        capacity = getattr(self, "sample_capacity", None)
        if capacity is not None:
            ridx, samples, depth, deltas, boundary, offsets, self.last_sample_count = render.raymarch_voxel(
                rays.origins, rays.dirs, occ, level, num_samples, seed, step, capacity=capacity)
        else:
            ridx, samples, depth, deltas, boundary, offsets = render.raymarch_voxel(
                rays.origins, rays.dirs, occ, level, num_samples, seed, step)
        return ASRaymarchResults(ridx=ridx, samples=samples, depth_samples=depth, deltas=deltas, boundary=boundary,
                                 ray_offsets=offsets)

    def raymarch(self, rays, raymarch_type, num_samples, level=None, seed=None, step=0) -> ASRaymarchResults:
        """``seed`` (with 'voxel' only): the fused march whose jitter is a function of ``(seed, step, ray, nugget, sample)``
        and which returns ``ray_offsets``; without it 'voxel' draws from torch's generator as the reference does. The 'ray'
        marcher takes its randomness as a jitter tensor, so a seed is refused there."""
        if raymarch_type == "voxel":
            if seed is not None:
                return self._raymarch_voxel_seeded(rays, num_samples, level, seed, step)
            return self._raymarch_voxel(rays, num_samples, level)
        if raymarch_type == "ray":
            if seed is not None:
                raise ValueError("raymarch_type='ray' takes no seed: its jitter is a tensor (render.raymarch_ray)")
            return self._raymarch_ray(rays, num_samples, level)
        raise TypeError(f"Raymarch sampler type: {raymarch_type} is not supported by OctreeAS.")

    def level_points(self, level: int) -> torch.Tensor:
        """The occupied cells of ``level`` in Morton order, int16 [cells, 3]."""
        level = self._level(level)
        if level == self.max_level:
            return self.points
        cells = torch.nonzero(self.occupancy_at(level))
        order = torch.argsort(_morton_index(cells, level))
        return cells[order].to(torch.int16)


from .aabb_as import AxisAlignedBBoxAS  # noqa: E402  (subclasses OctreeAS above)
