"""``StructuredPointCloud``: a coloured structured point cloud (SPC) of one level in the device layout of
include/shacira_hip.h ("Structured point clouds"): the packed occupancy ``words``, their popcount prefix ``rank`` and the RGBA
bytes ``colors`` by slot -- slots number the occupied cells in KEY order, key = (x G + y) G + z. Device tensors are built by
the fused kernels of spc.hip (``hip_ops.spc_from_points`` / ``spc_from_depth``: mark, scan, accumulate, resolve; no sort);
host tensors by the torch restatement below, which gives the same integers."""
import torch

from ...accelstructs import OctreeAS, _morton_index


def num_words(level):
    return max(1, (1 << (3 * int(level))) // 32)


def pack_occupancy(grid):
    """bool [G, G, G] -> the packed int32 words (bit key & 31 of word key >> 5), in slices that bound the temporary."""
    flat = grid.reshape(-1)
    if flat.numel() < 32:
        flat = torch.cat([flat, flat.new_zeros(32 - flat.numel())])
    flat = flat.reshape(-1, 32)
    shifts = torch.arange(32, dtype=torch.int64, device=grid.device)
    out = torch.empty((flat.shape[0],), dtype=torch.int32, device=grid.device)
    step = 1 << 19
    for s in range(0, flat.shape[0], step):
        w = (flat[s:s + step].to(torch.int64) << shifts).sum(dim=1)
        out[s:s + step] = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)      # the same 32 bits, signed
    return out


def unpack_occupancy(words, level):
    """The packed words of ``level`` -> bool [G, G, G]."""
    G = 1 << level
    shifts = torch.arange(32, dtype=torch.int32, device=words.device)
    bits = ((words.to(torch.int32)[:, None] >> shifts) & 1).bool().reshape(-1)
    return bits[:G * G * G].reshape(G, G, G)


def morton_to_cells(pidx, level):
    """Morton indices (x most significant of each bit triple) -> int64 cells [N, 3]."""
    p = pidx.long()
    xyz = torch.zeros((p.shape[0], 3), dtype=torch.int64, device=p.device)
    for b in range(level):
        xyz[:, 0] |= ((p >> (3 * b + 2)) & 1) << b
        xyz[:, 1] |= ((p >> (3 * b + 1)) & 1) << b
        xyz[:, 2] |= ((p >> (3 * b)) & 1) << b
    return xyz


def rounded_mean_colors(sums, counts):
    """int64 sums [cells, 3] and counts [cells] -> uint8 [cells, 4]: (2 sum + n) / (2 n) by integer division, A = 255."""
    n = counts.long()[:, None]
    rgb = torch.div(2 * sums.long() + n, 2 * n, rounding_mode="floor")
    alpha = torch.full_like(n, 255)
    return torch.cat([rgb, alpha], dim=1).to(torch.uint8)


class StructuredPointCloud:
    def __init__(self, level, words, rank, colors, num_cells):
        self.level, self.words, self.rank, self.colors, self.num_cells = int(level), words, rank, colors, int(num_cells)

    @property
    def device(self):
        return self.words.device

    @classmethod
    def from_pointcloud(cls, points, colors_u8, level):
        """The SPC of ``level`` holding ``points`` (fp32 [N, 3], quantised by ``OctreeAS.quantize_pointcloud``: points that are
        not finite are dropped) with the rounded mean of ``colors_u8`` (uint8 [N, 3], or None) per cell."""
        level = int(level)
        if points.is_cuda:
            from .... import hip_ops
            return cls(level, *hip_ops.spc_from_points(points.float(), colors_u8, level))
        if not 1 <= level <= 10:
            raise ValueError(f"an SPC level must be in 1..10, got {level}")
        G = 1 << level
        cells, keep = OctreeAS.quantize_pointcloud(points, level)
        keys = (cells[:, 0] * G + cells[:, 1]) * G + cells[:, 2]
        uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
        grid = torch.zeros((G * G * G,), dtype=torch.bool)
        grid[uniq] = True
        words = pack_occupancy(grid.reshape(G, G, G))
        rank = cls._rank_of(words)
        colors = None
        if colors_u8 is not None:
            sums = torch.zeros((uniq.shape[0], 3), dtype=torch.int64).index_add_(0, inverse, colors_u8[keep].long())
            colors = rounded_mean_colors(sums, torch.bincount(inverse, minlength=uniq.shape[0]))
        return cls(level, words, rank, colors, uniq.shape[0])

    @classmethod
    def from_depth(cls, records, depth, images, level, bg_color="white", mip=0):
        """The SPC of the points of the finite pixels of ``depth`` (fp32 [V, H, W]) seen through the camera ``records``, coloured
        from ``images`` (uint8, or the uint16 sums of ``mip``; None: no colours). Device tensors only: the cloud is never made."""
        from .... import hip_ops
        return cls(int(level), *hip_ops.spc_from_depth(records, depth, images, level, bg_color, mip))

    @staticmethod
    def _rank_of(words):
        w = words.long() & 0xFFFFFFFF
        pop = torch.zeros_like(w)
        for b in range(32):
            pop += (w >> b) & 1
        return (torch.cumsum(pop, dim=0) - pop).to(torch.int32)

    def _keys(self):
        """The keys of the occupied cells in slot order (ascending), cached."""
        if getattr(self, "_key_cache", None) is None:
            self._key_cache = torch.nonzero(unpack_occupancy(self.words, self.level).reshape(-1)).flatten()
        return self._key_cache

    def to_octree_as(self):
        """The ``OctreeAS`` of the same occupied set; it keeps these ``words`` as its packed occupancy."""
        blas = OctreeAS(self.level, unpack_occupancy(self.words, self.level))
        blas._packed = (blas.occupancy_grid, self.words)
        return blas

    def slots_of(self, pidx):
        """Morton indices ``pidx`` [N] of occupied cells (as the tracers write them) -> their slots, int64 [N]. The slot of a
        cell that is not occupied is meaningless."""
        G = 1 << self.level
        c = morton_to_cells(pidx, self.level)
        key = (c[:, 0] * G + c[:, 1]) * G + c[:, 2]
        keys = self._keys()
        return torch.searchsorted(keys, key).clamp(max=max(keys.shape[0] - 1, 0))

    def colors_morton(self):
        """uint8 [cells, 4]: the colours in the Morton order of ``OctreeAS.points``."""
        G = 1 << self.level
        keys = self._keys()
        cells = torch.stack([keys // (G * G), (keys // G) % G, keys % G], dim=1)
        order = torch.argsort(_morton_index(cells, self.level))
        return self.colors[order]
