"""Octree feature lookup for ``OctreeGrid`` / ``CodebookOctreeGrid``: the corner index, the autograd Function and the
functional API over the HIP kernels of ``octree.hip`` (contract: include/shacira_hip.h, shacira_octree_forward).

The reference looks features up per level with ``kaolin.ops.spc.unbatched_interpolate_trilinear`` and Python glue
(wisp/models/grids/octree_grid.py:303-391), on top of kaolin's sparse point hierarchy and its dual octree
(``make_trilinear_spc``). Here the occupied set is ``OctreeAS``'s dense bit grid and one launch serves every level.

The corner index of a level l (G = 2^l cells, S = G + 1 lattice points per axis), built by ``build_octree_index``:

  ``points_dual``   int16 [C, 3]: the distinct lattice points that are a corner of at least one occupied cell, in ASCENDING
                    LINEAR KEY (x * S + y) * S + z -- x slowest, z fastest. This row order is the row order of the level's
                    feature table [C + 1, F] (the last row is the reference's padding row). It is deterministic and a
                    function of the occupied set alone. It is not kaolin's order: no checkpoint compatibility is claimed.
  ``trinkets``      int32 [cells, 8]: row c belongs to cell ``level_points[c]`` (Morton order); entry k is the table row of
                    corner (k >> 2 & 1, k >> 1 & 1, k & 1), z fastest (kaolin's coefficient order). Built on first use:
                    the kernels do not read it.
  ``occupancy``     int32 [ceil(G^3 / 32)]: bit key & 31 of word key >> 5, key = (x * G + y) * G + z, per occupied cell.
  ``corner_index``  int32 [ceil(S^3 / 32), 2]: per 32 lattice keys {corner bits, corners before the word}; a corner's row is
                    the count plus the popcount of the bits below its own. This is what the kernels read.

Kept from the reference's composition: gradients reach every feature table, and the coordinates when they require one;
first order only (``once_differentiable``: a backward with ``create_graph=True`` works, a second differentiation raises).
One stated deviation: the reference casts the table to fp16 for kaolin's kernel; the lookup here is fp32. Tables of other
dtypes (fp16 / fp64 modules) take the torch composition ``octree_torch`` after one ``hip_ops.warn_unfused`` warning; host
tensors raise in ``octree_interpolate``, as every ``hip_ops`` entry does (``octree_torch`` itself runs anywhere).
"""
import torch
from torch.autograd.function import once_differentiable

from ... import hip_ops
from ..accelstructs import _morton_index

_CORNERS = tuple((k >> 2 & 1, k >> 1 & 1, k & 1) for k in range(8))


def _pack_bits(flat: torch.Tensor):
    """bool [n] -> (int32 [ceil(n / 32)] words, bit i of word w = flat[32 w + i]; int32 set bits per word)."""
    n = flat.shape[0]
    words = (n + 31) // 32
    if words * 32 != n:
        flat = torch.cat([flat, torch.zeros(words * 32 - n, dtype=torch.bool, device=flat.device)])
    bits = flat.reshape(words, 32)
    weights = torch.ones(32, dtype=torch.int64, device=flat.device) << torch.arange(32, device=flat.device)
    packed = torch.empty(words, dtype=torch.int32, device=flat.device)
    count = torch.empty(words, dtype=torch.int32, device=flat.device)
    step = 1 << 20          # words per pass: the int64 [step, 32] product stays at 256 MiB whatever the level
    for w0 in range(0, words, step):
        chunk = bits[w0:w0 + step]
        v = (chunk.to(torch.int64) * weights).sum(-1)
        packed[w0:w0 + step] = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)
        count[w0:w0 + step] = chunk.sum(-1, dtype=torch.int32)
    return packed, count


class OctreeLevelIndex:
    """The index of one level (module docstring). ``rows`` = C, the table has C + 1 rows."""

    def __init__(self, level, level_points, points_dual, occupancy, corner_index):
        self.level = int(level)
        self.level_points = level_points
        self.points_dual = points_dual
        self.occupancy = occupancy
        self.corner_index = corner_index
        self.rows = int(points_dual.shape[0])
        self._trinkets = None
        self._cell_codes = None
        self._on = {}

    @property
    def device(self):
        return self.corner_index.device

    def corner_keys(self) -> torch.Tensor:
        """int64 [C], ascending: the linear keys of ``points_dual``."""
        S = (1 << self.level) + 1
        p = self.points_dual.long()
        return (p[:, 0] * S + p[:, 1]) * S + p[:, 2]

    @property
    def trinkets(self) -> torch.Tensor:
        if self._trinkets is None:
            S = (1 << self.level) + 1
            keys = self.corner_keys()
            c = self.level_points.long()
            offs = torch.tensor(_CORNERS, dtype=torch.int64, device=c.device)
            q = c[:, None, :] + offs[None]
            self._trinkets = torch.searchsorted(keys, ((q[..., 0] * S + q[..., 1]) * S + q[..., 2]).contiguous()
                                                ).to(torch.int32)
        return self._trinkets

    @property
    def cell_codes(self) -> torch.Tensor:
        """int64 [cells], ascending: the Morton codes of ``level_points`` (``pidx`` of ``OctreeAS.query`` -> cell rank)."""
        if self._cell_codes is None:
            self._cell_codes = _morton_index(self.level_points, self.level)
        return self._cell_codes

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        if device not in self._on:
            moved = OctreeLevelIndex(self.level, self.level_points.to(device), self.points_dual.to(device),
                                     self.occupancy.to(device), self.corner_index.to(device))
            self._on[device] = moved
        return self._on[device]


class OctreeIndex:
    """``index[level]`` -> ``OctreeLevelIndex`` for every level it was built for. ``source``: the structure it describes."""

    def __init__(self, levels, source=None):
        self.levels = dict(levels)
        self.source = source

    def __getitem__(self, level):
        return self.levels[int(level)]

    def __contains__(self, level):
        return int(level) in self.levels


def build_octree_level(blas, level) -> OctreeLevelIndex:
    G = 1 << level
    S = G + 1
    occ = blas.occupancy_at(level)
    corner = torch.zeros((S, S, S), dtype=torch.bool, device=occ.device)
    for dx, dy, dz in _CORNERS:
        corner[dx:dx + G, dy:dy + G, dz:dz + G] |= occ
    flat = corner.reshape(-1)
    keys = torch.nonzero(flat).flatten()       # ascending linear key: the row order
    points_dual = torch.stack([keys // (S * S), (keys // S) % S, keys % S], dim=-1).to(torch.int16)
    bits, count = _pack_bits(flat)
    before = torch.cumsum(count, 0, dtype=torch.int64) - count
    corner_index = torch.stack([bits, before.to(torch.int32)], dim=-1).contiguous()
    occupancy = blas.packed_occupancy(level)         # a rasterised mesh brings its words
    if occupancy is None:
        occupancy, _ = _pack_bits(occ.reshape(-1))
    return OctreeLevelIndex(level, blas.level_points(level).to(occ.device), points_dual, occupancy, corner_index)


def build_octree_index(blas, levels) -> OctreeIndex:
    """The corner index of ``levels`` for the occupied set of ``blas`` (an ``OctreeAS``), with torch operations on the
    device the occupancy lives on."""
    return OctreeIndex({int(l): build_octree_level(blas, int(l)) for l in levels}, source=blas)


def _gather(index, lods, device):
    return [index[l].to(device) for l in lods]


class OctreeInterpolate(torch.autograd.Function):
    """coords fp32 [N, 3], one fp32 table [C_l + 1, F] per level -> [N, F] ('sum') or [N, len(lods) * F]."""

    @staticmethod
    def forward(ctx, coords, lods, index, multiscale_sum, *features):
        levels = _gather(index, lods, coords.device)
        feats = hip_ops.octree_forward(coords, levels, features, multiscale_sum)
        ctx.levels, ctx.multiscale_sum, ctx.fdim = levels, bool(multiscale_sum), features[0].shape[1]
        if ctx.needs_input_grad[0]:   # the coordinate gradient reads the table values; nothing else does
            ctx.save_for_backward(coords, *features)
        else:
            ctx.save_for_backward(coords)
        return feats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        need_coords = ctx.needs_input_grad[0]
        need_features = any(ctx.needs_input_grad[4:])
        saved = ctx.saved_tensors
        coords, features = saved[0], (saved[1:] if need_coords else None)
        grads, grad_coords = hip_ops.octree_backward(coords, ctx.levels, ctx.fdim, grad_output, ctx.multiscale_sum,
                                                     features=features, need_features=need_features,
                                                     need_coords=need_coords)
        if grads is None:
            grads = [None] * (len(ctx.needs_input_grad) - 4)
        else:
            grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:])]
        return (grad_coords, None, None, None, *grads)


def octree_torch(coords, lods, features, index, multiscale_sum):
    """The plain torch composition, per level ``feats[trinkets[rank]] * coeffs`` summed over the corners (the reference's
    'trilinear_old' branch), then 'cat' or a sum over the levels. Runs on any device and dtype; the cell location follows
    the coordinates' dtype."""
    N = coords.shape[0]
    per_level = []
    for l, table in zip(lods, features):
        li = index[l].to(coords.device)
        G = 1 << li.level
        p = (coords + 1.0) * (G / 2)
        fl = torch.floor(p)
        hit = ((p >= 0) & (p < G)).all(dim=-1)
        cell = torch.nan_to_num(fl, nan=0.0).clamp(0, G - 1).long()
        codes = li.cell_codes
        if codes.shape[0] == 0:
            per_level.append(torch.zeros((N, table.shape[1]), dtype=table.dtype, device=coords.device))
            continue
        code = _morton_index(cell, li.level)
        rank = torch.searchsorted(codes, code).clamp(max=codes.shape[0] - 1)
        hit = hit & (codes[rank] == code)
        t = torch.where(hit[:, None], p - fl, torch.zeros_like(p)).to(table.dtype)
        coeffs = torch.stack([(t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1])
                              * (t[:, 2] if dz else 1 - t[:, 2]) for dx, dy, dz in _CORNERS], dim=-1)
        corner_feats = table[li.trinkets[rank].long()]
        val = (corner_feats * coeffs[..., None]).sum(-2)
        per_level.append(torch.where(hit[:, None], val, torch.zeros_like(val)))
    if multiscale_sum:
        return torch.stack(per_level, dim=0).sum(0)
    return torch.cat(per_level, dim=-1)


def octree_interpolate(coords, lods, features, index, multiscale_sum):
    """coords [N, 3] -> [N, F] (``multiscale_sum``) or [N, len(lods) * F], levels in the order given.

    ``lods``: the octree level of each table; ``features``: one [C_l + 1, F] table per level; ``index``: an ``OctreeIndex``
    holding those levels."""
    features = list(features)
    lods = tuple(int(l) for l in lods)
    hip_ops._need_gpu(coords, *features)
    if coords.dim() != 2 or coords.shape[-1] != 3:
        raise RuntimeError(f"shacira_amd: coords must be [N, 3], got {tuple(coords.shape)}")
    if len(features) != len(lods):
        raise RuntimeError(f"shacira_amd: {len(lods)} levels need {len(lods)} feature tables, got {len(features)}")
    fdt = {f.dtype for f in features}
    if fdt == {torch.float32} and coords.dtype in (torch.float32, torch.float16, torch.bfloat16):
        return OctreeInterpolate.apply(coords.float().contiguous(), lods, index, bool(multiscale_sum),
                                       *[f if f.is_contiguous() else f.contiguous() for f in features])
    hip_ops.warn_unfused("octree lookup", f"tables {sorted(str(d) for d in fdt)}, coordinates {coords.dtype}: the kernels "
                         "take fp32")
    return octree_torch(coords, lods, features, index, multiscale_sum)
