"""Operations on the integer cells of one octree level (pure torch: they run on any device)."""
import torch

from ...accelstructs import _morton_index


def morton_sorted_unique(points: torch.Tensor, level: int):
    """The distinct cells of ``points`` [N, 3] in Morton order: (cells int16 [M, 3], row of every input point in them [N])."""
    codes, inverse = torch.unique(_morton_index(points, level), sorted=True, return_inverse=True)
    cells = torch.empty((codes.shape[0], 3), dtype=torch.int64, device=points.device)
    cells[inverse] = points.long()          # the points of one code are equal: any of them
    return cells.to(torch.int16), inverse


def dilate_points(points: torch.Tensor, level: int) -> torch.Tensor:
    """The cells of ``points`` [N, 3] grown by their 26 neighbours, clipped into the grid of ``level``, distinct and in
    Morton order (int16). As in the reference, clipping folds a border cell's outside neighbours onto the border, so the
    input cells are always part of the result."""
    G = 1 << level
    r = torch.arange(-1, 2, device=points.device)
    offsets = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(27, 3)
    grown = (points.long()[:, None, :] + offsets[None]).reshape(-1, 3).clamp(0, G - 1)
    return morton_sorted_unique(grown, level)[0]
