"""Samplers over cells and depth intervals, the argument lists of the reference's ``wisp.ops.spc`` samplers (pure torch: they
run on any device)."""
import torch


def sample_spc(corners: torch.Tensor, level: int, num_samples: int, seed=None, segment=0) -> torch.Tensor:
    """``num_samples`` uniform points inside every cell of ``corners`` [N, >= 3] (integer cells of ``level``), in [-1, 1]^3:
    [N * num_samples, 3], the samples of one cell adjacent. A uniform point of cell c is (c + U[0, 1)^3) * 2 / G - 1. With
    an int ``seed`` (``corners`` on the GPU) the fused kernel of mesh_sample.hip makes them, each a function of (seed, index,
    ``segment``), in the same operator order."""
    if seed is not None:
        from .... import hip_ops
        hip_ops._need_gpu(corners)
        return hip_ops.mesh_sample("cells", seed=seed, segment=segment, corners=corners, samples_per_cell=num_samples,
                                   cell_level=level).points
    cell_width = 2.0 / (1 << level)
    low = corners[:, :3].to(torch.float32) * cell_width - 1.0            # the cell's corner towards -1
    offsets = torch.rand((corners.shape[0], num_samples, 3), device=corners.device) * cell_width
    return (low.unsqueeze(1) + offsets).reshape(-1, 3)


def sample_from_depth_intervals(depth_intervals: torch.Tensor, num_samples: int) -> torch.Tensor:
    """[K, 2] entry / exit depths -> [K, num_samples] stratified depths: sample s is uniform in stratum s of the
    ``num_samples`` equal strata of its interval, so every row ascends from entry to exit."""
    near, far = depth_intervals[:, 0:1], depth_intervals[:, 1:2]
    stratum = torch.arange(num_samples, device=depth_intervals.device, dtype=torch.float32).unsqueeze(0)
    u = torch.rand((depth_intervals.shape[0], num_samples), device=depth_intervals.device)
    return torch.lerp(near.expand_as(u), far.expand_as(u), (stratum + u) / num_samples)


def expand_pack_boundary(pack_boundary: torch.Tensor, num_samples: int) -> torch.Tensor:
    """Pack boundaries [N] -> int32 [N * num_samples] for packs whose every entry became ``num_samples`` samples: the first
    sample of a boundary entry is a boundary, nothing else is."""
    out = torch.zeros((pack_boundary.shape[0], num_samples), dtype=torch.int32, device=pack_boundary.device)
    out[:, 0] = pack_boundary.to(torch.int32)
    return out.reshape(-1)
