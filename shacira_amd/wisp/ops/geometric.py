"""Geometric helpers (reference wisp/ops/geometric.py): ``find_depth_bound`` on the HIP kernel of sphere_trace.hip and the two
sphere samplers. Same names and argument orders as the reference."""
import numpy as np
import torch

from ... import render


def pack_ends(info):
    """bool [K] pack boundaries (True at every pack's first nugget) -> (first int32 [P], end int32 [P]): end[p] is
    first[p + 1], and the last pack ends at K. One device-to-host size read-back (``nonzero``)."""
    first = torch.nonzero(info).flatten().int()
    last = torch.full((1,), info.shape[0], dtype=torch.int32, device=info.device)
    return first, torch.cat([first[1:], last])


def find_depth_bound(query, nug_depth, info, curr_idxes=None):
    """For every ray pack the nugget that holds the depth ``query[p]``, or the next one behind it, searched in depth order
    from ``curr_idxes[p]`` to the end of the pack; -1 where there is none or ``curr_idxes[p]`` is -1.

    query fp32 [P] or [P, 1]; nug_depth fp32 [K, 2] (entry, exit); info bool [K], True at the first nugget of every pack;
    curr_idxes int32 [P], default: the pack starts. Returns int32 [P].

    The pack ends always come from ``info``. The reference ignores ``info`` when ``curr_idxes`` is given and bounds pack p by
    ``curr_idxes[p + 1]`` (and the last pack by the number of packs), which lets a walk run into the neighbour's nuggets and
    keeps the last ray from advancing; include/shacira_hip.h states both and the rule used here."""
    first, end = pack_ends(info)
    if curr_idxes is None:
        curr_idxes = first
    return render.find_depth_bound(query, curr_idxes, end, nug_depth)


def sample_unif_sphere(n):
    """n unit vectors, uniform on the sphere (normalised Gaussians), float64 [n, 3]."""
    u = np.random.randn(n, 3)
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def sample_fib_sphere(n):
    """n evenly spread unit vectors on the Fibonacci spiral (the order is not random), float64 [n, 3]."""
    k = np.arange(n, dtype=np.float64) + 0.5
    polar = np.arccos(1.0 - 2.0 * k / n)
    azimuth = 2.0 * np.pi * k / ((1.0 + np.sqrt(5.0)) / 2.0)
    return np.stack([np.cos(azimuth) * np.sin(polar), np.sin(azimuth) * np.sin(polar), np.cos(polar)], axis=-1)
