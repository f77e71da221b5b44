"""Helper, not a test: the seeded voxel march (include/shacira_hip.h, shacira_raymarch_voxel_emit) restated on the CPU. Only the
jitter is restated here -- word j & 3 of Philox4x32-10 on counter (r, i, j >> 2, step), key = the two halves of the seed, mapped
to [0, 1) -- with the generator of tests/mesh_sample_ref.py; the samples themselves come from oracle.render.raymarch_voxel fed
that jitter, so the sample arithmetic exists once."""
import numpy as np
import torch

from mesh_sample_ref import philox4x32_10, unit
from oracle import render as orr


def jitter_words(seed, step, r, i, j):
    """uint32 (broadcast over the operands): the word of sample j of nugget i of ray r."""
    r, i, j = (np.asarray(x, dtype=np.uint64) for x in (r, i, j))
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
    w = philox4x32_10(r, i, j >> np.uint64(2), step, seed & 0xFFFFFFFF, seed >> 32)
    lane = np.broadcast_to(j & np.uint64(3), w[0].shape)
    return np.choose(lane.astype(np.int64), w)


def nugget_index(ridx):
    """int64 [K]: the position of every nugget inside its ray's run (ridx ascending by runs, as raytrace_dense writes it)."""
    ridx = np.asarray(ridx, dtype=np.int64)
    k = np.arange(ridx.shape[0], dtype=np.int64)
    first = np.ones(ridx.shape[0], dtype=bool)
    first[1:] = ridx[1:] != ridx[:-1]
    return k - np.maximum.accumulate(np.where(first, k, 0))


def jitter(seed, step, ridx, num_samples):
    """float32 [K, num_samples]: the jitter of every sample of the given nuggets."""
    ridx = np.asarray(ridx, dtype=np.int64)
    j = np.arange(num_samples, dtype=np.int64)[None]
    return unit(jitter_words(seed, step, ridx[:, None], nugget_index(ridx)[:, None], j)).reshape(ridx.shape[0], num_samples)


def march(origins, dirs, ridx, depth, num_samples, seed, step=0):
    """The rows of the contract for the nuggets (ridx [K], depth [K, 2]) of `render.raytrace_dense`, all on the CPU:
    ridx int64 [S], samples [S, 3], depth_samples [S, 1], deltas [S, 1], boundary bool [S], ray_offsets int64 [N + 1]."""
    ridx = ridx.long()
    jit = torch.from_numpy(jitter(seed, step, ridx.numpy(), num_samples))
    out = orr.raymarch_voxel(origins, dirs, ridx, depth, num_samples, jit)
    offsets = torch.zeros(origins.shape[0] + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(ridx, minlength=origins.shape[0]) * num_samples, 0, out=offsets[1:])
    return out + (offsets,)
