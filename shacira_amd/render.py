"""Sample generation on a dense occupancy grid and volume integration over ray packs (SURVEY.md section 8 "next" f2):
tensor wrappers + autograd Functions over libshacira_hip.so's `shacira_pack_*`, `shacira_raymarch_ray_*`,
`shacira_raytrace_dense_*`, and the sphere tracer's `shacira_find_depth_bound` / `shacira_sphere_trace_step`.

Function names and argument order follow what the reference calls in kaolin 0.13 (`kaolin.render.spc` imported as
``spc_render`` in wisp/tracers/packed_rf_tracer.py:131-151 and wisp/accelstructs/octree_as.py:163-289), so the tracer
and the acceleration structure mirrors read like the reference's. HIP only: CPU tensors raise.
"""
import ctypes

import torch

from . import _lib
from .hip_ops import _need_gpu, _on_device, _ptr, _stream


def mark_pack_boundaries(ridx):
    """True at the first element of every run of equal ray ids (kaolin spc_render.mark_pack_boundaries)."""
    if ridx.numel() == 0:
        return torch.zeros(0, dtype=torch.bool, device=ridx.device)
    return torch.cat([torch.ones(1, dtype=torch.bool, device=ridx.device), ridx[1:] != ridx[:-1]])


def pack_offsets(boundary):
    """bool [S] -> int64 [R + 1] start row of every pack plus the end sentinel (one device->host size read-back)."""
    starts = torch.nonzero(boundary).flatten()
    end = torch.full((1,), boundary.shape[0], dtype=torch.int64, device=boundary.device)
    return torch.cat([starts, end])


class _ExponentialIntegration(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, tau, pack_start):
        _need_gpu(feats, tau, pack_start)
        feats = feats.float().contiguous()
        tau = tau.float().contiguous().reshape(-1)
        S, C = feats.shape
        R = pack_start.shape[0] - 1
        ray_feats = torch.empty((R, C), dtype=torch.float32, device=feats.device)
        weights = torch.zeros((S,), dtype=torch.float32, device=feats.device)   # rows no pack covers (capped emit): 0
        with _on_device(feats.device):
            _lib.check(_lib.lib().shacira_pack_integrate_forward(S, R, C, _ptr(feats), _ptr(tau), _ptr(pack_start),
                                                                 _ptr(ray_feats), _ptr(weights), _stream(feats)),
                       "shacira_pack_integrate_forward")
        ctx.save_for_backward(feats, tau, pack_start)
        return ray_feats, weights.reshape(S, 1)

    @staticmethod
    def backward(ctx, g_ray, g_w):
        feats, tau, pack_start = ctx.saved_tensors
        S, C = feats.shape
        R = pack_start.shape[0] - 1
        g_ray = g_ray.float().contiguous()
        g_w = g_w.float().contiguous().reshape(-1) if g_w is not None else None
        g_feats = torch.zeros_like(feats)
        g_tau = torch.zeros_like(tau)
        with _on_device(feats.device):
            _lib.check(_lib.lib().shacira_pack_integrate_backward(S, R, C, _ptr(feats), _ptr(tau), _ptr(pack_start),
                                                                  _ptr(g_ray), _ptr(g_w), _ptr(g_feats), _ptr(g_tau),
                                                                  _stream(feats)), "shacira_pack_integrate_backward")
        return g_feats, g_tau.reshape(S, 1), None


class _SumReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pack_start):
        _need_gpu(x, pack_start)
        x = x.float().contiguous()
        S, C = x.shape
        R = pack_start.shape[0] - 1
        out = torch.empty((R, C), dtype=torch.float32, device=x.device)
        with _on_device(x.device):
            _lib.check(_lib.lib().shacira_pack_sum(S, R, C, _ptr(x), _ptr(pack_start), _ptr(out), _stream(x)),
                       "shacira_pack_sum")
        ctx.save_for_backward(pack_start)
        ctx.shape = (S, C)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (pack_start,) = ctx.saved_tensors
        S, C = ctx.shape
        R = pack_start.shape[0] - 1
        g_out = g_out.float().contiguous()
        g_x = torch.zeros((S, C), dtype=torch.float32, device=g_out.device)
        with _on_device(g_out.device):
            _lib.check(_lib.lib().shacira_pack_broadcast(S, R, C, _ptr(g_out), _ptr(pack_start), _ptr(g_x),
                                                         _stream(g_out)), "shacira_pack_broadcast")
        return g_x, None


def exponential_integration(feats, tau, boundary, exclusive=True, pack_start=None):
    """kaolin spc_render.exponential_integration: (ray_feats [R, C], transmittance*alpha [S, 1])."""
    if not exclusive:
        raise NotImplementedError("only exclusive=True (the reference's call sites) is implemented")
    if pack_start is None:
        pack_start = pack_offsets(boundary)
    return _ExponentialIntegration.apply(feats, tau.reshape(-1, 1), pack_start)


def sum_reduce(x, boundary, pack_start=None):
    """kaolin spc_render.sum_reduce: per-pack sums [R, C]."""
    if pack_start is None:
        pack_start = pack_offsets(boundary)
    return _SumReduce.apply(x, pack_start)


def _occupancy_u8(occupancy, level):
    G = 1 << level
    if tuple(occupancy.shape) != (G, G, G):
        raise RuntimeError(f"occupancy must be [{G}, {G}, {G}] for level {level}")
    return occupancy.to(torch.uint8).contiguous()


_pad_cache = {}


def _padding_positions(n, device):
    """[n, 3] fixed positions spread over the cube for the padding rows of a capped emit: the field is still evaluated on
    them (their gradient is zero), and identical positions would pile its scatter-add onto a handful of table rows."""
    key = (n, device.index)
    if key not in _pad_cache:
        # (built on the host: never inside a graph capture -- GraphedNerfFitter runs one eager step at every new capacity)
        if len(_pad_cache) >= 16:
            _pad_cache.clear()
        g = torch.Generator().manual_seed(12345)
        _pad_cache[key] = (torch.rand(n, 3, generator=g) * 2 - 1).to(device)
    return _pad_cache[key]


def raymarch_ray(origins, dirs, dist_min, dist_max, occupancy, level, num_samples, jitter=None, capacity=None):
    """`OctreeAS._raymarch_ray` (reference octree_as.py:235-290) on a dense occupancy grid [G, G, G] (bool, [x][y][z]).
    -> ridx int64 [S], samples [S, 3], depth_samples [S, 1], deltas [S, 1], boundary bool [S], and the per-ray pack
    offsets int64 [num_rays + 1] (rays without samples have empty packs) for callers that want to integrate without
    compacting the hit rays first.
    ``capacity`` (for steps captured into a HIP graph): no count is read back -- the outputs have exactly ``capacity``
    rows, survivors beyond it are dropped, the pack offsets are clamped to it, and the rows behind the last survivor are
    padding that belongs to no pack (ray 0, position 0, delta 0: whatever is computed for them integrates into nothing
    and receives a zero gradient). A seventh value is returned then: the true survivor count as a device int64 scalar."""
    _need_gpu(origins, dirs, occupancy)
    origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
    N, dev = origins.shape[0], origins.device
    if jitter is None:
        jitter = torch.rand(N, num_samples, device=dev)
    jitter = jitter.float().contiguous()
    lin = torch.linspace(0, 1.0, num_samples, device=dev)
    occ = _occupancy_u8(occupancy, level)
    L = _lib.lib()
    with _on_device(dev):
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        args = (N, int(num_samples), _ptr(origins), _ptr(dirs), float(dist_min), float(dist_max), _ptr(lin),
                _ptr(jitter), _ptr(occ), int(level))
        _lib.check(L.shacira_raymarch_ray_count(*args, _ptr(counts), _stream(origins)), "shacira_raymarch_ray_count")
        offsets = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        if capacity is not None:
            S = int(capacity)
            ridx = torch.zeros((S,), dtype=torch.int64, device=dev)
            samples = _padding_positions(S, dev).clone()     # rows behind the last survivor keep these
            depth = torch.zeros((S, 1), dtype=torch.float32, device=dev)
            deltas = torch.zeros((S, 1), dtype=torch.float32, device=dev)
            boundary = torch.zeros((S,), dtype=torch.uint8, device=dev)
            _lib.check(L.shacira_raymarch_ray_emit_capped(*args, _ptr(offsets), S, _ptr(ridx), _ptr(samples), _ptr(depth),
                                                          _ptr(deltas), _ptr(boundary), _stream(origins)),
                       "shacira_raymarch_ray_emit_capped")
            total = offsets[-1].clone()
            return ridx, samples, depth, deltas, boundary.bool(), offsets.clamp(max=S), total
        S = int(offsets[-1].item())
        ridx = torch.empty((S,), dtype=torch.int64, device=dev)
        samples = torch.empty((S, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((S, 1), dtype=torch.float32, device=dev)
        deltas = torch.empty((S, 1), dtype=torch.float32, device=dev)
        boundary = torch.empty((S,), dtype=torch.uint8, device=dev)
        _lib.check(L.shacira_raymarch_ray_emit(*args, _ptr(offsets), _ptr(ridx), _ptr(samples), _ptr(depth),
                                               _ptr(deltas), _ptr(boundary), _stream(origins)),
                   "shacira_raymarch_ray_emit")
    return ridx, samples, depth, deltas, boundary.bool(), offsets


def raymarch_voxel(origins, dirs, occupancy, level, num_samples, seed, step=0, capacity=None):
    """`OctreeAS._raymarch_voxel` (reference octree_as.py:171-233) fused and seeded: ``num_samples`` jittered samples inside
    every crossing of an occupied cell of the dense grid [G, G, G] (bool, [x][y][z]), the nuggets of `raytrace_dense`, in
    three launches (count, nuggets, expand) and one count read-back; the jitter is restated from ``(seed, step, ray, nugget,
    sample)`` (the contract above ``shacira_raymarch_voxel_emit``). ``step`` is an int or a device int64 tensor of one
    element, read when the kernel runs. Returns what `raymarch_ray` returns: ridx int64 [S], samples [S, 3], depth_samples
    [S, 1], deltas [S, 1], boundary bool [S], per-ray pack offsets int64 [num_rays + 1]; with ``capacity`` no count is read
    back, the outputs have ``capacity`` rows (padding behind the last survivor), the offsets are clamped and the true row
    count follows as a device int64 scalar."""
    _need_gpu(origins, dirs, occupancy)
    origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
    N, dev, ns = origins.shape[0], origins.device, int(num_samples)
    occ = _occupancy_u8(occupancy, level)
    step_dev = None
    if torch.is_tensor(step):
        _need_gpu(step)
        if step.dtype != torch.int64 or step.numel() != 1:
            raise RuntimeError("raymarch_voxel: a tensor step must be one int64 element")
        step, step_dev = 0, step
    L = _lib.lib()
    with _on_device(dev):
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        _lib.check(L.shacira_raytrace_dense_count(N, _ptr(origins), _ptr(dirs), _ptr(occ), int(level), _ptr(counts),
                                                  _stream(origins)), "shacira_raytrace_dense_count")
        nuggets = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=nuggets[1:])
        offsets = nuggets * ns
        if capacity is not None:
            S = int(capacity)
            ridx = torch.zeros((S,), dtype=torch.int64, device=dev)
            samples = _padding_positions(S, dev).clone()     # rows behind the last survivor keep these
            depth = torch.zeros((S, 1), dtype=torch.float32, device=dev)
            deltas = torch.zeros((S, 1), dtype=torch.float32, device=dev)
            boundary = torch.zeros((S,), dtype=torch.bool, device=dev)     # one byte a row: the kernel stores 0 / 1
        else:
            S = int(nuggets[-1].item()) * ns
            ridx = torch.empty((S,), dtype=torch.int64, device=dev)
            samples = torch.empty((S, 3), dtype=torch.float32, device=dev)
            depth = torch.empty((S, 1), dtype=torch.float32, device=dev)
            deltas = torch.empty((S, 1), dtype=torch.float32, device=dev)
            boundary = torch.empty((S,), dtype=torch.bool, device=dev)
        ws_bytes = int(L.shacira_raymarch_voxel_workspace_bytes(S, ns))
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        _lib.check(L.shacira_raymarch_voxel_emit(N, ns, _ptr(origins), _ptr(dirs), _ptr(occ), int(level), _ptr(nuggets),
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), _ptr(step_dev), S, _ptr(ws),
                                                 ws_bytes, _ptr(ridx), _ptr(samples), _ptr(depth), _ptr(deltas),
                                                 _ptr(boundary), _stream(origins)), "shacira_raymarch_voxel_emit")
    if capacity is not None:
        return ridx, samples, depth, deltas, boundary, offsets.clamp(max=S), offsets[-1].clone()
    return ridx, samples, depth, deltas, boundary, offsets


def raytrace_dense(origins, dirs, occupancy, level):
    """Ray / occupied-cell intersections in depth order (stands in for kaolin's unbatched_raytrace(with_exit=True) on a
    one-level dense octree): ridx int32 [K], pidx int32 [K] (Morton index of the cell), depth [K, 2]."""
    _need_gpu(origins, dirs, occupancy)
    origins, dirs = origins.float().contiguous(), dirs.float().contiguous()
    N, dev = origins.shape[0], origins.device
    occ = _occupancy_u8(occupancy, level)
    L = _lib.lib()
    with _on_device(dev):
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        _lib.check(L.shacira_raytrace_dense_count(N, _ptr(origins), _ptr(dirs), _ptr(occ), int(level), _ptr(counts),
                                                  _stream(origins)), "shacira_raytrace_dense_count")
        offsets = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offsets[1:])
        K = int(offsets[-1].item())
        ridx = torch.empty((K,), dtype=torch.int32, device=dev)
        pidx = torch.empty((K,), dtype=torch.int32, device=dev)
        depth = torch.empty((K, 2), dtype=torch.float32, device=dev)
        _lib.check(L.shacira_raytrace_dense_emit(N, _ptr(origins), _ptr(dirs), _ptr(occ), int(level), _ptr(offsets),
                                                 _ptr(ridx), _ptr(pidx), _ptr(depth), _stream(origins)),
                   "shacira_raytrace_dense_emit")
    return ridx, pidx, depth


def find_depth_bound(query, curr_idxes, pack_end, depth):
    """Per pack, the first nugget at or after ``curr_idxes[p]`` and before ``pack_end[p]`` that holds the depth ``query[p]``
    or lies behind it, -1 if there is none or ``curr_idxes[p] < 0`` (the contract above ``shacira_find_depth_bound``).
    query fp32 [P] or [P, 1], curr_idxes / pack_end int32 [P], depth fp32 [K, 2] -> int32 [P]."""
    _need_gpu(query, curr_idxes, pack_end, depth)
    query = query.float().contiguous().reshape(-1)
    curr_idxes, pack_end = curr_idxes.int().contiguous(), pack_end.int().contiguous()
    depth = depth.float().contiguous()
    P, K = query.shape[0], depth.shape[0]
    if curr_idxes.shape[0] != P or pack_end.shape[0] != P or depth.dim() != 2 or depth.shape[1] != 2:
        raise RuntimeError("find_depth_bound: query, curr_idxes and pack_end must have one entry per pack, depth must be [K, 2]")
    out = torch.empty((P,), dtype=torch.int32, device=query.device)
    with _on_device(query.device):
        _lib.check(_lib.lib().shacira_find_depth_bound(P, K, _ptr(query), _ptr(curr_idxes), _ptr(pack_end), _ptr(depth),
                                                       _ptr(out), _stream(query)), "shacira_find_depth_bound")
    return out


class SphereTrace:
    """The state of one sphere trace over P ray packs and its fused step (the contract above ``shacira_find_depth_bound``).

    ``origins`` / ``dirs`` fp32 [P, 3] are the packs' rays, ``depth`` fp32 [K, 2] the nuggets (entries already offset by the
    caller), ``first`` / ``pack_end`` int32 [P] each pack's first nugget and end, ``pidx`` int32 [K] optional. After the
    constructor ``coords[:count]`` (and ``pidx_active[:count]``) are the positions to evaluate the field at, slot j belonging
    to pack ``active_list[j]``; ``step(sdf)`` consumes those values in one launch, refills the three and returns the new count
    (ONE device-to-host read-back). ``t, dist, dist_prev, curr, x, active, hit`` are the per-pack state."""

    def __init__(self, origins, dirs, depth, first, pack_end, pidx=None, step_size=1.0, min_dis=0.0003,
                 dist_max=float("inf")):
        _need_gpu(origins, dirs, depth, first, pack_end, pidx)
        dev = origins.device
        self.origins, self.dirs = origins.float().contiguous(), dirs.float().contiguous()
        self.depth = depth.float().contiguous()
        self.pack_end = pack_end.int().contiguous()
        self.pidx = pidx.int().contiguous() if pidx is not None else None
        self.step_size, self.min_dis, self.dist_max = float(step_size), float(min_dis), float(dist_max)
        P, K = self.origins.shape[0], self.depth.shape[0]
        if tuple(self.origins.shape) != (P, 3) or tuple(self.dirs.shape) != (P, 3) or tuple(self.depth.shape) != (K, 2) \
                or first.shape[0] != P or self.pack_end.shape[0] != P or (pidx is not None and pidx.shape[0] != K):
            raise RuntimeError("SphereTrace: origins / dirs [P, 3], first / pack_end [P], depth [K, 2], pidx [K]")
        self.num_packs, self.num_nugs = P, K
        self.curr = first.int().clone().contiguous()
        self.t = self.depth[:, 0].index_select(0, self.curr.long()).contiguous()
        self.x = (self.origins + self.dirs * self.t[:, None]).contiguous()
        self.dist = torch.zeros(P, dtype=torch.float32, device=dev)
        self.dist_prev = torch.zeros(P, dtype=torch.float32, device=dev)
        self.active = torch.ones(P, dtype=torch.uint8, device=dev)
        self.hit = torch.zeros(P, dtype=torch.uint8, device=dev)
        self.iteration = 0
        self.count = P
        self.active_list = torch.arange(P, dtype=torch.int32, device=dev)
        self.coords = self.x.clone()
        self.pidx_active = self.pidx.index_select(0, self.curr.long()) if self.pidx is not None else None
        self._spare = (torch.empty_like(self.active_list), torch.empty_like(self.coords),
                       torch.empty_like(self.pidx_active) if self.pidx is not None else None)
        self._counters = torch.zeros(2, dtype=torch.int32, device=dev)   # used in turn: each launch clears the other one

    def step(self, sdf):
        """Consume ``sdf`` (one value per slot of the current active list); returns the number of survivors."""
        if self.count == 0:
            return 0
        _need_gpu(sdf)
        sdf = sdf.detach().float().contiguous().reshape(-1)
        if sdf.shape[0] != self.count:
            raise RuntimeError(f"SphereTrace.step: {self.count} active packs, {sdf.shape[0]} sdf values")
        out_list, out_coords, out_pidx = self._spare
        mine, other = self._counters[self.iteration & 1:], self._counters[(self.iteration + 1) & 1:]
        with _on_device(sdf.device):
            _lib.check(_lib.lib().shacira_sphere_trace_step(
                self.num_packs, self.num_nugs, self.count, 1 if self.iteration == 0 else 0, _ptr(self.active_list),
                _ptr(sdf), _ptr(self.origins), _ptr(self.dirs), _ptr(self.depth), _ptr(self.pack_end), _ptr(self.pidx),
                self.step_size, self.min_dis, self.dist_max, _ptr(self.t), _ptr(self.dist), _ptr(self.dist_prev),
                _ptr(self.curr), _ptr(self.x), _ptr(self.active), _ptr(self.hit), _ptr(out_list), _ptr(out_coords),
                _ptr(out_pidx), _ptr(mine), _ptr(other), _stream(sdf)), "shacira_sphere_trace_step")
        self._spare = (self.active_list, self.coords, self.pidx_active)
        self.active_list, self.coords, self.pidx_active = out_list, out_coords, out_pidx
        self.iteration += 1
        self.count = int(self._counters[(self.iteration - 1) & 1].item())
        return self.count
