"""The yardsticks of the sphere tracer, written from the contract above ``shacira_find_depth_bound`` in
include/shacira_hip.h and not from the product code.

  find_depth_bound_ref             the contract's rule (pack ends), numpy
  find_depth_bound_reference_rule  the reference kernel's literal bounds (curr[p + 1]; num_packs for the last pack)
  trace_ref                        the contract's per-pack scalar loop in numpy fp32, field values through a callback
  trace_literal                    the reference tracer's masked-tensor loop (torch ops, any device) with the pack ends fixed
  make_case / analytic_sdf         the shared inputs: rays from the radius-3 sphere toward uniform points of the cube, a
                                   shell (or dense) occupancy walked by oracle.render.raytrace_dense, sdf = |x| - 0.7

Everything is fp32 with one rounding per operator: numpy scalars and arrays of dtype float32 never contract.
"""
import functools

import numpy as np
import torch

import octree_ref
from oracle import render as oracle_render

F = np.float32
RADIUS = 0.7
ENTRY_OFFSET = F(1e-5)      # what the tracer adds to every nugget's entry depth before it starts


# ---- find_depth_bound -------------------------------------------------------------------------------------------------------
def _walk(q, c, end, depth):
    if c < 0:
        return -1
    for i in range(int(c), int(end)):
        entry, exit_ = depth[i, 0], depth[i, 1]
        if (q >= entry and q <= exit_) or q < entry:
            return i
    return -1


def find_depth_bound_ref(query, curr, end, depth):
    """int32 [P]: per pack the first nugget in [curr[p], end[p]) that holds query[p] or lies behind it, else -1."""
    query = np.asarray(query, dtype=F).reshape(-1)
    depth = np.asarray(depth, dtype=F)
    return np.array([_walk(query[p], curr[p], end[p], depth) for p in range(query.shape[0])], dtype=np.int32)


def find_depth_bound_reference_rule(query, curr, depth):
    """The reference kernel's own bounds: pack p walks to curr[p + 1], the last pack to num_packs. Its output buffer starts at
    -1 (the kernel writes only what it finds)."""
    query = np.asarray(query, dtype=F).reshape(-1)
    depth = np.asarray(depth, dtype=F)
    P = query.shape[0]
    out = np.full(P, -1, dtype=np.int32)
    for p in range(P):
        bound = P if p == P - 1 else int(curr[p + 1])
        out[p] = _walk(query[p], curr[p], bound, depth)
    return out


# ---- the contract's loop ------------------------------------------------------------------------------------------------------
def trace_ref(origins, dirs, depth, first, end, sdf_fn, num_steps, step_size=1.0, min_dis=0.0003, dist_max=np.inf,
              snapshots=None):
    """origins / dirs fp32 [P, 3] (per pack), depth fp32 [K, 2] with the entry offset already added, first / end int [P].
    ``sdf_fn(coords [n, 3] fp32, packs int [n], iteration)`` -> [n] values for the active packs, in ascending pack order.
    Returns the state dict (t, dist, dist_prev, curr, x, active, hit) plus ``jumps`` (moves to another nugget) and
    ``iterations`` (rounds that had an active pack). ``snapshots``: a list that receives a copy of the state after every round."""
    o, d = np.asarray(origins, dtype=F), np.asarray(dirs, dtype=F)
    depth = np.asarray(depth, dtype=F)
    P = o.shape[0]
    step_size, min_dis, dist_max = F(step_size), F(min_dis), F(dist_max)
    min_dis5 = F(5.0) * min_dis
    curr = np.asarray(first, dtype=np.int32).copy()
    t = depth[curr, 0].copy() if P else np.zeros(0, dtype=F)
    x = o + d * t[:, None]
    dist, dist_prev = np.zeros(P, dtype=F), np.zeros(P, dtype=F)
    active, hit = np.ones(P, dtype=bool), np.zeros(P, dtype=bool)
    jumps = iterations = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(num_steps):
            packs = np.nonzero(active)[0]
            if packs.shape[0] == 0:
                break
            iterations += 1
            s = np.asarray(sdf_fn(x[packs].copy(), packs, i), dtype=F).reshape(-1)
            for j, p in enumerate(packs):
                dist[p] = s[j] * step_size
                if i == 0:
                    dist_prev[p] = dist[p]
                t[p] = t[p] + dist[p]
                x[p] = o[p] + d[p] * t[p]
                hit[p] = bool(np.abs(dist[p]) < min_dis or np.abs(dist[p] + dist_prev[p]) * F(0.5) < min_dis5)
                if hit[p] or not (t[p] < dist_max):
                    active[p] = False
                    continue
                dist_prev[p] = dist[p]
                n = _walk(t[p], curr[p], end[p], depth)
                if n == -1:
                    active[p] = False
                    continue
                if n != curr[p]:
                    t[p] = depth[n, 0]
                    jumps += 1
                curr[p] = n
                x[p] = o[p] + d[p] * t[p]
            if snapshots is not None:
                snapshots.append(dict(t=t.copy(), dist=dist.copy(), dist_prev=dist_prev.copy(), curr=curr.copy(), x=x.copy(),
                                      active=active.copy(), hit=hit.copy()))
    return dict(t=t, dist=dist, dist_prev=dist_prev, curr=curr, x=x, active=active, hit=hit, jumps=jumps,
                iterations=iterations)


# ---- the reference tracer's loop -------------------------------------------------------------------------------------------------
def trace_literal(origins, dirs, depth, first, end, sdf_fn, num_steps, step_size=1.0, min_dis=0.0003, dist_max=float("inf"),
                  find_depth_bound=None):
    """The masked-tensor loop of the reference's PackedSDFTracer.trace, in its order of operations, on torch tensors of any
    device: every ray is carried through every operation and a mask says which results count; ``t`` is advanced for all rays
    (the reference's drift). ``find_depth_bound(query [P, 1], curr int32 [P], end int32 [P], depth)`` is the rule with the pack
    ends fixed (default: find_depth_bound_ref on the host). ``sdf_fn(coords [n, 3])`` -> [n, 1] or [n].
    Returns dict(hit bool [P], x [P, 3], t [P], iterations) -- t is the drifting depth."""
    if find_depth_bound is None:
        def find_depth_bound(query, curr, end_, depth_):
            return torch.from_numpy(find_depth_bound_ref(query.cpu().numpy(), curr.cpu().numpy(), end_.cpu().numpy(),
                                                         depth_.cpu().numpy())).to(query.device)
    o, d = origins, dirs
    P = o.shape[0]
    thr = float(F(min_dis))
    thr5 = float(F(5.0) * F(min_dis))
    curr = first.int().clone()
    end = end.int()
    mask = torch.ones(P, dtype=torch.bool, device=o.device)
    hit = torch.zeros_like(mask)
    t = depth[first.long(), 0:1].clone()
    x = o + d * t
    dist = torch.zeros_like(t)
    iterations = 0
    dist[mask] = sdf_fn(x[mask]).reshape(-1, 1).to(dist.dtype) * step_size
    dist[~mask] = 20
    dist_prev = dist.clone()
    for _ in range(num_steps):
        iterations += 1
        t = t + dist
        x = torch.where(mask[:, None], o + d * t, x)
        hit = torch.where(mask, dist.abs()[:, 0] < thr, hit)
        hit = hit | torch.where(mask, (dist + dist_prev).abs()[:, 0] * 0.5 < thr5, hit)
        mask = torch.where(mask, (t < dist_max)[:, 0], mask)
        mask = mask & ~hit
        if not mask.any():
            break
        dist_prev = torch.where(mask[:, None], dist, dist_prev)
        nxt = find_depth_bound(t, curr, end, depth)
        mask = mask & (nxt != -1)
        jumped = nxt != curr
        curr = torch.where(mask, nxt, curr)
        t = torch.where((mask & jumped)[:, None], depth[curr.long(), 0:1], t)
        x = torch.where(mask[:, None], o + d * t, x)
        if not mask.any():
            break
        dist[mask] = sdf_fn(x[mask]).reshape(-1, 1).to(dist.dtype) * step_size
    return dict(hit=hit, x=x, t=t[:, 0], iterations=iterations)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def analytic_sdf(x, packs=None, iteration=None):
    """|x| - 0.7 in fp32, one rounding per operator: sqrt((x0 * x0 + x1 * x1) + x2 * x2) - 0.7f."""
    x = np.asarray(x, dtype=F)
    return np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) - F(RADIUS)


def occupancy_grid(level, dense=False):
    G = 1 << level
    occ = torch.zeros(G, G, G, dtype=torch.bool)
    if dense:
        occ[:] = True
    else:
        cells = torch.from_numpy(octree_ref.shell_cells(level, RADIUS))
        occ[cells[:, 0], cells[:, 1], cells[:, 2]] = True
    return occ


def make_rays(num_rays, seed=0):
    """Origins on the radius-3 sphere, unit directions toward uniform points of [-1, 1]^3; fp32 [num_rays, 3] each."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((num_rays, 3))
    origins = 3.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    toward = rng.uniform(-1.0, 1.0, (num_rays, 3)) - origins
    dirs = toward / np.linalg.norm(toward, axis=1, keepdims=True)
    return origins.astype(F), dirs.astype(F)


def packs_of(ridx, depth):
    """ridx [K] (sorted by ray), depth [K, 2] -> first, end int32 [P], ray of every pack int64 [P], offset depth fp32 [K, 2]."""
    ridx = np.asarray(ridx).astype(np.int64)
    K = ridx.shape[0]
    boundary = np.ones(K, dtype=bool)
    boundary[1:] = ridx[1:] != ridx[:-1]
    first = np.nonzero(boundary)[0].astype(np.int32)
    end = np.concatenate([first[1:], np.array([K], dtype=np.int32)]).astype(np.int32)
    depth = np.asarray(depth, dtype=F).copy()
    depth[:, 0] = depth[:, 0] + ENTRY_OFFSET
    return first, end, ridx[first], depth


@functools.lru_cache(maxsize=None)
def make_case(level, num_rays=512, dense=False, seed=0):
    """The shared CPU inputs (computed once per shape; callers must not write into them): dict(origins, dirs [N, 3], ridx [K],
    depth [K, 2] offset, first, end [P], ray [P], o, d [P, 3] per pack)."""
    origins, dirs = make_rays(num_rays, seed)
    ridx, _, depth = oracle_render.raytrace_dense(torch.from_numpy(origins), torch.from_numpy(dirs),
                                                  occupancy_grid(level, dense), level)
    first, end, ray, depth = packs_of(ridx.numpy(), depth.numpy())
    return dict(origins=origins, dirs=dirs, ridx=ridx.numpy(), depth=depth, first=first, end=end, ray=ray, o=origins[ray],
                d=dirs[ray])


def closest_approach(o, d):
    """Distance of the origin to the line o + d * t, fp64."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.linalg.norm(o - np.sum(o * d, axis=1, keepdims=True) * d, axis=1)
