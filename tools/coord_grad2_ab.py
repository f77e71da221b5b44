"""Backward of the hash-grid coordinate backward (second order): timing of its three results beside the first-order calls.

    python tools/coord_grad2_ab.py [--shapes S1,D256k,D64k,B] [--iters 40]

Per shape, HIP-event times of the forward, the codebook backward, the coordinate backward, and of
hip_ops.hashgrid_coords_backward2 asked for (1) grad_grad_output alone, (3) grad_coords alone, (1) + (3) in one launch,
(2) grad_codebook alone, and all three. 3-D shapes with a plan time the gathers with and without it (the plan selects the
sorted walk). Calls are warmed up, then timed round-robin (one call of each kind per round); medians, minima and the 10-90 %
spread in ms. For (2), the number of float adds (corners whose row lies inside the table, times F) and
the achieved rate of added bytes. One JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shacira_amd import hip_ops  # noqa: E402


def geo(mn, mx, L):
    b = np.exp((np.log(mx) - np.log(mn)) / (L - 1))
    return [int(1 + np.floor(mn * (b ** l))) for l in range(L)]


D = (3, geo(16, 2048, 16), 19, 2)
SHAPES = {   # name: (dim, resolutions, bitwidth, F, N, table dtype)
    "S1": D + (1 << 20, torch.float32),
    "D256k": D + (1 << 18, torch.float32),
    "D64k": D + (1 << 16, torch.float32),
    "B": (2, geo(16, 512, 16), 11, 2, 393_216, torch.float32),
}


def run(name, iters, dev):
    dim, res, bw, F, N, dt = SHAPES[name]
    sizes = [min(2 ** bw, r ** dim) for r in res]
    first = torch.tensor(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32), device=dev)
    T = int(sum(sizes))
    g = torch.Generator(device=dev).manual_seed(0)
    coords = torch.rand((N, dim), device=dev, generator=g) * 2 - 1
    table = (torch.randn((T, F), device=dev, generator=g) * 0.05).to(dt)
    go = torch.randn((N, len(res) * F), device=dev, generator=g).to(dt)
    v = torch.randn((N, dim), device=dev, generator=g)
    plan = hip_ops.hashgrid_plan_buffer(dim, coords, table, res, bw)
    fwd_op = hip_ops.hashgrid_interpolate_cuda if dim == 3 else hip_ops.hashgrid_interpolate2d_cuda
    pk = {} if plan is None else {"plan": plan}

    def second(want, p):
        return lambda: hip_ops.hashgrid_coords_backward2(dim, coords, go, v, table, first, res, bw, want=want, plan=p)

    kinds = {
        "forward": lambda: fwd_op(coords, table, first, res, bw, **pk),
        "bwd_table": lambda: hip_ops.hashgrid_backward(dim, coords, go, T, dt, first, res, bw, F, **pk),
        "bwd_coords": lambda: hip_ops.hashgrid_coords_backward(dim, coords, go, table, first, res, bw, plan=plan),
        "g1": second((True, False, False), plan),
        "g3": second((False, False, True), plan),
        "g1+g3": second((True, False, True), plan),
        "scatter": second((False, True, False), plan),
        "all": second((True, True, True), plan),
    }
    if plan is not None:
        kinds["g1+g3_unsorted"] = second((True, False, True), None)
        kinds["all_unsorted"] = second((True, True, True), None)
    kinds["forward"]()   # the plan of this batch
    for f in kinds.values():
        for _ in range(3):
            f()
    times = {k: [] for k in kinds}
    for _ in range(iters):
        for k, f in kinds.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    stat = {k: {"median": round(float(np.median(t)), 4), "min": round(float(np.min(t)), 4),
                "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4)}
            for k, t in times.items()}
    # the adds of (2): one per feature for every corner whose row lies inside the table (the kernel skips zero weights, i.e.
    # clamped axes: none for coordinates inside the cube); the timed call also zeroes the table first
    rows, _ = hip_ops.hashgrid_debug_corners(dim, coords, res, bw)
    inside = (rows.long() + first.long()[None, :, None]) < T
    adds = int(inside.sum().item()) * F
    rate = adds * 4 / (stat["scatter"]["median"] * 1e-3) / 1e12
    return {"shape": name, "N": N, "planned": plan is not None, "ms": stat, "scatter_adds": adds,
            "scatter_TBps_of_added_bytes": round(rate, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="S1,D256k,D64k,B")
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        print(json.dumps(run(name, args.iters, dev)), flush=True)


if __name__ == "__main__":
    main()
