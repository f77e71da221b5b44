"""Coordinate backward of the hash-grid operator: timing against the forward of the same batch, and bit equality of its
variants (option coord_variant).

    python tools/coord_grad_ab.py [--shapes S1,lego,lego16,B,D64k] [--iters 30]

Per shape, HIP-event times of (a) the coordinate backward alone, every variant, (b) the forward alone in the same process
(the yardstick), (c) the full backward (codebook gradient) without and with the coordinate gradient. Calls are warmed up,
then timed round-robin (one call of each kind per round) and reported as medians. Planned shapes (a plan exists for the
batch) run the forward and both backwards with the batch's plan, as the autograd wrapper does. One JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shacira_amd import _lib, hip_ops  # noqa: E402


def geo(mn, mx, L):
    b = np.exp((np.log(mx) - np.log(mn)) / (L - 1))
    return [int(1 + np.floor(mn * (b ** l))) for l in range(L)]


SHAPES = {   # name: (dim, resolutions, bitwidth, F, N, table dtype)
    "S1": (3, geo(16, 2048, 16), 19, 2, 1 << 20, torch.float32),
    "lego": (3, geo(16, 512, 24), 19, 4, 409_600, torch.float32),
    "lego16": (3, geo(16, 512, 24), 19, 4, 409_600, torch.float16),
    "B": (2, geo(16, 512, 16), 11, 2, 393_216, torch.float32),
    "D64k": (3, geo(16, 2048, 16), 19, 2, 65_536, torch.float32),
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
    plan = hip_ops.hashgrid_plan_buffer(dim, coords, table, res, bw)
    fwd_op = hip_ops.hashgrid_interpolate_cuda if dim == 3 else hip_ops.hashgrid_interpolate2d_cuda
    pk = {} if plan is None else {"plan": plan}

    def fwd():
        fwd_op(coords, table, first, res, bw, **pk)

    def coord(v):
        def f():
            _lib.set_option("coord_variant", v)
            hip_ops.hashgrid_coords_backward(dim, coords, go, table, first, res, bw, plan=plan)
        return f

    def bwd_table():
        hip_ops.hashgrid_backward(dim, coords, go, T, dt, first, res, bw, F, **pk)

    def bwd_both():
        hip_ops.hashgrid_backward(dim, coords, go, T, dt, first, res, bw, F, **pk)
        hip_ops.hashgrid_coords_backward(dim, coords, go, table, first, res, bw, plan=plan)

    fwd()   # the plan of this batch (the backward reads it)
    variants = [0, 3] + ([8] if plan is not None else [])
    outs = {}
    for v in [-1] + variants:
        _lib.set_option("coord_variant", v)
        outs[v] = hip_ops.hashgrid_coords_backward(dim, coords, go, table, first, res, bw, plan=plan)
    _lib.set_option("coord_variant", -1)
    bit_equal = all(torch.equal(outs[v], outs[-1]) for v in variants)
    kinds = {"forward": fwd, "bwd_table": bwd_table, "bwd_table_and_coords": bwd_both}
    for v in [-1] + variants:
        kinds[f"coords_v{v}"] = coord(v)
    for f in kinds.values():
        for _ in range(3):
            f()
    _lib.set_option("coord_variant", -1)
    times = {k: [] for k in kinds}
    for _ in range(iters):
        for k, f in kinds.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
        _lib.set_option("coord_variant", -1)
    med = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    return {"shape": name, "N": N, "dtype": str(dt).split(".")[-1], "planned": plan is not None, "bit_equal": bit_equal,
            "median_ms": med, "coords_over_forward": round(med["coords_v-1"] / med["forward"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="S1,lego,lego16,B,D64k")
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ok = True
    for name in args.shapes.split(","):
        r = run(name, args.iters, dev)
        ok = ok and r["bit_equal"]
        print(json.dumps(r), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
