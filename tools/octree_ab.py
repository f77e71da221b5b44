"""Octree feature lookup: HIP kernels against the torch composition ``octree_torch`` on the same GPU and build,
interleaved medians with the spread across repetitions.

    python tools/octree_ab.py [--n 1048576] [--reps 30]        -> forward, backward, forward + backward per occupancy / order
    python tools/octree_ab.py --bwd-only --reps 5 [--occ dense] [--order uniform]
                                                                -> backward calls only (for a kernel trace of its own)

Shape: nerf_octree.yaml (feature_dim 5, base_lod 5, 4 LODs, 'sum'); occupancies: dense, and a thin spherical shell at
level 8; batch orders: uniform in the cube, and ray by ray (64 equidistant samples on camera rays through the cube).
Also prints the bytes of global float adds a feature backward issues on each batch, counted from the batch itself."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shacira_amd import harness  # noqa: E402
from shacira_amd.wisp.accelstructs import OctreeAS  # noqa: E402
from shacira_amd.wisp.ops.octree import build_octree_index, octree_interpolate, octree_torch  # noqa: E402


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def shell(level, radius=0.7):
    G = 1 << level
    ax = (torch.arange(G, dtype=torch.float32) + 0.5) * (2.0 / G) - 1.0
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    return OctreeAS(level, (r - radius).abs() < 2.0 / G)


def batches(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    uni = torch.rand(n, 3, device=dev, generator=g) * 2 - 1
    steps = 64
    o, d = harness.camera_rays((n + steps - 1) // steps, torch.Generator().manual_seed(0), dev)
    t = torch.linspace(1.5, 4.5, steps, device=dev)
    rays = (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3)[:n].contiguous()
    return {"uniform": uni, "rays": rays}


def flushed_rows(coords, blas, lods, fdim, cells_log2=3):
    """Global float adds of one feature backward, counted from the batch: per level the distinct (sort block, corner row)
    pairs the samples in occupied cells touch -- what the LDS windows flush -- against the 8 adds per sample before
    combining. ``cells_log2`` = 3 is the block edge ``octree_backward_plan`` picks for this shape (8 cells of level 8). A
    block with more than 512 samples is flushed once per 512, which this count leaves out."""
    fine = max(lods)
    pf = torch.floor((coords + 1.0) * (1 << (fine - 1))).long()
    out, total = [], 0
    for lev in lods:
        hit = blas.query(coords, lev).pidx >= 0
        cell = pf[hit] >> (fine - lev)
        blk = pf[hit] >> cells_log2
        nb = 1 << (fine - cells_log2)
        bkey = (blk[:, 0] * nb + blk[:, 1]) * nb + blk[:, 2]
        S = (1 << lev) + 1
        keys = []
        for k in range(8):
            x, y, z = cell[:, 0] + (k >> 2 & 1), cell[:, 1] + (k >> 1 & 1), cell[:, 2] + (k & 1)
            keys.append(bkey * S ** 3 + (x * S + y) * S + z)
        rows = int(torch.unique(torch.cat(keys)).numel())
        out.append((lev, 8 * int(hit.sum()), rows))
        total += rows
    return out, total * fdim * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bwd-only", action="store_true")
    ap.add_argument("--occ", choices=["dense", "shell"], default=None, help="only this occupancy")
    ap.add_argument("--order", choices=["uniform", "rays"], default=None, help="only this batch order")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lods, fdim = [5, 6, 7, 8], 5
    go = torch.randn(args.n, fdim, device=dev)
    for occ_name, make in (("dense", lambda: OctreeAS.make_dense(8)), ("shell", lambda: shell(8))):
        if args.occ not in (None, occ_name):
            continue
        blas = make()
        index = build_octree_index(blas, lods)
        torch.manual_seed(0)
        tables = [(torch.randn(index[l].rows + 1, fdim, device=dev) * 0.1).requires_grad_(True) for l in lods]
        for l in lods:
            index[l].to(dev).trinkets, index[l].to(dev).cell_codes      # built once, outside the timed region
        for order, coords in batches(args.n, dev).items():
            if args.order not in (None, order):
                continue
            tag = f"{occ_name}/{order}"
            hip_out = octree_interpolate(coords, lods, tables, index, True)
            hits = float((hip_out.detach().abs().sum(-1) > 0).float().mean())
            if args.bwd_only:
                for _ in range(args.reps):
                    torch.autograd.grad(hip_out, tables, go, retain_graph=True)
                torch.cuda.synchronize()
                print(f"{tag}: {args.reps} backward calls done (samples in occupied cells: {hits:.3f})")
                continue
            per_level, nbytes = flushed_rows(coords, blas, lods, fdim)
            for lev, before, rows in per_level:
                print(f"{tag:14s} level {lev}: adds before combining {before:9d}, rows flushed {rows:9d}, "
                      f"ratio {before / max(rows, 1):5.1f}")
            print(f"{tag:14s} global float adds per backward: {nbytes / 1e6:.1f} MB "
                  f"({nbytes / 1.3e12 * 1e3:.3f} ms at 1.3 TB/s)")
            ref_out = octree_torch(coords, lods, tables, index, True)
            print(f"{tag}: samples in occupied cells {hits:.3f}, max |HIP - torch| forward "
                  f"{float((hip_out - ref_out).detach().abs().max()):.3e}")
            legs = {
                "hip fwd": lambda: octree_interpolate(coords, lods, tables, index, True),
                "torch fwd": lambda: octree_torch(coords, lods, tables, index, True),
                "hip bwd": lambda: torch.autograd.grad(hip_out, tables, go, retain_graph=True),
                "torch bwd": lambda: torch.autograd.grad(ref_out, tables, go, retain_graph=True),
                "hip fwd+bwd": lambda: torch.autograd.grad(octree_interpolate(coords, lods, tables, index, True), tables, go),
                "torch fwd+bwd": lambda: torch.autograd.grad(octree_torch(coords, lods, tables, index, True), tables, go),
            }
            times = {k: [] for k in legs}
            for r in range(args.reps + 3):
                for k, fn in legs.items():
                    t = _time(fn)
                    if r >= 3:
                        times[k].append(t)
            med = {k: statistics.median(v) for k, v in times.items()}
            for k, v in times.items():
                lo, hi = np.percentile(v, [10, 90])
                print(f"{tag:14s} {k:14s} median {med[k]:8.3f} ms   p10 {lo:8.3f}   p90 {hi:8.3f}")
            for leg in ("fwd", "bwd", "fwd+bwd"):
                print(f"{tag:14s} speed-up {leg:8s} {med['torch ' + leg] / med['hip ' + leg]:6.1f}x")
            del ref_out, hip_out


if __name__ == "__main__":
    main()
