"""Triplane sampling: HIP kernels against the torch grid_sample composition (the reference's hot path), interleaved medians.

    python tools/triplane_ab.py [--n 2097152] [--reps 30]        -> forward, backward, forward + backward per batch order
    python tools/triplane_ab.py --bwd-only --reps 5               -> backward calls only (for a counter run of its own)

Shape: nerf_triplanar.yaml (feature_dim 4, base_lod 5, 4 LODs, 'sum'); batch orders: uniform in the cube, and ray by ray
from the AABB voxel marcher (4096 rays x 512 steps). Also times the forward's two plane layouts (option triplane_layout)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shacira_amd import _lib, harness  # noqa: E402
from shacira_amd.wisp.accelstructs import AxisAlignedBBoxAS  # noqa: E402
from shacira_amd.wisp.core import Rays  # noqa: E402
from shacira_amd.wisp.ops.triplane import triplane_interpolate, triplane_torch  # noqa: E402


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def batches(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    uni = torch.rand(n, 3, device=dev, generator=g) * 2 - 1
    o, d = harness.camera_rays(4096, torch.Generator().manual_seed(0), dev)
    torch.manual_seed(0)
    rays = AxisAlignedBBoxAS().raymarch(Rays(o, d, 1.0, 5.0), raymarch_type="voxel", num_samples=512, level=0).samples
    reps = (n + rays.shape[0] - 1) // rays.shape[0]
    return {"uniform": uni, "rays": rays.repeat(reps, 1)[:n].contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bwd-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lods = [5, 6, 7, 8]
    torch.manual_seed(0)
    planes = [(torch.randn(1, 4, 2 ** l + 1, 2 ** l + 1, device=dev) * 0.1).requires_grad_(True) for l in lods for _ in
              range(3)]
    go = torch.randn(args.n, 12, device=dev)
    for order, coords in batches(args.n, dev).items():
        hip_out = triplane_interpolate(coords, lods, planes, True)
        if args.bwd_only:
            for _ in range(args.reps):
                torch.autograd.grad(hip_out, planes, go, retain_graph=True)
            torch.cuda.synchronize()
            print(f"{order}: {args.reps} backward calls done")
            continue
        ref_out = triplane_torch(coords, planes, len(lods), True)
        print(f"{order}: max |HIP - torch| forward {float((hip_out - ref_out).abs().max()):.3e}")
        legs = {
            "hip fwd": lambda: triplane_interpolate(coords, lods, planes, True),
            "torch fwd": lambda: triplane_torch(coords, planes, len(lods), True),
            "hip bwd": lambda: torch.autograd.grad(hip_out, planes, go, retain_graph=True),
            "torch bwd": lambda: torch.autograd.grad(ref_out, planes, go, retain_graph=True),
            "hip fwd+bwd": lambda: torch.autograd.grad(triplane_interpolate(coords, lods, planes, True), planes, go),
            "torch fwd+bwd": lambda: torch.autograd.grad(triplane_torch(coords, planes, len(lods), True), planes, go),
        }

        def layout(v):
            def run():
                _lib.set_option("triplane_layout", v)
                t = _time(lambda: triplane_interpolate(coords, lods, planes, True))
                _lib.set_option("triplane_layout", -1)
                return t
            return run
        times = {k: [] for k in list(legs) + ["hip fwd NCHW", "hip fwd HWC"]}
        for r in range(args.reps + 3):
            for k, fn in legs.items():
                t = _time(fn)
                if r >= 3:
                    times[k].append(t)
            for k, v in (("hip fwd NCHW", 0), ("hip fwd HWC", 1)):
                t = layout(v)()
                if r >= 3:
                    times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in med.items():
            print(f"{order:8s} {k:14s} {v:8.3f} ms")
        for leg in ("fwd", "bwd", "fwd+bwd"):
            print(f"{order:8s} speed-up {leg:8s} {med['torch ' + leg] / med['hip ' + leg]:6.1f}x")


if __name__ == "__main__":
    main()
