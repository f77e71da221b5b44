"""Mesh to occupancy: the HIP rasteriser (``wisp.ops.spc.mesh_to_octree``, mesh_voxelize.hip) against the reference's method
restated with this package's own torch operators, on the same GPU. Host-clock times around a window of ``--calls`` calls that
ends in a device synchronise, divided by the number of calls, after warm-up, the legs interleaved.

    python tools/mesh_voxelize_ab.py [--reps 5] [--calls 20] [--levels 7 8] [--samples 10000000 100000000]

The reference's method (its ``mesh_to_octree``): ``num_samples`` surface samples and a copy of them displaced, per axis, by a
uniform offset of at most 1 / 2^(level + 1) in cube coordinates -- a QUARTER of a cell, the cell being 2 / 2^level wide --
both quantised into cells. Such a sample lies within 0.75 cell, per axis, of the centre of its cell, so the limit of the method
is the exact set of margin 0.25, not of the default margin 0.5. Reported per level: the kernel sequence alone
(``hip_ops.mesh_voxelize``: zeroing, prologue, scan, pair kernel, finish), ``mesh_to_octree`` end to end (plus the Morton-ordered
cell list of ``OctreeAS``), the sampling run per sample count, and per sampling run its true holes (cells of the margin-0.25
set it misses), the cells it marks outside that set, and the cells of the default margin-0.5 set that are beyond its reach.

Mesh: an icosphere of level 6 (81 920 triangles, the mesh of profiles/mesh_sdf.md), radius 0.7."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_ref as ref  # noqa: E402
from shacira_amd import hip_ops  # noqa: E402
from shacira_amd.wisp.accelstructs import OctreeAS  # noqa: E402
from shacira_amd.wisp.ops.mesh import sample_surface  # noqa: E402
from shacira_amd.wisp.ops.spc import mesh_to_octree  # noqa: E402


def sampled_octree(V, F, level, num_samples):
    quarter_cell = 0.5 / (1 << level)                       # in cube coordinates: a cell is 2 / 2^level wide
    on_surface = sample_surface(V, F, num_samples)[0]
    displaced = on_surface + torch.empty_like(on_surface).uniform_(-quarter_cell, quarter_cell)
    return OctreeAS.from_pointcloud(torch.cat([on_surface, displaced]), level)


def _time(fn, calls=1):
    """(milliseconds per call over a window of ``calls`` calls ending in a device synchronise, the last result)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window (sampling legs: a tenth of it, at least 1)")
    ap.add_argument("--levels", type=int, nargs="+", default=[7, 8])
    ap.add_argument("--samples", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--mesh-level", type=int, default=6)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, F = ref.icosphere(args.mesh_level, 0.7)
    V, F = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    tri = V[F].contiguous()
    torch.manual_seed(0)
    for level in args.levels:
        legs = {"kernels": lambda: hip_ops.mesh_voxelize(tri, level, 0.5), "mesh_to_octree": lambda: mesh_to_octree(V, F, level)}
        for n in args.samples:
            legs[f"sampling {n:.0e}"] = (lambda n: lambda: sampled_octree(V, F, level, n))(n)
        wide = mesh_to_octree(V, F, level).occupancy_grid                      # the default, margin 0.5
        limit = mesh_to_octree(V, F, level, margin=0.25).occupancy_grid        # the limit set of the sampling
        print(f"level {level}: margin 0.5 set {int(wide.sum())} cells, margin 0.25 set {int(limit.sum())} cells "
              f"({int((limit & ~wide).sum())} of them outside the margin 0.5 set)")
        times = {k: [] for k in legs}
        for k in list(legs):        # warm-up; a sample count that does not fit is dropped
            try:
                out = _time(legs[k])[1]
            except torch.OutOfMemoryError:
                print(f"level {level} {k}: does not fit")
                del legs[k], times[k]
                torch.cuda.empty_cache()
                continue
            if k.startswith("sampling"):
                got = out.occupancy_grid
                print(f"level {level} {k}: {int(got.sum())} cells, holes (cells of the margin 0.25 set missed) "
                      f"{int((limit & ~got).sum())}, marked outside the margin 0.25 set {int((got & ~limit).sum())}, outside "
                      f"the margin 0.5 set {int((got & ~wide).sum())}; cells of the margin 0.5 set not marked "
                      f"{int((wide & ~got).sum())}")
            del out
        for _ in range(args.reps):
            for k in legs:
                times[k].append(_time(legs[k], max(1, args.calls // 10) if k.startswith("sampling") else args.calls)[0])
        for k, v in times.items():
            print(f"level {level} T {tri.shape[0]} {k:16s} ms per call {' '.join(f'{t:9.3f}' for t in v)}   median "
                  f"{statistics.median(v):9.3f} ms")
        for k in times:
            if k.startswith("sampling"):
                print(f"level {level} {k} / mesh_to_octree time ratio "
                      f"{statistics.median(times[k]) / statistics.median(times['mesh_to_octree']):.1f}x")


if __name__ == "__main__":
    main()
