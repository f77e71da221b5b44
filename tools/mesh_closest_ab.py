"""Closest point on a mesh: ``closest_point`` (signed and unsigned) against ``compute_sdf`` and against an argmin composed of
torch ops, on the same GPU, HIP-event times after warm-up, interleaved.

    python tools/mesh_closest_ab.py [--reps 3] [--torch-fraction 16]

Shape: the reference dataset's resample (MeshSDFDataset: 100 000 samples per technique, techniques rand, rand, near, near,
trace = 500 000 points) against an icosphere of level 6 (81 920 triangles), as tools/mesh_sdf_ab.py.

Legs, all through the Python entry points (operand checks and the workspace cache included):
  closest signed     closest_point(V, F, points): distance with the bits of compute_sdf, closest point, face index
  closest unsigned   closest_point(..., signed=False): no ray stabbing
  compute_sdf        the distance alone (shacira_mesh_sdf)
  torch argmin       mesh_closest_torch(signed=False) on device tensors: the same arithmetic as chunked torch ops over
                     [points, triangles] blocks of 2^25 pairs. Timed on the first 1 / --torch-fraction of the points and
                     scaled: it is far slower, and linear in the number of points.
Before anything is timed the outputs are compared: closest signed against compute_sdf, unsigned against its absolute value,
and the torch leg against the kernel on its subset, bit for bit."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_ref as ref  # noqa: E402
from shacira_amd.wisp.ops.mesh import closest_point, compute_sdf, point_sample  # noqa: E402
from shacira_amd.wisp.ops.mesh.closest_point import mesh_closest_torch  # noqa: E402

RESAMPLE_MODES = ["rand", "rand", "near", "near", "trace"]
RESAMPLE_PER_MODE = 100_000
TORCH_BLOCK_PAIRS = 1 << 25


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-fraction", type=int, default=16, help="the torch leg runs on 1/this of the points (0: skip it)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, F = ref.icosphere(6, 0.7)
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    points = point_sample(Vd, Fd, RESAMPLE_MODES, RESAMPLE_PER_MODE).contiguous()
    tri = Vd[Fd].contiguous()
    N, T = points.shape[0], tri.shape[0]
    legs = {"closest signed": lambda: closest_point(Vd, Fd, points),
            "closest unsigned": lambda: closest_point(Vd, Fd, points, signed=False),
            "compute_sdf": lambda: compute_sdf(Vd, Fd, points)}
    scale = {k: 1 for k in legs}
    if args.torch_fraction > 0:
        # the host path's block size suits a CPU's caches; on the GPU larger blocks mean fewer launches
        importlib.import_module("shacira_amd.wisp.ops.mesh.compute_sdf")._BLOCK_PAIRS = TORCH_BLOCK_PAIRS
        subset = points[:max(1, N // args.torch_fraction)].contiguous()
        legs["torch argmin"] = lambda: mesh_closest_torch(subset, tri, signed=False)
        scale["torch argmin"] = N / subset.shape[0]

    outs = {k: fn() for k, fn in legs.items()}          # warm-up, and the outputs to compare
    torch.cuda.synchronize()
    sdf = outs["compute_sdf"]
    signed, unsigned = outs["closest signed"], outs["closest unsigned"]
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))   # noqa: E731
    print(f"N {N} x T {T}: closest signed dist == compute_sdf bits: {same(signed[0], sdf)}; "
          f"unsigned == |compute_sdf|: {same(unsigned[0], sdf.abs())}; "
          f"hit and face equal between the two: {same(signed[1], unsigned[1]) and torch.equal(signed[2], unsigned[2])}")
    if "torch argmin" in legs:
        d, h, i = outs["torch argmin"]
        n = d.shape[0]
        print(f"torch argmin on {n} points == kernel bits: dist {same(d, unsigned[0][:n, 0])}, hit {same(h, unsigned[1][:n])}, "
              f"face {torch.equal(i.long(), unsigned[2][:n])}")
    inside = float((sdf < 0).float().mean())
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(_time(fn) * scale[k])
    for k, v in times.items():
        med = statistics.median(v)
        note = f"   (timed on 1/{args.torch_fraction} of the points, scaled)" if scale[k] != 1 else ""
        print(f"N {N} x T {T} {k:16s} runs (ms) {' '.join(f'{t:10.3f}' for t in v)}   median {med:10.3f} ms   "
              f"{N * T / med / 1e6:8.2f} G pairs/s{note}")
    base = statistics.median(times["compute_sdf"])
    for k in legs:
        if k != "compute_sdf":
            print(f"N {N} x T {T} {k} / compute_sdf time ratio {statistics.median(times[k]) / base:.3f}x")
    print(f"(inside: {inside:.3f})")


if __name__ == "__main__":
    main()
