"""Mesh to signed distance: the fused kernel of mesh_sdf.hip against its plain variant on the same GPU, HIP-event times after
warm-up, interleaved.

    make -C shacira_amd/csrc variant NAME=mesh_plain FILE=mesh_sdf.hip EXTRA=-DMESH_SDF_PLAIN=1
    python tools/mesh_sdf_ab.py [--reps 3] [--plain shacira_amd/lib/variants/mesh_plain.so] [--also NAME=lib.so ...]

The plain variant is one lane per point with no prologue: every per-triangle quantity recomputed per pair from the vertices
in global memory (the reference kernel's shape). Both libraries are loaded into this process and called through the C ABI on
the same buffers; their outputs are compared bit for bit before anything is timed. ``--also`` adds further builds of the
library (other ``make variant`` outputs) to the same rounds.

Shapes: the reference dataset's resample (MeshSDFDataset: 100 000 samples per technique, techniques rand, rand, near, near,
trace = 500 000 points) against an icosphere of level 6 (81 920 triangles), and 4 096 points against level 3 (1 280)."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_ref as ref  # noqa: E402
from shacira_amd import _lib, hip_ops  # noqa: E402
from shacira_amd.wisp.ops.mesh import point_sample  # noqa: E402

RESAMPLE_MODES = ["rand", "rand", "near", "near", "trace"]
RESAMPLE_PER_MODE = 100_000


def _bind(handle):
    name = "shacira_mesh_sdf"
    fn = getattr(handle, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return fn


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
    ap.add_argument("--plain", default=os.path.join(ROOT, "shacira_amd", "lib", "variants", "mesh_plain.so"))
    ap.add_argument("--also", action="append", default=[], metavar="NAME=LIB", help="another build to time in the same rounds")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    legs = {"fused": _bind(_lib.lib())}
    if os.path.exists(args.plain):
        legs["plain"] = _bind(ctypes.CDLL(args.plain))
    else:
        print(f"no plain variant at {args.plain}: timing without it")
    for item in args.also:
        name, _, path = item.partition("=")
        legs[name] = _bind(ctypes.CDLL(os.path.abspath(path)))
    torch.manual_seed(0)
    for level, modes, per_mode in ((6, RESAMPLE_MODES, RESAMPLE_PER_MODE), (3, ["rand"], 4096)):
        V, F = ref.icosphere(level, 0.7)
        Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
        points = point_sample(Vd, Fd, modes, per_mode).contiguous()
        tri = Vd[Fd].contiguous()
        N, T = points.shape[0], tri.shape[0]
        nbytes = int(_lib.lib().shacira_mesh_sdf_workspace_bytes(N, T))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        outs = {k: torch.empty(N, dtype=torch.float32, device=dev) for k in legs}

        def call(k):
            rc = legs[k](N, T, points.data_ptr(), tri.data_ptr(), outs[k].data_ptr(), ws.data_ptr(), nbytes, stream)
            assert rc == 0, (k, rc)

        for k in legs:          # warm-up, and the outputs to compare
            call(k)
        torch.cuda.synchronize()
        assert torch.equal(outs["fused"], hip_ops.mesh_sdf(points, tri))
        for k in legs:
            if k != "fused":
                same = torch.equal(outs["fused"].view(torch.int32), outs[k].view(torch.int32))
                print(f"N {N} x T {T}: fused and {k} outputs bit-equal: {same}")
        inside = float((outs["fused"] < 0).float().mean())
        times = {k: [] for k in legs}
        for _ in range(args.reps):
            for k in legs:
                times[k].append(_time(lambda: call(k)))
        for k, v in times.items():
            med = statistics.median(v)
            print(f"N {N} x T {T} {k:6s} runs (ms) {' '.join(f'{t:9.3f}' for t in v)}   median {med:9.3f} ms   "
                  f"{N * T / med / 1e6:8.2f} G pairs/s   (inside: {inside:.3f})")
        for k in legs:
            if k != "fused":
                print(f"N {N} x T {T} {k} / fused time ratio {statistics.median(times[k]) / statistics.median(times['fused']):.2f}x")


if __name__ == "__main__":
    main()
