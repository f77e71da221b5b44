"""Mesh point sampling: the fused kernel of mesh_sample.hip (``hip_ops.mesh_sample``, the seeded path of ``wisp.ops.mesh``)
against the torch-op chains it stands beside (``seed=None``), on the same GPU, device events around windows of back-to-back calls.

    python tools/mesh_sample_ab.py [--n 500000] [--samples 5] [--calls 10] [--level 7] [--out FILE]

Meshes: icosphere(5) (20 480 faces) and a procedural torus of 262 144 faces. Legs, each warmed up before anything is timed:
  technique     'trace' / 'near' / 'rand' at ``--n`` samples: one kernel launch against sample_surface / sample_near_surface /
                sample_uniform (host rand + copy, as point_sample calls it), and the default five-technique ``point_sample``
  pool          the narrowband pool of OctreeSampledSDFDataset at ``--level`` (icosphere(5) scaled to 0.6, 32 samples per cell,
                the default five techniques): five filtered kernel calls (count, scan, read-back, write) + cat, against
                sample_spc / sample_near_surface / sample_surface + cat + OctreeAS.query + boolean index
  resample      MeshSampledSDFDataset.resample() at 100 000 samples per technique, split into sampling and distance
Per round one window of the kernel between two windows of the chain, so the chain's own band is known."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mesh_sdf_ref import icosphere  # noqa: E402
from shacira_amd import hip_ops  # noqa: E402
from shacira_amd.wisp.accelstructs import OctreeAS  # noqa: E402
from shacira_amd.wisp.ops import mesh, spc  # noqa: E402

MODES = ["rand", "rand", "near", "near", "trace"]


def torus(nu=512, nv=256, R=0.6, r=0.25):
    """(V [nu * nv, 3], F [2 * nu * nv, 3]): a torus around the y axis."""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    V = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R + r * np.cos(v)) * np.sin(u)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    F = np.concatenate([np.stack([a, b, c], axis=-1).reshape(-1, 3), np.stack([a, c, d], axis=-1).reshape(-1, 3)])
    return V.astype(np.float32), F.astype(np.int64)


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def _fmt(v):
    return f"min {min(v):9.1f}  median {statistics.median(v):9.1f}  max {max(v):9.1f}"


def compare(say, name, kernel, chain, samples, calls):
    for fn in (kernel, chain):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    tk, tc = [], []
    for _ in range(samples):
        tc.append(_window(chain, calls))
        tk.append(_window(kernel, calls))
        tc.append(_window(chain, calls))
    say(f"{name} kernel  us/call  {_fmt(tk)}   ({len(tk)} windows of {calls} calls)")
    say(f"{name} chain   us/call  {_fmt(tc)}   ({len(tc)} windows of {calls} calls)")
    km = statistics.median(tk)
    verdict = "below" if km < min(tc) else ("above" if km > max(tc) else "inside")
    say(f"{name}: kernel median {km:.1f} us is {verdict} the chain's band {min(tc):.1f} .. {max(tc):.1f} us "
        f"(ratio of medians {statistics.median(tc) / km:.2f}x)")


def techniques(say, dev, name, V, F, n, samples, calls):
    V, F = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    tri = V[F]
    cdf = hip_ops.mesh_face_cdf(tri)
    distrib = mesh.area_weighted_distribution(V, F)
    say(f"--- {name}: {F.shape[0]} faces, n = {n} per technique")
    compare(say, f"{name} trace", lambda: hip_ops.mesh_sample("surface", n, seed=1, triangles=tri, cdf=cdf, want_normals=True),
            lambda: mesh.sample_surface(V, F, n, distrib), samples, calls)
    compare(say, f"{name} near ", lambda: hip_ops.mesh_sample("near", n, seed=1, triangles=tri, cdf=cdf, sigma=0.01),
            lambda: mesh.sample_near_surface(V, F, n, distrib=distrib), samples, calls)
    compare(say, f"{name} rand ", lambda: hip_ops.mesh_sample("cube", n, seed=1, device=dev),
            lambda: mesh.sample_uniform(n).to(device=dev), samples, calls)
    compare(say, f"{name} point_sample x5", lambda: mesh.point_sample(V, F, MODES, n, seed=1, distrib=cdf),
            lambda: mesh.point_sample(V, F, MODES, n), samples, calls)


def pool(say, dev, level, samples, calls):
    V, F = icosphere(5, 0.6)
    V, F = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    blas = OctreeAS.from_triangles(V, F, level)
    tri, corners, words = V[F], blas.points.to(dev), blas.packed_occupancy(level)
    cdf = hip_ops.mesh_face_cdf(tri)
    n = corners.shape[0] * 32
    sigma = 1.0 / 2 ** level

    def kernel():
        out = []
        for k, m in sorted(enumerate(MODES), key=lambda km: km[1] != "rand"):
            kw = dict(seed=1, segment=k, occupancy=words, occupancy_level=level)
            if m == "rand":
                out.append(hip_ops.mesh_sample("cells", corners=corners, samples_per_cell=32, cell_level=level, **kw).points)
            else:
                out.append(hip_ops.mesh_sample("near" if m == "near" else "surface", n, triangles=tri, cdf=cdf, sigma=sigma,
                                               **kw).points)
        return torch.cat(out)

    def chain():
        pts = [spc.sample_spc(corners, level, 32) for m in MODES if m == "rand"]
        for m in MODES:
            if m == "near":
                pts.append(mesh.sample_near_surface(V, F, n, variance=sigma))
            elif m == "trace":
                pts.append(mesh.sample_surface(V, F, n)[0])
        pts = torch.cat(pts)
        return pts[blas.query(pts).pidx > -1]

    k, c = kernel(), chain()
    say(f"--- pool: level {level}, {corners.shape[0]} cells, {n} samples per segment; kept {k.shape[0]} (kernel) / {c.shape[0]} "
        f"(chain) of {5 * n}")
    compare(say, f"pool level {level}", kernel, chain, samples, calls)


def resample(say, dev, samples):
    V, F = icosphere(5, 1.0)
    V, F = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    cdf = hip_ops.mesh_face_cdf(V[F])
    n = 100000
    ts, td = [], []
    for r in range(samples + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        pts = mesh.point_sample(V, F, MODES, n, seed=r, distrib=cdf)
        e[1].record()
        mesh.compute_sdf(V, F, pts)
        e[2].record()
        e[2].synchronize()
        if r:                                       # the first round warms up
            ts.append(e[0].elapsed_time(e[1]) * 1e3)
            td.append(e[1].elapsed_time(e[2]) * 1e3)
    say(f"--- resample: icosphere(5), {n} per technique, {5 * n} points")
    say(f"resample sampling  us  {_fmt(ts)}")
    say(f"resample distance  us  {_fmt(td)}")
    say(f"resample: sampling is {100 * statistics.median(ts) / (statistics.median(ts) + statistics.median(td)):.3f} % of the call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time without it"
    dev = torch.device("cuda:0")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(f"device: {torch.cuda.get_device_name(0)}")
    techniques(say, dev, "icosphere(5)", *icosphere(5), args.n, args.samples, args.calls)
    techniques(say, dev, "torus", *torus(), args.n, args.samples, args.calls)
    pool(say, dev, args.level, args.samples, max(1, args.calls // 2))
    resample(say, dev, args.samples)


if __name__ == "__main__":
    main()
