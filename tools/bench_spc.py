"""Structured point clouds: the fused kernels of spc.hip against the composed paths built from the operators the package had
before them, on the same GPU, and the register counts of the new kernels. Writes a Markdown report (profiles/spc.md).

    python tools/bench_spc.py [--views 64] [--size 400] [--level 8] [--rays 800] [--samples 9] [--out FILE]

The scene is made on the device, no files: a sphere of radius 0.9 at the origin seen from ``--views`` pinhole cameras at
distance 3, depth along this package's own rays, colours from the hit point, background depth NaN.
(a) SPC build at ``--level``: ``hip_ops.spc_from_depth`` (mark, popcount + scan, accumulate, resolve; the cloud is never made)
    against ``hip_ops.depth_points`` + ``pointcloud_to_octree(attributes=...)`` (the compacted cloud, a Morton sort of it and
    ``index_add_``). Peak device bytes of one call of each, above what is resident before it.
(b) First hit of ``--rays`` squared rays of a further camera: ``hip_ops.spc_first_hit`` (one launch) against
    ``PackedSPCTracer.trace_composed`` (every crossing emitted, the first of each ray marked, colours gathered, four scatters).
(c) ``render.raytrace_dense`` alone (count, scan, emit) on the rays of (b): the other visitor of the walk of ``grid_walk.h``,
    which (b) times only under the torch glue of ``trace_composed``. Windows of the same length, no second leg.
Every round times leg A, leg B and leg A again, each a window of back-to-back calls between device events after a warm-up of every
shape; the report gives min / median / max over the rounds, so the spread of a leg against itself is known before two legs are
compared. The outputs of the two legs are compared before anything is timed. No coarse "empty brick" bit was tried in the
tracer: there is one variant of it."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from shacira_amd import hip_ops, render  # noqa: E402
from shacira_amd.wisp.core import Camera, Rays  # noqa: E402
from shacira_amd.wisp.models.nefs import SPCField  # noqa: E402
from shacira_amd.wisp.ops.raygen import camera_records  # noqa: E402
from shacira_amd.wisp.ops.spc import StructuredPointCloud, pointcloud_to_octree  # noqa: E402
from shacira_amd.wisp.tracers import PackedSPCTracer  # noqa: E402

RADIUS = 0.9


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def _fmt(v):
    return f"min {min(v):10.1f} | median {statistics.median(v):10.1f} | max {max(v):10.1f}"


def _cameras(views, size, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    eye = torch.randn(views, 3, generator=gen, dtype=torch.float64)
    eye = 3.0 * eye / eye.norm(dim=1, keepdim=True)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64) + 1e-3 * eye
    return Camera.from_args(eye=eye, at=torch.zeros(3, dtype=torch.float64), up=up, focal_x=1.4 * size, width=size,
                            height=size, near=0.0, far=6.0).to(dev)


def make_scene(views, size, dev):
    """(records, depth fp32 [V, H, W] with NaN off the sphere, images uint8 [V, H, W, 4])."""
    records = camera_records(_cameras(views, size, dev))
    depth = torch.empty((views, size, size), dtype=torch.float32, device=dev)
    images = torch.empty((views, size, size, 4), dtype=torch.uint8, device=dev)
    for v in range(views):
        o, d, _, _ = hip_ops.raygen(records[v:v + 1], size, size)
        o, d = o.double(), d.double()
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - RADIUS ** 2)
        t = -b - disc.clamp_min(0).sqrt()
        hit = disc > 0
        p = o + d * t[:, None]
        rgba = torch.cat([(0.5 + p / (2 * RADIUS)).clamp(0, 1), torch.ones_like(t)[:, None]], -1) * hit[:, None]
        images[v] = (rgba * 255).round().to(torch.uint8).reshape(size, size, 4)
        depth[v] = torch.where(hit, t, torch.full_like(t, float("nan"))).float().reshape(size, size)
    return records, depth, images


def _peak(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def _rounds(leg_a, leg_b, samples, calls):
    a1, b, a2 = [], [], []
    for _ in range(samples):
        a1.append(_window(leg_a, calls))
        b.append(_window(leg_b, calls))
        a2.append(_window(leg_a, calls))
    return a1, b, a2


def _clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        lines = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return lines[:4] if lines else ["rocm-smi --showclocks printed no sclk / mclk line"]
    except Exception as exc:        # the report says so; nothing is set or changed either way
        return [f"clock state not read: {exc!r}"]


def register_table():
    from test_raygen_build import _metadata
    meta = _metadata()
    rows = sorted((k, v) for k, v in meta.items() if any(s in k for s in ("depthcloud_", "spc_", "raygen_", "raysums_")))
    out = ["| kernel | VGPRs | LDS bytes | private bytes |", "|---|---|---|---|"]
    for name, (private, lds, vgprs) in rows:
        short = name.replace("_ZN7shacira12_GLOBAL__N_1", "")[:72]            # the mangled name without its namespaces
        out.append(f"| `{short}` | {vgprs} | {lds} | {private} |")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--rays", type=int, default=800)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spc.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spc.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say("# Structured point clouds: fused kernels against the composed paths")
    say()
    say(f"`python tools/bench_spc.py --views {args.views} --size {args.size} --level {args.level} --rays {args.rays} "
        f"--samples {args.samples}` on {torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName}). Times in microseconds per call: device events around "
        "windows of back-to-back calls, every shape warmed up first. Each round times the fused leg, the composed leg and the "
        "fused leg again; min / median / max are over the rounds.")
    say()
    say("Clock state before the timed windows (read while the device idles, not set):")
    for ln in _clocks():
        say(f"    {ln}")
    say()
    records, depth, images = make_scene(args.views, args.size, dev)
    L = args.level

    # ---- (a) build
    fused = lambda: hip_ops.spc_from_depth(records, depth, images, L)

    def composed():
        pts, cols = hip_ops.depth_points(records, depth, images)
        return pointcloud_to_octree(pts, L, attributes=cols.float())
    words, rank, colors, cells = fused()
    blas, means = composed()
    spc = StructuredPointCloud(L, words, rank, colors, cells)
    assert torch.equal(spc.to_octree_as().occupancy_grid, blas.occupancy_grid.to(dev)), "the two builds disagree on the cells"
    worst = float((spc.colors_morton()[:, :3].float() - means).abs().max())
    assert worst <= 0.5 + 1e-2, worst
    valid = int(torch.isfinite(depth).sum())
    for _ in range(2):
        fused(), composed()
    f1, c, f2 = _rounds(fused, composed, args.samples, 20)
    say(f"## (a) SPC build, level {L}, from {args.views} views of {args.size} x {args.size}")
    say()
    say(f"{valid} valid pixels of {depth.numel()}, {cells} cells. The composed colours are fp32 means; the fused ones are their "
        f"integer rounding (largest difference {worst:.3f} of a byte).")
    say()
    say("| leg | us per call |")
    say("|---|---|")
    say(f"| fused `spc_from_depth`, first window of a round | {_fmt(f1)} |")
    say(f"| composed `depth_points` + `pointcloud_to_octree(attributes=...)` | {_fmt(c)} |")
    say(f"| fused, second window of a round | {_fmt(f2)} |")
    ratio_a = statistics.median(c) / statistics.median(f1 + f2)
    say()
    say(f"Composed / fused (medians): **{ratio_a:.2f}x**. Fused spread: {min(f1 + f2):.1f} .. {max(f1 + f2):.1f} us; composed "
        f"spread: {min(c):.1f} .. {max(c):.1f} us.")
    say()
    pf, pc = _peak(fused, dev), _peak(composed, dev)
    say(f"Peak device bytes of one call above what is resident: fused {pf / 1e6:.1f} MB, composed {pc / 1e6:.1f} MB "
        f"({pc / max(pf, 1):.1f}x).")
    say()
    resident = images.numel() + depth.numel() * 4 + records.numel() * 4
    say(f"Resident: {resident / depth.numel():.2f} bytes per pixel (RGBA bytes, fp32 depth, records) against the reference "
        "layout's 41; a 3-channel image makes it 7.")
    say()

    # ---- (b) tracing
    cam = _cameras(1, args.rays, dev, seed=5)
    o, d, _, _ = hip_ops.raygen(camera_records(cam), args.rays, args.rays)
    rays = Rays(o, d)
    nef, tracer = SPCField(spc), PackedSPCTracer()
    one = lambda: tracer.trace(nef, rays, {"rgb"}, set())
    many = lambda: tracer.trace_composed(nef, rays, {"rgb"}, set())
    ra, rb = one(), many()
    for name in ("depth", "hit", "rgb", "alpha"):
        assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    hits = int(ra.hit.sum())
    for _ in range(2):
        one(), many()
    t1, m, t2 = _rounds(one, many, args.samples, 100)
    say(f"## (b) First hit, {args.rays} x {args.rays} rays against that SPC")
    say()
    say(f"{hits} of {rays.origins.shape[0]} rays hit; the two buffers are equal bit for bit.")
    say()
    say("| leg | us per call |")
    say("|---|---|")
    say(f"| `PackedSPCTracer.trace` (one `spc_first_hit` launch), first window | {_fmt(t1)} |")
    say(f"| `PackedSPCTracer.trace_composed` | {_fmt(m)} |")
    say(f"| `trace`, second window | {_fmt(t2)} |")
    ratio_b = statistics.median(m) / statistics.median(t1 + t2)
    say()
    say(f"Composed / fused (medians): **{ratio_b:.2f}x**. Fused spread: {min(t1 + t2):.1f} .. {max(t1 + t2):.1f} us; composed "
        f"spread: {min(m):.1f} .. {max(m):.1f} us. The coarse empty-brick bit was not tried.")
    say()
    pt, pm = _peak(one, dev), _peak(many, dev)
    say(f"Peak device bytes of one call: fused {pt / 1e6:.1f} MB, composed {pm / 1e6:.1f} MB.")
    say()

    # ---- (c) the dense trace alone
    occ = nef.grid.blas.occupancy_at(L, dev)
    dense = lambda: render.raytrace_dense(o, d, occ, L)
    nuggets = dense()[0].shape[0]
    dense()
    dn = [_window(dense, 100) for _ in range(2 * args.samples)]
    say("## (c) `render.raytrace_dense` alone on the rays of (b)")
    say()
    say(f"{nuggets} nuggets. Count launch, scan (with the read-back of the total that sizes the outputs) and emit launch: what "
        "`trace_composed` spends before its torch glue. Two windows a round, as many as the fused leg of (b).")
    say()
    say("| leg | us per call |")
    say("|---|---|")
    say(f"| `render.raytrace_dense` | {_fmt(dn)} |")
    say()
    say(f"Medians (us): `spc_first_hit` {statistics.median(t1 + t2):.1f} | `trace_composed` {statistics.median(m):.1f} | "
        f"`raytrace_dense` {statistics.median(dn):.1f}")
    say()
    say("## Register counts (gfx950 code objects, `llvm-readelf --notes`)")
    say()
    for ln in register_table():
        say(ln)
    say()
    say("The ray kernels are listed because their body moved into `raygen_device.h`, shared with `spc.hip`: before the move "
        "they took 45 / 46 (`raygen_kernel<false / true>`) and 46 / 47 (`raysums_kernel`) VGPRs.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
