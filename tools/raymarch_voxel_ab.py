"""The voxel march: the fused seeded kernels of render.hip (``OctreeAS.raymarch(..., "voxel", seed=...)``) against the composed
torch chain that the same call runs without a seed (``OctreeAS._raymarch_voxel``: raytrace_dense, then about twenty torch
operators), on the same GPU, device events around windows of back-to-back calls.

    python tools/raymarch_voxel_ab.py [--rays 4096] [--samples 7] [--calls 50] [--steps 20] [--out FILE]

March alone, two shapes: (a) ``--rays`` rays of ``harness.camera_rays``, level 7, 16 samples per crossed cell, occupancy a
spherical shell of radius 0.6, two cells thick (the VQ-AD configuration's march); (b) the same rays through AxisAlignedBBoxAS, 512
samples (the triplanar configuration's). Per shape, after a warm-up of both legs and a comparison of the nuggets: ``--samples``
rounds, each one window of the fused march between TWO of the composed one, so the composed leg's own min .. max band is known; a
window is ``--calls`` calls between two events (both legs read one count back per call, so a call ends in a synchronise). The
kernel launches of one call (torch.profiler) and its peak temporary bytes (the allocator's peak over the call) are printed too.

The traced training step on shape (a): PackedRFTracer forward + L1 to the closed-form scene's colours + backward through a hash
grid and its decoders, composed against fused (eager both); then the fused step with Adam, eager against replayed from a HIP graph
(harness.GraphedNerfFitter)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import harness  # noqa: E402
from shacira_amd.wisp.accelstructs import AxisAlignedBBoxAS, OctreeAS  # noqa: E402
from shacira_amd.wisp.core import Rays  # noqa: E402
from shacira_amd.wisp.tracers import PackedRFTracer  # noqa: E402


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


def _launches(fn):
    """Kernel launches of one call, None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as exc:   # noqa: BLE001 -- a count is a courtesy: the timings do not depend on it
        print(f"(launch count not taken: {type(exc).__name__}: {str(exc)[:120]})")
        return None


def _peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    kept = sum(t.numel() * t.element_size() for t in out if torch.is_tensor(t))
    return peak, kept


def shell_occupancy(level, radius=0.6, cells=2.0):
    G = 1 << level
    c = (torch.arange(G, dtype=torch.float32) + 0.5) * (2.0 / G) - 1.0
    r = torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    return (r - radius).abs() <= 0.5 * cells * (2.0 / G)


def _compare(legs, samples, calls, say, unit="us/call"):
    """legs: (name of the baseline, fn), (name of the candidate, fn). Baseline windows before and after every candidate window."""
    (bname, base), (cname, cand) = legs
    t = {bname: [], cname: []}
    for _ in range(samples):
        t[bname].append(_window(base, calls))
        t[cname].append(_window(cand, calls))
        t[bname].append(_window(base, calls))
    for k, v in t.items():
        say(f"{k:18s} {unit}  {_fmt(v)}   ({len(v)} windows of {calls} calls)")
    cm, b = statistics.median(t[cname]), t[bname]
    verdict = "below" if max(t[cname]) < min(b) else ("median below" if cm < min(b) else "NOT below")
    say(f"{cname} median {cm:.1f} is {verdict} the {bname} band {min(b):.1f} .. {max(b):.1f} "
        f"(ratio of medians {statistics.median(b) / cm:.2f}x)")


def march_shapes(dev, rays, samples, calls, say):
    o, d = harness.camera_rays(rays, torch.Generator().manual_seed(0), dev)
    batch = Rays(o, d, dist_min=0.0, dist_max=6.0)
    shell = OctreeAS(7, shell_occupancy(7).to(dev))
    shapes = [("(a) level 7 shell, 16 samples per cell", shell, 7, 16), ("(b) AxisAlignedBBoxAS, 512 samples", AxisAlignedBBoxAS(), 0, 512)]
    for name, blas, level, ns in shapes:
        composed = lambda: blas.raymarch(batch, "voxel", ns, level=level)
        fused = lambda: blas.raymarch(batch, "voxel", ns, level=level, seed=7, step=3)
        for fn in (composed, fused):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        c, f = composed(), fused()
        rows = f.ridx.shape[0]
        say(f"## march alone, {name}: {rays} rays, {rows // ns} nuggets, {rows} rows")
        assert torch.equal(c.ridx, f.ridx) and torch.equal(c.boundary, f.boundary) and rows > 0
        assert c.samples.shape == f.samples.shape and f.ray_offsets is not None and int(f.ray_offsets[-1]) == rows
        for leg, fn in (("composed", composed), ("fused", fused)):
            peak, kept = _peak_bytes(fn)
            say(f"{leg:9s} kernel launches per call {_launches(fn)}; peak bytes over a call {peak} of which returned {kept} "
                f"(temporaries {peak - kept})")
        _compare((("composed", composed), ("fused", fused)), samples, calls, say)
        say("")


def traced_step(dev, rays, samples, steps, say):
    from shacira_amd.wisp.models.grids import HashGrid
    from shacira_amd.wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    level, ns = 7, 16
    grid = HashGrid.from_geometric(feature_dim=2, num_lods=16, multiscale_type="cat", resolution_dim=3, feature_std=0.01,
                                   codebook_bitwidth=19, min_grid_res=16, max_grid_res=2048, blas_level=level)
    grid.blas = OctreeAS(level, shell_occupancy(level))
    nef = NeuralRadianceField(grid, view_embedder="positional", view_multires=4, hidden_dim=64, num_layers=1).to(dev)
    truth = harness._AnalyticNef(grid)
    gen = torch.Generator().manual_seed(1)
    pool_o, pool_d, pool_rgb = [], [], []
    gt = PackedRFTracer(raymarch_type="voxel", num_steps=ns, bg_color="white", seed=99)
    with torch.no_grad():
        for _ in range(8):
            o, d = harness.camera_rays(rays, gen, dev)
            pool_o.append(o)
            pool_d.append(d)
            pool_rgb.append(gt(truth, Rays(o, d, dist_min=0.0, dist_max=6.0)).rgb)
    batch, target = Rays(pool_o[0], pool_d[0], dist_min=0.0, dist_max=6.0), pool_rgb[0]

    def step_of(tracer):
        def step():
            nef.zero_grad(set_to_none=True)
            rb = tracer(nef, batch)
            torch.abs(rb.rgb[..., :3] - target[..., :3]).mean().backward()
        return step

    composed = step_of(PackedRFTracer(raymarch_type="voxel", num_steps=ns, bg_color="white"))
    fused = step_of(PackedRFTracer(raymarch_type="voxel", num_steps=ns, bg_color="white", seed=7))
    for fn in (composed, fused):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    say(f"## traced step (forward + L1 + backward), shape (a): {rays} rays, hash grid 16 levels x 2^19, decoders 64 wide")
    for leg, fn in (("composed", composed), ("fused", fused)):
        say(f"{leg:9s} kernel launches per step {_launches(fn)}")
    _compare((("composed", composed), ("fused", fused)), samples, steps, say, unit="us/step")
    say("")
    # the fused step with Adam: eager against replayed
    tracer = PackedRFTracer(raymarch_type="voxel", num_steps=ns, bg_color="white", seed=7)
    groups = [g for g in harness.param_groups(nef, lr=1e-3, grid_lr=1e-2) if g["params"]]
    fitter = harness.GraphedNerfFitter(nef, tracer, groups, (torch.stack(pool_o), torch.stack(pool_d), torch.stack(pool_rgb)),
                                       0.0, 6.0, dev)
    for _ in range(3):
        fitter._body()
    fitter.prepare()
    torch.cuda.synchronize()
    say(f"## fused step with Adam, eager against graph replay: capacity {fitter.capacity} rows")

    def eager():
        fitter.blas.sample_capacity = None
        fitter._body()

    for _ in range(3):
        eager()
        fitter.graph.replay()
    _compare((("fused eager", eager), ("fused graphed", fitter.graph.replay)), samples, steps, say, unit="us/step")
    say(f"overflow steps {int(fitter.overflow)} (graphed steps whose rows exceeded the capacity)")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    march_shapes(dev, args.rays, args.samples, args.calls, say)
    traced_step(dev, args.rays, args.samples, args.steps, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
