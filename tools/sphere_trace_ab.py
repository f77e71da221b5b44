"""Sphere tracing: ``PackedSDFTracer`` (one fused HIP launch between two evaluations of the field) against the reference's
masked-tensor loop (tests/sphere_trace_ref.py ``trace_literal``, pack ends fixed) run with torch ops on the same GPU, the same
rays, the same field.

    python tools/sphere_trace_ab.py [--side 512] [--level 7] [--reps 5] [--fit-steps 300]

Two fields: the analytic sphere |x| - 0.7 (a torch module), and a ``NeuralSDF`` on an ``OctreeGrid`` over the same shell
occupancy, fitted to that sphere for ``--fit-steps`` Adam steps first so that its trace is a trace of a surface. Rays:
``side * side`` of them from the radius-3 sphere toward uniform points of the cube.

Per field and leg, alternating the legs inside every repetition after one warm-up each:
  whole trace   host clock around raytrace + pack set-up + loop (+ the scatter into per-ray buffers for the fused leg), ending
                in a device synchronise; median over the repetitions
  field         HIP-event time of the field evaluations inside it
  per round     (whole trace - field - raytrace and set-up) / rounds: what one iteration costs outside the field
  operators     ATen operator calls per round outside the field (counted by a dispatch mode in a run of its own), plus the
                library launches the leg makes per round
The two legs' hit flags and hit points are compared bit for bit before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import octree_ref  # noqa: E402
import sphere_trace_ref as ref  # noqa: E402
from shacira_amd import render  # noqa: E402
from shacira_amd.wisp.accelstructs import OctreeAS  # noqa: E402
from shacira_amd.wisp.core import Rays  # noqa: E402
from shacira_amd.wisp.models.grids import OctreeGrid  # noqa: E402
from shacira_amd.wisp.models.nefs import NeuralSDF  # noqa: E402
from shacira_amd.wisp.ops.geometric import pack_ends  # noqa: E402
from shacira_amd.wisp.tracers import PackedSDFTracer  # noqa: E402

MIN_DIS = 0.0003


class ShellGrid:
    def __init__(self, blas, level):
        self.blas, self.active_lods, self.num_lods = blas, [level], 1

    def raytrace(self, rays, level=None, with_exit=False):
        return self.blas.raytrace(rays, level, with_exit=with_exit)


class SphereNef(torch.nn.Module):
    def __init__(self, grid):
        super().__init__()
        self.grid = grid

    def sdf(self, coords, lod_idx=None):
        x = coords
        return dict(sdf=(torch.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) - ref.RADIUS)[:, None])

    def forward(self, channels=None, coords=None, lod_idx=None, pidx=None):
        return self.sdf(coords)[channels]


class Metered(torch.nn.Module):
    """The field with HIP events around every evaluation, and a switch the operator counter reads."""

    def __init__(self, nef):
        super().__init__()
        self.nef, self.grid = nef, nef.grid
        self.events, self.inside = [], False

    def forward(self, **kwargs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.inside = True
        a.record()
        out = self.nef(**kwargs)
        b.record()
        self.inside = False
        self.events.append((a, b))
        return out

    def take_ms(self):
        ms = sum(a.elapsed_time(b) for a, b in self.events)
        calls, self.events = len(self.events), []
        return ms, calls


class OpCounter(TorchDispatchMode):
    def __init__(self, metered):
        super().__init__()
        self.metered, self.count = metered, 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not self.metered.inside:
            self.count += 1
        return func(*args, **(kwargs or {}))


def prepare(nef, rays, lod_idx):
    """What both legs do before their loop: the ray / cell intersections and the packs."""
    traced = nef.grid.raytrace(rays, nef.grid.active_lods[lod_idx], with_exit=True)
    depth = traced.depth
    depth[:, 0] += 1e-5
    first, end = pack_ends(render.mark_pack_boundaries(traced.ridx))
    ray = traced.ridx.index_select(0, first.long()).long()
    return depth, first, end, ray


def loop_leg(nef, rays, lod_idx, num_steps):
    depth, first, end, ray = prepare(nef, rays, lod_idx)
    with torch.no_grad():
        out = ref.trace_literal(rays.origins.index_select(0, ray), rays.dirs.index_select(0, ray), depth, first, end,
                                lambda x: nef(coords=x, lod_idx=lod_idx, channels="sdf"), num_steps, 1.0, MIN_DIS,
                                find_depth_bound=render.find_depth_bound)
    return out["hit"], out["x"], ray, out["iterations"]


def fused_leg(nef, rays, lod_idx, num_steps):
    rb = PackedSDFTracer(num_steps=num_steps, min_dis=MIN_DIS)(nef, rays, channels=("hit", "xyz", "depth"), lod_idx=lod_idx)
    return rb.hit, rb.xyz


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fit_sphere(nef, steps, dev):
    opt = torch.optim.Adam(nef.parameters(), lr=5e-3)
    for _ in range(steps):
        u = torch.nn.functional.normalize(torch.randn(1 << 15, 3, device=dev), dim=-1)
        x = u * (ref.RADIUS + 0.02 * torch.randn(1 << 15, 1, device=dev))
        loss = (nef.sdf(x)["sdf"][:, 0] - (x.norm(dim=-1) - ref.RADIUS)).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num-steps", type=int, default=128)
    ap.add_argument("--fit-steps", type=int, default=300)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is nothing to time without it"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cells = torch.from_numpy(octree_ref.shell_cells(args.level, ref.RADIUS)).to(dev)
    origins, dirs = ref.make_rays(args.side * args.side)
    rays = Rays(torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev))
    blas = OctreeAS.from_quantized_points(cells, args.level)
    sphere = SphereNef(ShellGrid(blas, args.level))
    grid = OctreeGrid.from_quantized_points(cells, feature_dim=4, base_lod=args.level - 2, num_lods=3, feature_std=0.01)
    neural = NeuralSDF(grid, hidden_dim=64, num_layers=1).to(dev)
    print(f"NeuralSDF fit to the sphere: {args.fit_steps} steps, final mean |error| {fit_sphere(neural, args.fit_steps, dev):.2e}")
    for p in neural.parameters():
        p.requires_grad_(False)

    for name, nef, lod_idx in (("analytic sphere", sphere, 0), ("NeuralSDF / OctreeGrid", neural, 2)):
        metered = Metered(nef)
        set_up = statistics.median(timed(lambda: prepare(metered, rays, lod_idx))[0] for _ in range(3))
        hit_l, x_l, ray, rounds_loop = loop_leg(metered, rays, lod_idx, args.num_steps)      # warm-up and the comparison
        metered.take_ms()
        hit_f, x_f = fused_leg(metered, rays, lod_idx, args.num_steps)
        _, calls_fused = metered.take_ms()
        same = torch.equal(hit_f[ray], hit_l) and torch.equal(x_f[ray][hit_l].view(torch.int32), x_l[hit_l].view(torch.int32))
        print(f"{name}: {rays.origins.shape[0]} rays, {ray.shape[0]} packs, {int(hit_l.sum())} hits; the two legs' hit flags and "
              f"hit points are bit-equal: {same}; rounds: loop {rounds_loop}, fused {calls_fused}")
        ops = {}
        for leg, fn in (("loop", loop_leg), ("fused", fused_leg)):
            with OpCounter(metered) as counter:
                fn(metered, rays, lod_idx, args.num_steps)
            ops[leg] = counter.count
            metered.take_ms()
        whole, field = {"loop": [], "fused": []}, {"loop": [], "fused": []}
        for _ in range(args.reps):
            for leg, fn in (("loop", loop_leg), ("fused", fused_leg)):
                ms, _ = timed(lambda: fn(metered, rays, lod_idx, args.num_steps))
                whole[leg].append(ms)
                field[leg].append(metered.take_ms()[0])
        for leg, rounds, extra in (("loop", rounds_loop, "+ 1 find_depth_bound launch"), ("fused", calls_fused, "+ 1 step launch")):
            w, f = statistics.median(whole[leg]), statistics.median(field[leg])
            print(f"  {leg:5s} whole trace (ms) {' '.join(f'{t:8.2f}' for t in whole[leg])}  median {w:8.2f}   field {f:8.2f}   "
                  f"raytrace and set-up {set_up:6.2f}   per round outside the field {(w - f - set_up) / max(rounds, 1) * 1e3:8.1f} us"
                  f"   ATen operator calls per round {ops[leg] / max(rounds, 1):6.1f} {extra}")
        print(f"  loop / fused whole-trace time ratio {statistics.median(whole['loop']) / statistics.median(whole['fused']):.2f}x")


if __name__ == "__main__":
    main()
