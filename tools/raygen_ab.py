"""Ray generation: the fused kernel of raygen.hip (``hip_ops.raygen``) against this package's own torch composite
(``wisp.ops.raygen.composite_rays``) on the same GPU, device events around batches of back-to-back calls. There is no older
ray generation in this repository to compare with: the composite is the only other way it has to make a ray.

    python tools/raygen_ab.py [--views 100] [--size 800] [--samples 9] [--calls 200] [--out FILE]

Cameras on the radius-3 sphere, ``--views`` RGBA images of ``--size`` squared with random bytes. Three shapes: ``sample()``-style
batches of 4 096 and 65 536 random (view, pixel) pairs over all views, and one whole view. Per shape, after a warm-up of every leg
and a comparison of the outputs: ``--samples`` rounds, each round one window of the kernel and TWO of the composite (before and
after it), so the composite's own min .. max band is known; a window is ``--calls`` calls between two events, the figure its time
over the calls. Legs: the kernel; the composite with the dataset's fp64 cameras (what a host-side caller gets, run on the device);
the composite with the cameras cast to fp32 (the same operator chain at the kernel's precision); and ONE fill of 37 n bytes -- a
kernel that does nothing but store the bytes the ray kernel writes (9 floats and a mask byte per ray).

The resident bytes of a dataset against the reference's layout are printed from the counters of a NeRFSyntheticDataset loaded from
four views written to a temporary directory."""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import hip_ops  # noqa: E402
from shacira_amd.wisp.core import Camera  # noqa: E402
from shacira_amd.wisp.ops.raygen import camera_records, composite_rays  # noqa: E402


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def _fmt(v):
    return f"min {min(v):8.1f}  median {statistics.median(v):8.1f}  max {max(v):8.1f}"


def time_shapes(dev, views, size, samples, calls, say):
    gen = torch.Generator().manual_seed(0)
    eye = torch.randn(views, 3, generator=gen, dtype=torch.float64)
    eye = 3.0 * eye / eye.norm(dim=1, keepdim=True)
    cams = Camera.from_args(eye=eye, at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0], fov=0.69, width=size, height=size, near=0.0,
                            far=6.0).to(dev)
    cams32 = cams.to(torch.float32)
    records = camera_records(cams)
    images = torch.randint(0, 256, (views, size, size, 4), dtype=torch.uint8, device=dev)
    hw = size * size
    say(f"# {views} views of {size} x {size} RGBA: images {images.numel() / 1e6:.1f} MB, records {records.numel() * 4} bytes")
    dgen = torch.Generator(device=dev).manual_seed(1)
    shapes = [("sample 4 096", 4096, None), ("sample 65 536", 65536, None), (f"whole view ({hw} rays)", hw, views // 3)]
    for name, n, whole in shapes:
        if whole is None:
            vi = torch.randint(0, views, (n,), device=dev, dtype=torch.int32, generator=dgen)
            pi = torch.randint(0, hw, (n,), device=dev, dtype=torch.int32, generator=dgen)
            kernel = lambda: hip_ops.raygen(records, size, size, vi, pi, None, images, "white")
            comp64 = lambda: composite_rays(cams, vi, pi, None, images, "white")
            comp32 = lambda: composite_rays(cams32, vi, pi, None, images, "white")
        else:
            rec1, img1, cam1, cam1_32 = records[whole:whole + 1], images[whole:whole + 1], cams[whole], cams32[whole]
            kernel = lambda: hip_ops.raygen(rec1, size, size, None, None, None, img1, "white", num_rays=hw)
            comp64 = lambda: composite_rays(cam1, None, None, None, img1, "white")
            comp32 = lambda: composite_rays(cam1_32, None, None, None, img1, "white")
        sink = torch.empty(37 * n, dtype=torch.uint8, device=dev)
        stores = lambda: sink.fill_(1)
        for fn in (kernel, comp64, comp32, stores):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        (o, d, rgb, mask), (r64, rgb64, mask64) = kernel(), comp64()
        derr = float((d - r64.dirs).abs().max())
        say(f"## {name}")
        say(f"outputs: max |kernel - composite| on a direction {derr:.3e}; colours equal: {torch.equal(rgb, rgb64)}; masks equal: "
            f"{torch.equal(mask, mask64)}; origins equal: {torch.equal(o, r64.origins)}")
        assert derr <= 64 * 2.0 ** -24 and torch.equal(rgb, rgb64) and torch.equal(mask, mask64)
        t = {k: [] for k in ("kernel", "composite fp64", "composite fp32", "stores only")}
        for _ in range(samples):
            t["composite fp64"].append(_window(comp64, calls))
            t["composite fp32"].append(_window(comp32, calls))
            t["kernel"].append(_window(kernel, calls))
            t["composite fp64"].append(_window(comp64, calls))
            t["composite fp32"].append(_window(comp32, calls))
            t["stores only"].append(_window(stores, calls))
        for k, v in t.items():
            say(f"{k:16s} us/call  {_fmt(v)}   ({len(v)} windows of {calls} calls)")
        km = statistics.median(t["kernel"])
        for leg in ("composite fp64", "composite fp32"):
            c = t[leg]
            verdict = "below" if km < min(c) else "NOT below"
            say(f"kernel median {km:.1f} us is {verdict} the {leg} band {min(c):.1f} .. {max(c):.1f} us "
                f"(ratio of medians {statistics.median(c) / km:.2f}x)")
        sm = statistics.median(t["stores only"])
        say(f"stores only: {37 * n / 1e6:.2f} MB in {sm:.1f} us = {37 * n / sm / 1e6:.3f} TB/s; the kernel takes {km / sm:.2f}x that")
        say("")


def residency(dev, size, say):
    from PIL import Image
    import json
    from shacira_amd.wisp.datasets import NeRFSyntheticDataset
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "train"))
        frames = []
        for i in range(4):
            Image.fromarray(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "RGBA").save(
                os.path.join(root, "train", f"r_{i}.png"), compress_level=1)
            frames.append(dict(file_path=f"./train/r_{i}", transform_matrix=np.eye(4).tolist()))
        with open(os.path.join(root, "transforms_train.json"), "w") as fh:
            json.dump(dict(camera_angle_x=0.69, frames=frames), fh)
        ds = NeRFSyntheticDataset(root, device=dev)
    ours, theirs = ds.resident_bytes(), ds.reference_resident_bytes()
    say(f"## residency, {len(ds)} views of {size} x {size} RGBA (the dataset's counters)")
    say(f"resident_bytes {ours}   reference_resident_bytes {theirs}   ratio {theirs / ours:.4f}x "
        f"(per pixel 37 / 4 = 9.25; the records add {ds.records.numel() * 4} bytes)")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    time_shapes(dev, args.views, args.size, args.samples, args.calls, say)
    residency(dev, args.size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
