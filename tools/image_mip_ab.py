"""Mip levels: the block-sum kernel of image_mip.hip (``hip_ops.image_mip``) against the same sums as torch operators on the same
GPU and against the stream rate of probe.hip, and the ray kernel on a level's uint16 sums against the ray kernel on uint8 images.
Device events around batches of back-to-back calls.

    python tools/image_mip_ab.py [--views 100] [--size 800] [--samples 9] [--calls 20] [--ray-calls 200] [--out FILE]

(a) ``image_mip`` on ``--views`` RGBA images of ``--size`` squared with random bytes, at mip 1, 2 and 4. Legs, after a warm-up and
    a comparison of the outputs: the kernel (the call a user makes, its output allocation included); the torch chain
    ``view -> int32 -> sum`` (``wisp.ops.raygen.image_mip_torch``), timed before and after the kernel in every round so that its
    own min .. max band is known; and ``shacira_stream_probe`` reading the same number of bytes. The kernel's bytes (source read
    once, sums written once) over its median time are reported as a fraction of the probe's read rate; the probe's copy rate
    (read + write of the same buffer) is printed once beside it.
(b) ``hip_ops.raygen`` on the sums of a level (``--size >> 2`` squared, mip 2) against the same call on uint8 images of that
    size: batches of 4 096 and 65 536 random (view, pixel) pairs and one whole view. Every round times the uint8 call, the sums
    call and the uint8 call again: the uint8 call's band is the yardstick.
(c) The resident bytes of a NeRFSyntheticDataset at mip 2 against the reference's layout, from the dataset's counters (four views
    written to a temporary directory)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import _lib, hip_ops  # noqa: E402
from shacira_amd.wisp.core import Camera  # noqa: E402
from shacira_amd.wisp.ops.raygen import camera_records, image_mip_torch  # noqa: E402


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


def time_image_mip(dev, views, size, samples, calls, say):
    images = torch.randint(0, 256, (views, size, size, 4), dtype=torch.uint8, device=dev)
    nbytes = images.numel()
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sink = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    probe = lambda: _lib.check(_lib.lib().shacira_stream_probe(0, images.data_ptr(), sink.data_ptr(), nbytes, strm), "probe")
    copy = lambda: _lib.check(_lib.lib().shacira_stream_probe(2, images.data_ptr(), sink.data_ptr(), nbytes, strm), "probe")
    say(f"# (a) image_mip: {views} views of {size} x {size} RGBA, {nbytes / 1e6:.1f} MB of source bytes")
    for _ in range(3):
        copy()
    cm = statistics.median(_window(copy, calls) for _ in range(samples))
    say(f"probe copy of {nbytes / 1e6:.1f} MB (read + write, {2 * nbytes / 1e6:.1f} MB moved): median {cm:.1f} us = "
        f"{2 * nbytes / cm / 1e6:.3f} TB/s")
    for mip in (1, 2, 4):
        kernel = lambda: hip_ops.image_mip(images, mip)
        chain = lambda: image_mip_torch(images, mip)
        for fn in (kernel, chain, probe):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        same = bool((kernel().cpu().to(torch.int32) == chain().cpu()).all())
        say(f"## mip {mip}")
        say(f"outputs: kernel sums equal the torch chain's: {same}")
        assert same
        t = {k: [] for k in ("kernel", "torch chain", "probe read")}
        for _ in range(samples):
            t["torch chain"].append(_window(chain, calls))
            t["kernel"].append(_window(kernel, calls))
            t["torch chain"].append(_window(chain, calls))
            t["probe read"].append(_window(probe, calls))
        for k, v in t.items():
            say(f"{k:12s} us/call  {_fmt(v)}   ({len(v)} windows of {calls} calls)")
        km, pm = statistics.median(t["kernel"]), statistics.median(t["probe read"])
        verdict = "below" if km < min(t["torch chain"]) else "NOT below"
        say(f"kernel median {km:.1f} us is {verdict} the torch chain's minimum {min(t['torch chain']):.1f} us "
            f"(ratio of medians {statistics.median(t['torch chain']) / km:.2f}x)")
        moved = nbytes + nbytes * 2 // 4 ** mip
        say(f"bytes moved {moved / 1e6:.1f} MB (read {nbytes / 1e6:.1f} + written {(moved - nbytes) / 1e6:.1f}): "
            f"{moved / km / 1e6:.3f} TB/s; probe reads {nbytes / 1e6:.1f} MB at {nbytes / pm / 1e6:.3f} TB/s; "
            f"fraction of the stream rate {(moved / km) / (nbytes / pm):.3f}")
        say("")
    del images, sink


def time_raygen(dev, views, size, samples, calls, say):
    mip = 2
    side = size >> mip
    gen = torch.Generator().manual_seed(0)
    eye = torch.randn(views, 3, generator=gen, dtype=torch.float64)
    eye = 3.0 * eye / eye.norm(dim=1, keepdim=True)
    cams = Camera.from_args(eye=eye, at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0], fov=0.69, width=side, height=side, near=0.0,
                            far=6.0).to(dev)
    records = camera_records(cams)
    full = torch.randint(0, 256, (views, size, size, 4), dtype=torch.uint8, device=dev)
    sums = hip_ops.image_mip(full, mip)
    del full
    bytes8 = torch.randint(0, 256, (views, side, side, 4), dtype=torch.uint8, device=dev)
    hw = side * side
    say(f"# (b) raygen: {views} views of {side} x {side} (mip {mip} of {size} x {size}); sums {sums.numel() * 2 / 1e6:.1f} MB, "
        f"uint8 images of the same size {bytes8.numel() / 1e6:.1f} MB")
    dgen = torch.Generator(device=dev).manual_seed(1)
    shapes = [("sample 4 096", 4096, None), ("sample 65 536", 65536, None), (f"whole view ({hw} rays)", hw, views // 3)]
    for name, n, whole in shapes:
        if whole is None:
            vi = torch.randint(0, views, (n,), device=dev, dtype=torch.int32, generator=dgen)
            pi = torch.randint(0, hw, (n,), device=dev, dtype=torch.int32, generator=dgen)
            on_bytes = lambda: hip_ops.raygen(records, side, side, vi, pi, None, bytes8, "white")
            on_sums = lambda: hip_ops.raygen(records, side, side, vi, pi, None, sums, "white", mip=mip)
        else:
            rec1, b1, s1 = records[whole:whole + 1], bytes8[whole:whole + 1], sums[whole:whole + 1]
            on_bytes = lambda: hip_ops.raygen(rec1, side, side, None, None, None, b1, "white", num_rays=hw)
            on_sums = lambda: hip_ops.raygen(rec1, side, side, None, None, None, s1, "white", num_rays=hw, mip=mip)
        for fn in (on_bytes, on_sums):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        (o8, d8, _, _), (o16, d16, rgb, _) = on_bytes(), on_sums()
        same = torch.equal(o8, o16) and torch.equal(d8, d16)
        say(f"## {name}")
        say(f"outputs: origins and directions of the two calls equal: {same}; colours finite: {bool(torch.isfinite(rgb).all())}")
        assert same
        t = {"uint8": [], "sums": []}
        for _ in range(samples):
            t["uint8"].append(_window(on_bytes, calls))
            t["sums"].append(_window(on_sums, calls))
            t["uint8"].append(_window(on_bytes, calls))
        for k, v in t.items():
            say(f"{k:6s} us/call  {_fmt(v)}   ({len(v)} windows of {calls} calls)")
        sm, lo, hi = statistics.median(t["sums"]), min(t["uint8"]), max(t["uint8"])
        say(f"sums median {sm:.1f} us is {'inside' if lo <= sm <= hi else 'below' if sm < lo else 'ABOVE'} the uint8 call's band "
            f"{lo:.1f} .. {hi:.1f} us")
        say("")


def residency(dev, size, say):
    from PIL import Image
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
        ds = NeRFSyntheticDataset(root, device=dev, mip=2)
        ds0 = NeRFSyntheticDataset(root, device=dev)
    ours, theirs = ds.resident_bytes(), ds.reference_resident_bytes()
    say(f"# (c) residency, {len(ds)} views of {size} x {size} RGBA at mip 2 = {ds.img_shape[0]} x {ds.img_shape[1]} (the dataset's "
        f"counters)")
    say(f"resident_bytes {ours}   reference_resident_bytes {theirs}   ratio {theirs / ours:.4f}x (per pixel of the level 37 / 8); "
        f"the same views at mip 0: resident_bytes {ds0.resident_bytes()}, {ds0.resident_bytes() / ours:.3f}x the level's")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ray-calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    time_image_mip(dev, args.views, args.size, args.samples, args.calls, say)
    time_raygen(dev, args.views, args.size, args.samples, args.ray_calls, say)
    residency(dev, args.size, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
