"""Positional-encoding rows: the fused kernel of posenc.hip (``PositionalEmbedder(fused=True).rows``) against the torch composite
``torch.cat([prefix, PositionalEmbedder(coords)], -1)`` on the same GPU, device events around batches of back-to-back calls.

    python tools/posenc_ab.py [--samples 9] [--calls 200] [--noise] [--out FILE]

Shapes: the config-B image row (N = 393 216, d = 2, P = 32, F = 10 and F = 4, no raw position) and the NeRF view row (N = 2^19,
d = 3, P = 16, F = 4, with the position). Per shape, after a warm-up of every leg: ``--samples`` rounds, each round one window of
the fused call and TWO of the composite (before and after it), so the composite's own min .. max band is known; a window is
``--calls`` calls between two events, the figure its time over the calls. Also timed, the same way: a device copy of the row
(``out.copy_(src)``, bytes read + written over the time = the measured copy rate) -- the fused call writes the row once and reads
the prefix and the coordinates, so ``bytes moved / copy rate`` is the time a store-bound kernel would take -- and the forward +
backward of both paths (gradients to prefix and coordinates). Outputs of the two paths are compared before anything is timed.

``--noise``: the yardstick of tests/test_gpu_neural_image.py -- on the NeuralImage of that test built with the composite row, the
fused-MLP decoder against the plain nn.Linear chain on identical inputs (worst relative difference over rgb and the gradients),
and next to it the fused row against the composite row through the same fused decoder."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd.wisp.models.embedders import PositionalEmbedder  # noqa: E402

SHAPES = [   # name, N, d, P, F, include_input
    ("image F=10", 393_216, 2, 32, 10, False),
    ("image F=4", 393_216, 2, 32, 4, False),
    ("nerf view F=4", 1 << 19, 3, 16, 4, True),
]


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


def time_shapes(dev, samples, calls, say):
    for name, N, d, P, F, inc in SHAPES:
        torch.manual_seed(0)
        fused = PositionalEmbedder(F, F - 1, include_input=inc, input_dim=d, fused=True).to(dev)
        plain = PositionalEmbedder(F, F - 1, include_input=inc, input_dim=d, fused=False).to(dev)
        coords = torch.rand(N, d, device=dev) * 2 - 1
        prefix = torch.randn(N, P, device=dev)
        width = P + fused.out_dim
        cg, pg = coords.clone().requires_grad_(True), prefix.clone().requires_grad_(True)
        go = torch.randn(N, width, device=dev)
        src, dst = torch.randn(N, width, device=dev), torch.empty(N, width, device=dev)

        def f_fwd():
            with torch.no_grad():
                return fused.rows(prefix, coords)

        def c_fwd():
            with torch.no_grad():
                return torch.cat([prefix, plain(coords)], dim=-1)

        def f_step():
            return torch.autograd.grad(fused.rows(pg, cg), (pg, cg), go)

        def c_step():
            return torch.autograd.grad(torch.cat([pg, plain(cg)], dim=-1), (pg, cg), go)

        def copy():
            dst.copy_(src)

        for fn in (f_fwd, c_fwd, f_step, c_step, copy):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        a, b = f_fwd(), c_fwd()
        enc = float((a[:, P + (d if inc else 0):] - b[:, P + (d if inc else 0):]).abs().max())
        same_head = torch.equal(a[:, :P + (d if inc else 0)], b[:, :P + (d if inc else 0)])
        (gpa, gca), (gpb, gcb) = f_step(), c_step()
        gdiff = float((gca - gcb).abs().max() / gcb.abs().max())
        say(f"## {name}: N = {N}, d = {d}, P = {P}, F = {F}, include_input = {inc}: row of {width} floats")
        say(f"outputs: prefix / coordinate columns equal: {same_head}; sin / cos max |fused - composite| = {enc:.3e}; "
            f"coordinate gradient max |difference| / max |g| = {gdiff:.3e}; prefix gradients equal: {torch.equal(gpa, gpb)}")
        assert same_head and enc <= 1e-6 and gdiff <= 1e-5
        t = {k: [] for k in ("fused fwd", "composite fwd", "fused fwd+bwd", "composite fwd+bwd", "row copy")}
        for _ in range(samples):
            t["composite fwd"].append(_window(c_fwd, calls))
            t["fused fwd"].append(_window(f_fwd, calls))
            t["composite fwd"].append(_window(c_fwd, calls))
            t["composite fwd+bwd"].append(_window(c_step, calls))
            t["fused fwd+bwd"].append(_window(f_step, calls))
            t["composite fwd+bwd"].append(_window(c_step, calls))
            t["row copy"].append(_window(copy, calls))
        for k, v in t.items():
            say(f"{k:18s} us/call  {_fmt(v)}   ({len(v)} windows of {calls} calls)")
        for leg in ("fwd", "fwd+bwd"):
            f, c = t[f"fused {leg}"], t[f"composite {leg}"]
            verdict = "below" if statistics.median(f) < min(c) else "NOT below"
            say(f"{leg}: fused median {statistics.median(f):.1f} us is {verdict} the composite's band "
                f"{min(c):.1f} .. {max(c):.1f} us (ratio of medians {statistics.median(c) / statistics.median(f):.2f}x)")
        copy_rate = 2 * N * width * 4 / (statistics.median(t["row copy"]) * 1e-6)           # bytes / s, read + write
        moved = N * (width + P + d) * 4
        floor = moved / copy_rate * 1e6
        fm = statistics.median(t["fused fwd"])
        say(f"measured copy rate {copy_rate / 1e12:.2f} TB/s; the fused forward moves {moved / 1e6:.1f} MB = {floor:.1f} us at "
            f"that rate; it takes {fm:.1f} us = {fm / floor:.2f}x the store-bound time "
            f"({'stores' if fm < 1.5 * floor else 'VALU (sincosf)'} bound it)")
        say("")


def decoder_noise(dev, say):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_neural_image as T
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(-1, 1, (T.PIXELS, 2)).astype(np.float32)).to(dev)
    target = torch.from_numpy(rng.uniform(0, 1, (T.PIXELS, 3)).astype(np.float32)).to(dev)
    fused, _, _ = T.build(dev, True)
    plain, _, _ = T.build(dev, False, fused.state_dict())
    linear, _, _ = T.build(dev, False, fused.state_dict())
    linear.decoder_color._fused_dims = lambda x: None          # the nn.Linear chain on the same rows
    want = T.evaluate(plain, coords, target)
    noise = T.relative_differences(T.evaluate(linear, coords, target), want)
    row = T.relative_differences(T.evaluate(fused, coords, target), want)
    say("## NeuralImage (16 lods x 2, 4 099 pixels, 48-wide row): relative differences max |a - b| / max |b|")
    for k in sorted(want):
        say(f"{k:40s} Linear chain vs fused MLP (identical composite rows) {noise[k]:.3e}    fused row vs composite row "
            f"(same fused MLP) {row[k]:.3e}")
    say(f"worst: decoder noise {max(noise.values()):.6e}   fused row {max(row.values()):.6e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.noise:
        decoder_noise(dev, say)
    else:
        time_shapes(dev, args.samples, args.calls, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
