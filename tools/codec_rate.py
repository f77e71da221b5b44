"""Entropy codec, end to end on a device-resident table: `codec.compress_latents` / `codec.decompress_latents` with the
device rANS path (coder="rans": HIP kernels, only bytes cross the bus) against the host range coder of the same checkout in
the same process (coder="range": the table goes to the host, one CPU thread codes it, the result is uploaded).

    python tools/codec_rate.py [--rows 7879908] [--ld 1] [--std 2.0] [--reps 5] [--steps 4096]

The table is nerf_lego.yaml's size (7 879 908 latents, tests/test_codec.py) with rounded-Gaussian values, on the GPU. Both
legs start from that tensor and end with the container bytes on the host (compress) or the decoded fp32 table on the device
(decompress), copies included. Each call is timed with a host clock around work that ends in a device synchronise (a call
holds host loops and blocking copies, so events alone would miss part of it); one warm-up per leg, `--reps` rounds with the
legs alternating; medians and the runs are printed. Outputs are checked before anything is timed: both containers restore
round(table) exactly, and the device container equals the one the host rANS coder writes."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import codec  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=7_879_908)
    ap.add_argument("--ld", type=int, default=1)
    ap.add_argument("--std", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=codec.RANS_STEPS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "codec_rate.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    table = torch.randn((args.rows, args.ld), device=dev) * args.std
    want = torch.round(table)
    n = args.rows * args.ld

    legs = {
        "rans  (device) compress": lambda: codec.compress_latents(table, coder="rans", steps=args.steps),
        "range (host)   compress": lambda: codec.compress_latents(table, coder="range"),
    }
    blobs = {k: fn() for k, fn in legs.items()}                      # warm-up, and the outputs to check
    b_rans, b_range = blobs["rans  (device) compress"], blobs["range (host)   compress"]
    legs["rans  (device) decompress"] = lambda: codec.decompress_latents(b_rans, dev)
    legs["range (host)   decompress"] = lambda: codec.decompress_latents(b_range, dev)
    assert torch.equal(legs["rans  (device) decompress"](), want)
    assert torch.equal(legs["range (host)   decompress"](), want)
    assert b_rans == codec.compress_latents(table.cpu(), coder="rans", steps=args.steps), "device and host rANS bytes differ"
    lo, counts = codec.symbol_counts(table)
    entropy = sum(codec.entropy_bits(counts[c]) for c in range(args.ld))
    print(f"table [{args.rows}, {args.ld}] fp32 on {torch.cuda.get_device_name(dev)}, rounded N(0, {args.std}^2): {n} symbols, "
          f"empirical entropy {entropy / 8:.0f} bytes ({entropy / n:.4f} bit/symbol)")
    for name, blob in (("rans", b_rans), ("range", b_range)):
        print(f"{name:5s} container {len(blob)} bytes, payload {codec.payload_bits(blob) // 8} bytes "
              f"({codec.payload_bits(blob) / n:.4f} bit/symbol, {100 * (codec.payload_bits(blob) / entropy - 1):+.3f} % of entropy)")

    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(_timed(fn)[0])
    for k, v in times.items():
        print(f"{k:26s} runs (ms) {' '.join(f'{t:8.2f}' for t in v)}   median {statistics.median(v):8.2f}")
    for what in ("compress", "decompress"):
        host = statistics.median(times[f"range (host)   {what}"])
        devt = statistics.median(times[f"rans  (device) {what}"])
        print(f"{what}: host range / device rans time ratio {host / devt:.2f}x")

    # what of a compress call is the coder itself: the encode wrapper alone (model already built, table already counted)
    from shacira_amd import hip_ops
    T, ld, steps, chans = codec._parse_rans(b_rans)
    nbins = [ch["nbins"] for ch in chans]
    cdf = codec.cdf_table([ch["freq"] for ch in chans])
    los = [ch["lo"] for ch in chans]
    kernels = lambda: hip_ops.latent_rans_encode(table, los, nbins, cdf, steps)   # noqa: E731
    kernels()
    runs = [_timed(kernels)[0] for _ in range(args.reps)]
    print(f"encode + pack kernels, read-backs included: runs (ms) {' '.join(f'{t:8.2f}' for t in runs)}   "
          f"median {statistics.median(runs):8.2f}")


if __name__ == "__main__":
    main()
