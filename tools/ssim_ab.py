"""SSIM: the fused kernels of ssim.hip against the same definition in torch ops (metrics.ssim_torch) on the same GPU, HIP-event
times after one warm-up, three interleaved rounds.

    python tools/ssim_ab.py [--reps 3] [--calls 10] [--shapes 800x800,4096x4096]

Legs, per shape [H, W, 3] fp32 on the device: the value alone (``hip_ops.ssim_forward`` / ``ssim_torch``) and the value with its
gradient (``metrics.ssim_loss`` + backward / ``1 - ssim_torch`` + backward). The outputs of the two paths are compared before
anything is timed. A window is ``--calls`` calls between two events; the figure is the window over the calls.

What the figures can say: the forward's algorithmic traffic is 2 * H * W * C * 4 bytes (15 MB at 800 x 800 x 3), so the kernel leg
at that size is bound by its two launches; the torch leg moves on the order of twenty image-sized temporaries."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import hip_ops  # noqa: E402
from shacira_amd.wisp.ops.image import metrics  # noqa: E402


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shapes", default="800x800,4096x4096")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for shape in args.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        gt = torch.rand(H, W, 3, device=dev)
        pred = (gt + 0.1 * (torch.rand(H, W, 3, device=dev) - 0.5)).clamp(0, 1)
        pk, pt = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)

        def kernel_fwd():
            return hip_ops.ssim_forward(pred, gt)[0]

        def torch_fwd():
            with torch.no_grad():
                return metrics.ssim_torch(pred, gt)

        def kernel_step():
            pk.grad = None
            metrics.ssim_loss(pk, gt).backward()

        def torch_step():
            pt.grad = None
            (1.0 - metrics.ssim_torch(pt, gt)).backward()

        legs = {"kernel fwd": kernel_fwd, "torch fwd": torch_fwd, "kernel fwd+bwd": kernel_step, "torch fwd+bwd": torch_step}
        for fn in legs.values():      # warm-up, and the outputs to compare
            fn()
        torch.cuda.synchronize()
        vk, vt = kernel_fwd().item(), torch_fwd().item()
        gdiff = float((pk.grad - pt.grad).abs().max() / pt.grad.abs().max())
        print(f"{H}x{W}x3: ssim kernel {vk:.9f} torch {vt:.9f} |difference| {abs(vk - vt):.2e}; gradient max|difference| / max|g| "
              f"{gdiff:.2e}")
        assert abs(vk - vt) <= 1e-5 and gdiff <= 1e-3
        times = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                times[k].append(_window(fn, args.calls))
        for k, v in times.items():
            print(f"{H}x{W}x3 {k:15s} runs (ms/call) {' '.join(f'{t:9.4f}' for t in v)}   median {statistics.median(v):9.4f}")
        for a, b in (("kernel fwd", "torch fwd"), ("kernel fwd+bwd", "torch fwd+bwd")):
            print(f"{H}x{W}x3 {b} / {a} time ratio {statistics.median(times[b]) / statistics.median(times[a]):.2f}x")
        peak = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        print(f"{H}x{W}x3 peak allocated {peak:.0f} MiB (both paths in one process; image {H * W * 12 / 2 ** 20:.0f} MiB)")


if __name__ == "__main__":
    main()
