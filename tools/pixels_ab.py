"""Pixel batches and the pixel loss: the fused kernels of pixels.hip (``hip_ops.pixel_batch``, ``hip_ops.pixel_loss``) against the
torch-op chains they replace, on the same GPU, device events around batches of back-to-back calls.

    python tools/pixels_ab.py [--samples 7] [--calls 100] [--skip-pearl | --skip-kodak] [--out FILE]

Two shapes. "kodak": a 512 x 768 image, one batch of all 393 216 pixels in a stored permutation (sample_mode 'full'). "pearl": a
20000 x 23466 image made on the device, 2^18 uniformly drawn int64 indices (sample_mode 'wreplace'). Legs per shape, each warmed up
and its outputs compared with the kernel's before anything is timed:
  batch   kernel        coords and colours from indices and the uint8 image
          gather fp32   the reference's layout held on the device: materialised fp32 coords [HW, 2] and colours [HW, 3], indexed
                        (kodak only for the coordinates; at pearl the colours alone are 5.6 GB and the coordinates come from the
                        index arithmetic in torch ops, as transform_coords does it -- with the exact integer rule)
  loss    kernel        pixel_loss forward, the scaled backward, and nothing else: the statistics are its second output
          chain         ImageFitter.step / read_last of the parent commit: ((pred - rgb) ** 2).sum(), its backward, and the
                        clamped-PSNR statistics (clamp, * 255, to uint8, float, difference, square, sum, stack, double); the
                        quantised target is cached at kodak (the target is static) and formed per call at pearl (it is not)
  loss fwd      the forward halves alone under no autograd, as validation calls them
  C entry points   shacira_pixel_loss_forward + _backward on preallocated buffers: the three launches without the tensor wrappers
                and autograd, i.e. what the device spends (no chain stands beside it)
Per round one window of the kernel between two windows of the chain, so the chain's own min .. max band is known; a window is
``--calls`` calls between two events, the figure its time over the calls. Resident bytes are the datasets' own counters."""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import _lib, hip_ops  # noqa: E402
from shacira_amd.wisp.datasets import MultiImageDataset  # noqa: E402


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


def _compare(say, name, kernel, chain, samples, calls):
    for fn in (kernel, chain):
        for _ in range(3):
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


def _true_divide_255(image, chunk=1 << 26):
    """fp32 colours [HW, 3] by a correctly rounded division (torch's device division by a host scalar multiplies by a reciprocal)."""
    flat = image.reshape(-1)
    out = torch.empty(flat.shape, dtype=torch.float32, device=image.device)
    d = torch.tensor(255.0, device=image.device)
    for s in range(0, flat.numel(), chunk):
        out[s:s + chunk] = flat[s:s + chunk].float() / d
    return out.reshape(-1, 3)


def shape(say, dev, name, H, W, n, mode, samples, calls):
    g = torch.Generator(device=dev).manual_seed(0)
    image = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    with tempfile.TemporaryDirectory() as empty:
        ds = MultiImageDataset(empty, 0, "train", num_samples=n, sample_mode=mode, device=dev)
        ds.set_image(image)
    say(f"## {name}: {H} x {W}, n = {n}, sample_mode '{mode}'")
    say(f"resident_bytes {ds.resident_bytes()}   reference_resident_bytes {ds.reference_resident_bytes()}   "
        f"ratio {ds.reference_resident_bytes() / ds.resident_bytes():.2f}x")
    if mode == "full":
        idx = ds.shuffle_idx
    else:
        idx = torch.randint(0, H * W, (n,), device=dev, generator=g)                      # int64, as torch.randint gives it
    rgb_all = _true_divide_255(image)
    h, w = torch.tensor(float(H), device=dev), torch.tensor(float(W), device=dev)
    if mode == "full":
        coords_all, _ = hip_ops.pixel_batch(image, want_rgb=False)
        idx64 = idx.long()                                   # the reference's shuffle_idx is int64
        batch_chain = lambda: (coords_all[idx64], rgb_all[idx64])
    else:
        def batch_chain():
            y = torch.div(idx, W, rounding_mode="floor")
            x = idx - y * W
            return torch.stack([(y.float() / h - 0.5) * 2.0, (x.float() / w - 0.5) * 2.0], dim=-1), rgb_all[idx]
    batch_kernel = lambda: hip_ops.pixel_batch(image, idx)
    (kc, kr), (cc, cr) = batch_kernel(), batch_chain()
    say(f"batch outputs: coords equal {torch.equal(kc, cc)}, colours equal {torch.equal(kr, cr)}")
    assert torch.equal(kc, cc) and torch.equal(kr, cr)
    _compare(say, "batch", batch_kernel, batch_chain, samples, calls)

    pred = (torch.rand((n, 3), device=dev, generator=g) * 1.2 - 0.1).requires_grad_(True)
    rgb = kr
    scale = 1.0 / (3 * n)
    q = lambda t: (torch.clamp(t, 0, 1) * 255).to(torch.uint8).float()
    rgb_q = q(rgb) if mode == "full" else None
    out = {}

    def loss_kernel():
        pred.grad = None
        sq, stats = hip_ops.pixel_loss(pred, image, idx)
        (sq * scale).backward()
        out["kernel"] = (stats, pred.grad)

    def loss_chain():
        pred.grad = None
        sq = ((pred - rgb) ** 2).sum()
        (sq * scale).backward()
        with torch.no_grad():
            stats = torch.stack([sq.detach(), ((q(pred) - (rgb_q if rgb_q is not None else q(rgb))) ** 2).sum()]).double()
        out["chain"] = (stats, pred.grad)

    loss_kernel()
    loss_chain()
    (ks, kg), (cs, cg) = out["kernel"], out["chain"]
    ks, cs = ks.tolist(), cs.tolist()
    say(f"loss outputs: gradients equal {torch.equal(kg, cg)}; squared error kernel {ks[0]!r} (fp64 sum) chain {cs[0]!r} (fp32 sum); "
        f"level sum kernel {ks[1]!r} (integer) chain {cs[1]!r} (fp32 sum)")
    assert torch.equal(kg, cg) and abs(ks[0] - cs[0]) <= 1e-4 * ks[0] and abs(ks[1] - cs[1]) <= 1e-4 * ks[1]
    _compare(say, "loss fwd+bwd", loss_kernel, loss_chain, samples, calls)

    # the forward alone, as validation calls it (no autograd): statistics from one call against the chain's forward half
    pd = pred.detach()

    def fwd_kernel():
        return hip_ops.pixel_loss(pd, image, idx)[1]

    def fwd_chain():
        sq = ((pd - rgb) ** 2).sum()
        return torch.stack([sq, ((q(pd) - (rgb_q if rgb_q is not None else q(rgb))) ** 2).sum()]).double()

    _compare(say, "loss fwd    ", fwd_kernel, fwd_chain, samples, calls)

    # the three launches themselves through the C entry points on preallocated buffers: what the device spends, without the
    # tensor wrappers and autograd around them
    L = _lib.lib()
    nbytes = int(L.shacira_pixel_loss_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    gbuf = torch.empty((n, 3), dtype=torch.float32, device=dev)
    gdev = torch.full((1,), scale, dtype=torch.float32, device=dev)
    width = 32 if idx.dtype == torch.int32 else 64
    s = torch.cuda.current_stream().cuda_stream

    def raw():
        rc = L.shacira_pixel_loss_forward(pd.data_ptr(), 3, image.data_ptr(), H, W, idx.data_ptr(), width, 0, n, None,
                                          stats.data_ptr(), ws.data_ptr(), nbytes, s)
        rc |= L.shacira_pixel_loss_backward(pd.data_ptr(), 3, image.data_ptr(), H, W, idx.data_ptr(), width, 0, n, gdev.data_ptr(),
                                            gbuf.data_ptr(), s)
        assert rc == 0

    for _ in range(3):
        raw()
    torch.cuda.synchronize()
    assert torch.equal(gbuf, kg) and stats.tolist() == ks
    t = [_window(raw, calls) for _ in range(samples)]
    say(f"loss fwd+bwd, C entry points alone (three launches, no wrappers)  us/call  {_fmt(t)}   ({len(t)} windows of {calls} calls)")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--skip-pearl", action="store_true")
    ap.add_argument("--skip-kodak", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(s + "\n")

    if not args.skip_kodak:
        shape(say, dev, "kodak", 512, 768, 512 * 768, "full", args.samples, args.calls)
    if not args.skip_pearl:
        shape(say, dev, "pearl", 20000, 23466, 1 << 18, "wreplace", args.samples, args.calls)


if __name__ == "__main__":
    main()
