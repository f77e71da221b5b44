"""View shading: the four kernels of shade.hip (``hip_ops.shade_view``, ``shadow_rays``, ``shadow_apply``, ``sdf_slice_colors``)
against a torch chain on the same GPU that restates the same lines of the reference, and -- for the matcap lookup and the shadow
blur -- against the reference's own host route: copy out, scipy, copy back. Device events around batches of back-to-back calls.

    python tools/shade_ab.py [--samples 9] [--calls 200] [--kernel-calls 4000] [--host-calls 3] [--out FILE]

Two views: the reference's default 1024 x 720 and 256 x 256. Per view and kernel, after a warm-up of every leg and a comparison of
the outputs: ``--samples`` rounds, each round one window of the kernel between TWO windows of the torch chain, so the chain's own
min .. max band is known; a window is ``--calls`` calls (``--kernel-calls`` for the kernel legs, which are tens of microseconds
each) between two events, the figure its time over the calls. Two kernel legs work on fresh copies of the buffers they update in
place; the copies alone are timed as a leg of their own ("copies only"). The host routes are timed by the wall clock around
``--host-calls`` calls with a synchronisation at both ends. Records, not gates."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import hip_ops  # noqa: E402
from shacira_amd.wisp.offline_renderer import sdf_slice_colors_torch  # noqa: E402
from shacira_amd.wisp.ops.geometric import spherical_envmap_torch  # noqa: E402
from shacira_amd.wisp.ops.shaders import default_matcap  # noqa: E402


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def _wall(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def _fmt(v):
    return f"min {min(v):9.1f}  median {statistics.median(v):9.1f}  max {max(v):9.1f}"


def _sample_torch(tex, uv):
    """The bilinear lookup of ``sample_matcap_torch`` in fp32 on the device."""
    mh, mw = tex.shape[:2]
    t = tex[..., :3].float()
    x, y = uv[:, 0] * (mw - 1), uv[:, 1] * (mh - 1)
    x0 = torch.clamp(torch.floor(x).long(), max=mw - 2)
    y0 = torch.clamp(torch.floor(y).long(), max=mh - 2)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    return ((1 - fx) * (1 - fy) * t[y0, x0] + fx * (1 - fy) * t[y0, x0 + 1] + (1 - fx) * fy * t[y0 + 1, x0]
            + fx * fy * t[y0 + 1, x0 + 1]) / 255.0


def legs(dev, H, W):
    """{name: (kernel, torch chain, host route or None, check, the kernel leg's copies alone or None)} on one view's buffers."""
    from scipy.interpolate import RegularGridInterpolator
    from scipy.ndimage import gaussian_filter
    n = H * W
    g = torch.Generator(device=dev).manual_seed(0)
    normal = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    origins = torch.randn(n, 3, device=dev, generator=g) * 0.5 + torch.tensor([0.0, 1.0, 3.0], device=dev)
    hit = torch.rand(n, device=dev, generator=g) < 0.6
    depth = torch.where(hit, torch.rand(n, device=dev, generator=g) * 5 + 1, torch.zeros(n, device=dev))
    xyz = torch.where(hit[:, None], origins + dirs * depth[:, None], torch.zeros(n, 3, device=dev))
    rgb = torch.rand(n, 3, device=dev, generator=g)
    occluded = torch.rand(n, device=dev, generator=g) < 0.3
    light_hit = torch.rand(n, device=dev, generator=g) < 0.8
    sdf = torch.rand(n, device=dev, generator=g) * 2.6 - 1.3
    tex = default_matcap(512).to(dev)
    tex_host = tex.cpu().numpy().transpose(1, 0, 2)
    interp = RegularGridInterpolator((np.linspace(0, 1, tex_host.shape[0]), np.linspace(0, 1, tex_host.shape[1])), tex_host)
    light = torch.tensor([[1.5, 4.5, 1.5]], device=dev)
    out = {}

    # matcap shading with the segmentation
    nk = normal.clone()

    def matcap_kernel():
        return hip_ops.shade_view("matcap", normal=nk, dirs=dirs, hit=hit, matcap=tex)[0]

    def matcap_torch():
        c = _sample_torch(tex, spherical_envmap_torch(dirs, normal))
        nn = normal.clone()
        nn[~hit] = 1.0
        c[~hit] = 1.0
        return c

    def matcap_host():
        uv = spherical_envmap_torch(dirs, normal).cpu().numpy()
        c = torch.FloatTensor(interp(uv)[..., :3].reshape(n, 3)).to(dev) / 255.0
        c[~hit] = 1.0
        return c
    out["matcap + segmentation"] = (matcap_kernel, matcap_torch, matcap_host, 1e-4, None)

    # shadow rays
    def rays_kernel():
        return hip_ops.shadow_rays(origins, dirs, depth.clone(), xyz.clone(), normal.clone(), hit.clone())[1]

    def rays_torch():
        d_, x_, n_, h_ = depth.clone(), xyz.clone(), normal.clone(), hit.clone()
        plane_t = (origins[:, 1] + 2.0) / (-dirs[:, 1])
        ph = (plane_t > 0) & (plane_t < 500) & (plane_t < d_)
        h_ = h_ & ~ph
        d_ = torch.where(ph, plane_t, d_)
        x_ = torch.where(ph[:, None], origins + dirs * plane_t[:, None], x_)
        n_ = torch.where(ph[:, None], torch.tensor([0.0, 1.0, 0.0], device=dev), n_)
        so = x_ + 0.01 * n_
        sd = torch.nn.functional.normalize(torch.zeros_like(x_).normal_(0.0, 0.01) + light - so, dim=1)
        _ = (sd * n_).sum(-1) > 0.0
        return sd
    out["shadow rays"] = (rays_kernel, rays_torch, None, None,           # different jitter: no comparison
                          lambda: (depth.clone(), xyz.clone(), normal.clone(), hit.clone()))

    # shadow apply
    def apply_kernel():
        c = rgb.clone()
        hip_ops.shadow_apply(H, W, occluded, light_hit, c)
        return c

    k = torch.arange(-8, 9, dtype=torch.float64)
    taps = torch.exp(-0.5 * k * k / 4.0)
    taps = (taps / taps.sum()).float().to(dev)

    def apply_torch():          # the blur as two convolutions over edges mirrored by flips (views of 8 pixels and more)
        s = occluded & light_hit
        x = torch.clamp((1.0 - s.float()) + 0.7, 0.0, 1.0).reshape(1, 1, H, W)
        x = torch.nn.functional.conv2d(torch.cat([x[:, :, :8].flip(2), x, x[:, :, -8:].flip(2)], 2), taps.view(1, 1, 17, 1))
        x = torch.nn.functional.conv2d(torch.cat([x[..., :8].flip(3), x, x[..., -8:].flip(3)], 3), taps.view(1, 1, 1, 17))
        return rgb * x.reshape(n, 1)

    def apply_host():
        s = occluded & light_hit
        m = torch.clamp((1.0 - s.float()) + 0.7, 0.0, 1.0).reshape(H, W).cpu().numpy()
        return rgb * torch.from_numpy(gaussian_filter(m, sigma=2)).reshape(n, 1).to(dev)
    out["shadow apply (blur)"] = (apply_kernel, apply_torch, apply_host, 1e-5, lambda: rgb.clone())

    # slice colours
    def slice_host():
        return torch.from_numpy(sdf_slice_colors_torch(sdf.cpu()).numpy()).to(dev)
    out["slice colours"] = (lambda: hip_ops.sdf_slice_colors(sdf), lambda: sdf_slice_colors_torch(sdf), slice_host, 1e-6, None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--kernel-calls", type=int, default=4000)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for W, H in ((1024, 720), (256, 256)):
        say(f"# view {W} x {H} ({W * H} pixels)")
        for name, (kernel, chain, host, tol, copies) in legs(dev, H, W).items():
            for fn in (kernel, chain) + ((host,) if host else ()):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            say(f"## {name}")
            if tol is not None:
                a, b = kernel(), chain()
                err = float((a - b).abs().max())
                say(f"outputs: max |kernel - torch chain| {err:.3e}")
                assert err <= tol, (name, err)
                if host:
                    say(f"outputs: max |kernel - host route| {float((a - host()).abs().max()):.3e}")
            t = {"kernel": [], "torch chain": []}
            for _ in range(args.samples):
                t["torch chain"].append(_window(chain, args.calls))
                t["kernel"].append(_window(kernel, args.kernel_calls))
                t["torch chain"].append(_window(chain, args.calls))
            if copies:
                t["copies only"] = [_window(copies, args.kernel_calls) for _ in range(3)]
            if host:
                t["host route"] = [_wall(host, args.host_calls) for _ in range(3)]
            for k, v in t.items():
                say(f"{k:12s} us/call  {_fmt(v)}   ({len(v)} windows)")
            km, c = statistics.median(t["kernel"]), t["torch chain"]
            verdict = "below" if km < min(c) else "NOT below"
            say(f"kernel median {km:.1f} us is {verdict} the torch chain's band {min(c):.1f} .. {max(c):.1f} us "
                f"(ratio of medians {statistics.median(c) / km:.2f}x)")
            if host:
                say(f"host route median {statistics.median(t['host route']):.1f} us: "
                    f"{statistics.median(t['host route']) / km:.1f}x the kernel")
            say("")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
