"""Mixed-precision optimizer steps: the loss-scaled fused kernels of adam.hip under ``torch.amp.GradScaler`` against what the same
scaler does without them, on the same GPU. Device events around windows of back-to-back calls; medians over the windows.

    python tools/optim_amp_ab.py [--samples 7] [--calls 100] [--out FILE]

Shapes: the S1 hash table ``[6 098 925, 2]`` fp32 and the config-B table ``[26 704, 2]``, each alone and with the NeRF decoder's
tensors (``[64, 32]``, ``[64]``, ``[3, 64]``, ``[3]``) in the same launch. Legs, each ``scaler.step(opt); scaler.update()``:

  (a) FusedAdam(capturable=True) -- the scaler hands scale and inf flag over on the device -- against FusedAdam() on the scaler's
      generic path: torch's foreach unscale pass, an ``.item()`` of the inf flag, then the step (what the parent commit did);
  (b) FusedRMSprop(capturable=True) against torch.optim.RMSprop(foreach=True) on the generic path;
  (c) no scaler: FusedRMSprop().step() against torch.optim.RMSprop(foreach=True).step().

Beside them: the scaler's own inf check (``torch._amp_foreach_non_finite_check_and_unscale_``, which legs (a) and (b) still run
once per step on the fused side), each kernel alone with scale and flag bound by hand, the dwords per element each kernel moves
and its rate against ``shacira_stream_probe``'s copy rate in the same run. The scaler runs at scale 1.0 so that a gradient
buffer stepped thousands of times keeps its values; the work per call does not depend on the scale. Records, not gates."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shacira_amd import _lib  # noqa: E402
from shacira_amd.optim import FusedAdam, FusedRMSprop  # noqa: E402

TABLES = {"S1 table [6098925, 2]": (6_098_925, 2), "config-B table [26704, 2]": (26_704, 2)}
DECODER = [(64, 32), (64,), (3, 64), (3,)]


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def _params(shapes, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.1) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=g)
    return ps


def _scaled_leg(make, shapes, dev):
    ps = _params(shapes, dev)
    opt = make(ps)
    scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=1 << 30)
    scaler.scale(torch.zeros((), device=dev))        # the scale tensor is created lazily

    def call():
        scaler.step(opt)
        scaler.update()
    return call, (ps, opt, scaler)


def _plain_leg(make, shapes, dev, bind=False):
    ps = _params(shapes, dev)
    opt = make(ps)
    if bind:                                         # what GradScaler.step binds, by hand: the kernel without the scaler
        opt.grad_scale = torch.ones((), device=dev)
        opt.found_inf = torch.zeros((), device=dev)
    return opt.step, (ps, opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: nothing about speed is said from a CPU run"
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the stream rate of this run: shacira_stream_probe, copy (read + write), 256 MiB each way
    nb = 256 << 20
    src, dst = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
    strm = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    probe = lambda: _lib.check(_lib.lib().shacira_stream_probe(2, src.data_ptr(), dst.data_ptr(), nb, strm), "stream_probe")
    for _ in range(5):
        probe()
    copy_gbs = 2 * nb / (statistics.median(_window(probe, 20) for _ in range(5)) * 1e-6) / 1e9
    say(f"stream probe, copy (read + write) of 2 x 256 MiB: {copy_gbs:.0f} GB/s")
    del src, dst

    adam, rms = dict(lr=1e-3, eps=1e-15), dict(lr=1e-3)
    for name, table in TABLES.items():
        for with_decoder in (False, True):
            shapes = [table] + (DECODER if with_decoder else [])
            numel = sum(torch.Size(s).numel() for s in shapes)
            say(f"# {name}{' + decoder tensors' if with_decoder else ''}: {len(shapes)} tensors, {numel} elements")
            legs = {
                "(a) scaler + FusedAdam(capturable=True)": _scaled_leg(lambda p: FusedAdam(p, capturable=True, **adam), shapes, dev),
                "(a) scaler + FusedAdam(), generic path": _scaled_leg(lambda p: FusedAdam(p, **adam), shapes, dev),
                "(b) scaler + FusedRMSprop(capturable=True)": _scaled_leg(lambda p: FusedRMSprop(p, capturable=True, **rms), shapes, dev),
                "(b) scaler + torch RMSprop(foreach), generic path": _scaled_leg(lambda p: torch.optim.RMSprop(p, foreach=True, **rms), shapes, dev),
                "(c) FusedRMSprop().step()": _plain_leg(lambda p: FusedRMSprop(p, **rms), shapes, dev),
                "(c) torch RMSprop(foreach).step()": _plain_leg(lambda p: torch.optim.RMSprop(p, foreach=True, **rms), shapes, dev),
                "kernel: FusedAdam().step(), 7 dwords": _plain_leg(lambda p: FusedAdam(p, **adam), shapes, dev),
                "kernel: FusedAdam(capturable) scale bound, 8 dwords": _plain_leg(lambda p: FusedAdam(p, capturable=True, **adam), shapes, dev, True),
                "kernel: FusedRMSprop(capturable) scale bound, 6 dwords": _plain_leg(lambda p: FusedRMSprop(p, capturable=True, **rms), shapes, dev, True),
                "kernel: FusedRMSprop(momentum=0.9).step(), 7 dwords": _plain_leg(lambda p: FusedRMSprop(p, momentum=0.9, **rms), shapes, dev),
            }
            grads = [p.grad for p in _params(shapes, dev)]
            found, inv = torch.zeros((), device=dev), torch.ones((), device=dev)
            legs["scaler's inf check alone (foreach check-and-unscale)"] = (
                lambda: torch._amp_foreach_non_finite_check_and_unscale_(grads, found, inv), None)
            dwords = {"(c) FusedRMSprop().step()": 5}
            for leg in legs:
                if "dwords" in leg:
                    dwords[leg] = int(leg.rsplit(",", 1)[1].split()[0])
            for call, _ in legs.values():
                for _ in range(5):
                    call()
            torch.cuda.synchronize()
            t = {leg: [] for leg in legs}
            for _ in range(args.samples):                   # the legs alternate inside every round
                for leg, (call, _) in legs.items():
                    t[leg].append(_window(call, args.calls))
            med = {leg: statistics.median(v) for leg, v in t.items()}
            for leg, v in t.items():
                rate = ""
                if leg in dwords:
                    gbs = numel * 4 * dwords[leg] / (med[leg] * 1e-6) / 1e9
                    rate = f"   {gbs:7.0f} GB/s = {gbs / copy_gbs:.2f} of the probe's copy rate (launch and host time included)"
                say(f"{leg:58s} us/call  min {min(v):8.1f}  median {med[leg]:8.1f}  max {max(v):8.1f}{rate}")
            a1, a0 = med["(a) scaler + FusedAdam(capturable=True)"], med["(a) scaler + FusedAdam(), generic path"]
            b1, b0 = med["(b) scaler + FusedRMSprop(capturable=True)"], med["(b) scaler + torch RMSprop(foreach), generic path"]
            c1, c0 = med["(c) FusedRMSprop().step()"], med["(c) torch RMSprop(foreach).step()"]
            chk = med["scaler's inf check alone (foreach check-and-unscale)"]
            say(f"(a) {a0 / a1:.2f}x   (b) {b0 / b1:.2f}x   (c) {c0 / c1:.2f}x   (generic or torch over fused, medians); "
                f"the inf check is {chk / a1:.0%} of the fused (a) call")
            say("")
            del legs, grads
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
