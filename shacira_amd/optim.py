"""Fused Adam and RMSprop for the hash-grid path's parameters ("next" row f1 of SURVEY.md section 8).

``FusedAdam`` is a drop-in for ``torch.optim.Adam`` (the optimiser the reference's trainers build,
wisp/trainers/base_trainer.py:206-266) restricted to what those configs use: amsgrad=False, maximize=False, L2
``weight_decay``, per-group ``lr``. All fp32 GPU parameters that share (betas, eps) are stepped by ONE multi-tensor HIP launch
(``shacira_adam_step_multi``, up to 32 tensors per launch) instead of torch's ~10-kernel foreach chain; with
``zero_grad_in_step=True`` the same pass clears ``.grad`` (useful with ``dist.FlatGradients``, whose gradient buffer is
persistent); ``capturable=True`` keeps the step count on the device so ``step()`` can be recorded into a HIP graph. State dict
keys (``step``, ``exp_avg``, ``exp_avg_sq``) match torch's. Parameters that are not fp32-contiguous-on-GPU are stepped with the
same formula in torch ops.

``FusedRMSprop`` is the same for ``torch.optim.RMSprop`` (``optimizer_type: 'rmsprop'`` of the reference's nerf_base.yaml):
centered=False, maximize=False, state dict keys ``step``, ``square_avg``, ``momentum_buffer``.

Mixed precision: with ``capturable=True`` both classes follow torch's protocol for optimizers that handle the loss scale
themselves (``_step_supports_amp_scaling``): ``torch.amp.GradScaler.step`` runs its device-side inf check, binds
``optimizer.grad_scale`` and ``optimizer.found_inf`` (device tensors) and calls ``step()`` -- no unscale pass, no ``.item()``.
The kernels divide the gradient by the scale, skip the whole step when ``found_inf`` is non-zero, and the device step count
advances by ``found_inf == 0``; all of it on the stream, so a scaled step replays from a HIP graph. The protocol follows
``capturable`` because only the device-resident count can stand still on a skipped step without the host knowing.
"""
import ctypes
import math

import torch

from . import _lib
from .hip_ops import _on_device

_MAX = 32


def _fused_ok(p, g):
    return (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
            and g.dtype == torch.float32 and not g.is_sparse)


def _amp_tensors(opt):
    """(grad_scale, found_inf) as GradScaler binds them for the duration of one step() -- or a caller sets them -- else None."""
    return getattr(opt, "grad_scale", None), getattr(opt, "found_inf", None)


def _amp_ptr(t, device):
    """Device pointer of a one-element fp32 tensor; the converted tensor is returned too so that it outlives the launch."""
    if t is None:
        return None, None
    t = t.to(device=device, dtype=torch.float32)
    return ctypes.c_void_p(t.data_ptr()), t


def _bump(counter, found_inf):
    """Advance a device step counter on the stream (part of a captured graph); a skipped step does not count."""
    if found_inf is None:
        counter += 1
    else:
        counter += found_inf.to(counter.device) == 0


def _split_shared_counters(opt):
    """capturable: a device counter is shared by the parameters that have been stepped TOGETHER so far. When only some of its
    sharers have a gradient in this step (the others were skipped: grad None), the stepping ones move to a copy of the counter
    first, so that a skipped parameter's count -- and its later bias correction -- stays its own (torch.optim semantics).
    Eager bookkeeping: under graph replay the set of stepped parameters is fixed."""
    by_counter = {}
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p)
            if st and "step" in st and torch.is_tensor(st["step"]) and st["step"].is_cuda:
                by_counter.setdefault(st["step"].data_ptr(), (st["step"], [], []))[1 if p.grad is not None else 2].append(p)
    for sd, stepping, skipped in by_counter.values():
        if stepping and skipped:
            fresh = sd.clone()
            for p in stepping:
                opt.state[p]["step"] = fresh


def _new_counter(opt, p, born):
    if not opt.capturable:
        return torch.tensor(0.0)
    if p.device not in born:                         # one shared device counter for everything born in this step
        born[p.device] = torch.zeros((1,), dtype=torch.int32, device=p.device)
    return born[p.device]


def _restore_counters(opt):
    """After load_state_dict: host float counts, or (capturable) equal counts on one device re-shared as one device counter."""
    shared = {}
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p)
            if not st or "step" not in st:
                continue
            t = int(torch.as_tensor(st["step"]).item())
            if opt.capturable:
                key = (p.device, t)
                if key not in shared:
                    shared[key] = torch.full((1,), t, dtype=torch.int32, device=p.device)
                st["step"] = shared[key]
            else:
                st["step"] = torch.tensor(float(t))


def _host_skip(opt, found_inf):
    """capturable=False keeps the counts on the host, so a caller-set ``found_inf`` is read back once to leave them alone on a
    skipped step (GradScaler never takes this path: the protocol is advertised with capturable=True only)."""
    return found_inf is not None and not opt.capturable and bool(found_inf.item() != 0)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, zero_grad_in_step=False,
                 capturable=False):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.zero_grad_in_step = zero_grad_in_step
        self.capturable = capturable
        if capturable:
            self._step_supports_amp_scaling = True   # torch.amp.GradScaler.step: bind grad_scale / found_inf and call step()

    # Bias correction follows every parameter's OWN ``state['step']`` (as torch.optim.Adam does): a parameter that gets its
    # first gradient late starts at t = 1, and a restored checkpoint continues at the saved count. Parameters that share a
    # count are stepped by one launch. capturable: the count is an int32 DEVICE tensor shared by the parameters that were
    # born in the same step (the kernel reads it, so the launch can be replayed from a HIP graph while it advances).
    def _launch(self, batch, b1, b2, eps, device, step, step_dev, grad_scale=None, found_inf=None):
        k = len(batch)
        PtrArr, I64Arr, FArr = ctypes.c_void_p * k, ctypes.c_int64 * k, ctypes.c_float * k
        ps = PtrArr(*[p.data_ptr() for p, _, _, _, _, _ in batch])
        gs = PtrArr(*[g.data_ptr() for _, g, _, _, _, _ in batch])
        ms = PtrArr(*[m.data_ptr() for _, _, m, _, _, _ in batch])
        vs = PtrArr(*[v.data_ptr() for _, _, _, v, _, _ in batch])
        ns = I64Arr(*[p.numel() for p, _, _, _, _, _ in batch])
        lrs = FArr(*[float(lr) for _, _, _, _, lr, _ in batch])
        wds = FArr(*[float(wd) for _, _, _, _, _, wd in batch])
        sd = ctypes.c_void_p(step_dev.data_ptr()) if step_dev is not None else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        with _on_device(device):
            if grad_scale is None and found_inf is None:
                rc = _lib.lib().shacira_adam_step_multi(k, ns, ps, gs, ms, vs, lrs, wds, float(b1), float(b2), float(eps),
                                                        int(step), sd, int(self.zero_grad_in_step), stream)
            else:
                scale_ptr, _keep_s = _amp_ptr(grad_scale, device)
                inf_ptr, _keep_i = _amp_ptr(found_inf, device)
                rc = _lib.lib().shacira_adam_step_multi_scaled(k, ns, ps, gs, ms, vs, lrs, wds, float(b1), float(b2),
                                                               float(eps), int(step), sd, int(self.zero_grad_in_step),
                                                               scale_ptr, inf_ptr, stream)
        _lib.check(rc, "adam_step_multi")

    def _new_state(self, p, born):
        st = self.state[p]
        st["step"] = _new_counter(self, p, born)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = _amp_tensors(self)
        host_skip = _host_skip(self, found_inf)
        pending = {}      # (device, b1, b2, eps, step key) -> (host step, device step tensor, [tensors])
        bumped = set()    # device counters already advanced in this call
        born = {}
        if self.capturable:
            _split_shared_counters(self)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if host_skip:                        # nothing moves, no count advances; a persistent gradient is still cleared
                    if self.zero_grad_in_step:
                        p.grad.zero_()
                    continue
                st = self.state[p]
                if not st:
                    st = self._new_state(p, born)
                g, m, v = p.grad, st["exp_avg"], st["exp_avg_sq"]
                fused = _fused_ok(p, g)
                if self.capturable:
                    if not fused:
                        raise RuntimeError("FusedAdam(capturable=True) handles fp32 contiguous GPU parameters only")
                    sd = st["step"]
                    if sd.data_ptr() not in bumped:
                        _bump(sd, found_inf)         # on the stream: part of the captured graph
                        bumped.add(sd.data_ptr())
                    key = (p.device, b1, b2, group["eps"], sd.data_ptr())
                    pending.setdefault(key, (1, sd, []))[2].append((p, g, m, v, group["lr"], group["weight_decay"]))
                    continue
                st["step"] += 1
                t = int(st["step"])
                if fused:
                    key = (p.device, b1, b2, group["eps"], t)
                    pending.setdefault(key, (t, None, []))[2].append((p, g, m, v, group["lr"], group["weight_decay"]))
                    continue
                if grad_scale is not None:
                    g.div_(grad_scale.to(g.device))
                gr = g.add(p, alpha=group["weight_decay"]) if group["weight_decay"] else g
                m.mul_(b1).add_(gr, alpha=1 - b1)
                v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
                denom = (v.sqrt() / math.sqrt(1 - b2 ** t)).add_(group["eps"])
                p.addcdiv_(m, denom, value=-group["lr"] / (1 - b1 ** t))
                if self.zero_grad_in_step:
                    g.zero_()
        for (device, b1, b2, eps, _), (t, sd, items) in pending.items():
            for i in range(0, len(items), _MAX):
                self._launch(items[i:i + _MAX], b1, b2, eps, device, t, sd, grad_scale, found_inf)
        return loss

    def load_state_dict(self, state_dict):
        """torch.optim.Adam-compatible: restores the moments AND the per-parameter step counts (a checkpoint written by
        torch.optim.Adam or by this class). capturable: equal counts on one device are re-shared as one device counter."""
        super().load_state_dict(state_dict)
        _restore_counters(self)


class FusedRMSprop(torch.optim.Optimizer):
    """``torch.optim.RMSprop`` (centered=False, maximize=False) on one multi-tensor HIP launch per (alpha, eps, momentum):
        g' = g + wd*p ; sq = alpha*sq + (1-alpha)*g'^2 ; avg = sqrt(sq) + eps
        momentum == 0: p -= lr*g'/avg       otherwise: buf = momentum*buf + g'/avg ; p -= lr*buf
    Grouping, ``zero_grad_in_step``, ``capturable`` and the loss-scale protocol are FusedAdam's (module docstring). ``step`` is
    kept for torch's state dict only: no term of the update depends on it."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False,
                 zero_grad_in_step=False, capturable=False):
        if centered:
            raise NotImplementedError("FusedRMSprop: centered=True is not implemented (no reference configuration uses it)")
        if lr < 0 or eps < 0 or alpha < 0 or weight_decay < 0 or momentum < 0:
            raise ValueError("invalid RMSprop hyper-parameter")
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False,
                                      weight_decay=weight_decay))
        self.zero_grad_in_step = zero_grad_in_step
        self.capturable = capturable
        if capturable:
            self._step_supports_amp_scaling = True

    def _launch(self, batch, alpha, eps, momentum, device, grad_scale, found_inf):
        k = len(batch)
        PtrArr, I64Arr, FArr = ctypes.c_void_p * k, ctypes.c_int64 * k, ctypes.c_float * k
        ps = PtrArr(*[p.data_ptr() for p, _, _, _, _, _ in batch])
        gs = PtrArr(*[g.data_ptr() for _, g, _, _, _, _ in batch])
        sqs = PtrArr(*[sq.data_ptr() for _, _, sq, _, _, _ in batch])
        bufs = PtrArr(*[buf.data_ptr() for _, _, _, buf, _, _ in batch]) if momentum > 0 else None
        ns = I64Arr(*[p.numel() for p, _, _, _, _, _ in batch])
        lrs = FArr(*[float(lr) for _, _, _, _, lr, _ in batch])
        wds = FArr(*[float(wd) for _, _, _, _, _, wd in batch])
        scale_ptr, _keep_s = _amp_ptr(grad_scale, device)
        inf_ptr, _keep_i = _amp_ptr(found_inf, device)
        with _on_device(device):
            rc = _lib.lib().shacira_rmsprop_step_multi(k, ns, ps, gs, sqs, bufs, lrs, wds, float(alpha), float(eps),
                                                       float(momentum), scale_ptr, inf_ptr, int(self.zero_grad_in_step),
                                                       ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        _lib.check(rc, "rmsprop_step_multi")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = _amp_tensors(self)
        host_skip = _host_skip(self, found_inf)
        pending = {}      # (device, alpha, eps, momentum) -> [tensors]
        bumped = set()
        born = {}
        if self.capturable:
            _split_shared_counters(self)
        for group in self.param_groups:
            if group.get("centered") or group.get("maximize"):
                raise NotImplementedError("FusedRMSprop: centered / maximize are not implemented")
            alpha, eps, momentum, lr, wd = (group[k] for k in ("alpha", "eps", "momentum", "lr", "weight_decay"))
            for p in group["params"]:
                if p.grad is None:
                    continue
                if host_skip:
                    if self.zero_grad_in_step:
                        p.grad.zero_()
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = _new_counter(self, p, born)
                    st["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if momentum > 0:
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                g, sq, buf = p.grad, st["square_avg"], st.get("momentum_buffer")
                fused = _fused_ok(p, g)
                if self.capturable:
                    if not fused:
                        raise RuntimeError("FusedRMSprop(capturable=True) handles fp32 contiguous GPU parameters only")
                    if st["step"].data_ptr() not in bumped:
                        _bump(st["step"], found_inf)
                        bumped.add(st["step"].data_ptr())
                else:
                    st["step"] += 1
                if fused:
                    pending.setdefault((p.device, alpha, eps, momentum), []).append((p, g, sq, buf, lr, wd))
                    continue
                if grad_scale is not None:
                    g.div_(grad_scale.to(g.device))
                gr = g.add(p, alpha=wd) if wd != 0 else g                      # torch's _single_tensor_rmsprop, op for op
                sq.mul_(alpha).addcmul_(gr, gr, value=1 - alpha)
                avg = sq.sqrt().add_(eps)
                if momentum > 0:
                    buf.mul_(momentum).addcdiv_(gr, avg)
                    p.add_(buf, alpha=-lr)
                else:
                    p.addcdiv_(gr, avg, value=-lr)
                if self.zero_grad_in_step:
                    g.zero_()
        for (device, alpha, eps, momentum), items in pending.items():
            for i in range(0, len(items), _MAX):
                self._launch(items[i:i + _MAX], alpha, eps, momentum, device, grad_scale, found_inf)
        return loss

    def load_state_dict(self, state_dict):
        """torch.optim.RMSprop-compatible, both ways; the step counts are restored as FusedAdam restores them."""
        super().load_state_dict(state_dict)
        _restore_counters(self)
