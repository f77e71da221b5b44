"""Loss-scaled fused optimizers, the parts that need no GPU: the fp64 RMSprop reference against torch.optim.RMSprop,
FusedRMSprop's torch-op path (CPU parameters) bit for bit against torch, state-dict exchange with torch both ways, and the
GradScaler protocol flags (tests/test_gpu_optim_amp.py holds the kernels to the reference)."""
import copy
import inspect

import numpy as np
import pytest
import torch

import optim_amp_ref
from shacira_amd import _lib
from shacira_amd.optim import FusedAdam, FusedRMSprop


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_equals_torch_rmsprop_in_float64(momentum, wd):
    """torch gets the hyper-parameters as the C-ABI would carry them (rounded to fp32, as the reference rounds them itself);
    relative to the largest magnitude of each tensor."""
    rng = np.random.default_rng(3)
    lr, alpha, eps, momentum, wd = (float(np.float32(x)) for x in (0.01, 0.99, 1e-8, momentum, wd))
    n = 4099
    p = rng.standard_normal(n) * 0.1
    sq = rng.random(n) * 0.01
    buf = rng.standard_normal(n) * 0.1 if momentum else None
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.RMSprop([tp], lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=momentum, foreach=False)
    opt.state[tp] = {"step": torch.tensor(0.0), "square_avg": torch.from_numpy(sq.copy())}
    if momentum:
        opt.state[tp]["momentum_buffer"] = torch.from_numpy(buf.copy())
    for _ in range(4):
        g = rng.standard_normal(n)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, sq, buf, _ = optim_amp_ref.rmsprop_step(p, g, sq, buf, lr, alpha, eps, wd, momentum)
        for got, want in ((tp.detach().numpy(), p), (opt.state[tp]["square_avg"].numpy(), sq)) + \
                (((opt.state[tp]["momentum_buffer"].numpy(), buf),) if momentum else ()):
            assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_cpu_parameters_step_bit_for_bit_like_torch(momentum, wd):
    torch.manual_seed(5)
    shapes = [(33, 2), (7,), (0,), (5, 3, 2)]
    mine = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    a = FusedRMSprop([dict(params=mine[:2], lr=0.02), dict(params=mine[2:], weight_decay=wd)], lr=1e-2, momentum=momentum)
    b = torch.optim.RMSprop([dict(params=theirs[:2], lr=0.02), dict(params=theirs[2:], weight_decay=wd)], lr=1e-2,
                            momentum=momentum, foreach=False)
    for _ in range(5):
        for p, q in zip(mine, theirs):
            p.grad = torch.randn_like(p)
            q.grad = p.grad.clone()
        a.step()
        b.step()
        for p, q in zip(mine, theirs):
            assert torch.equal(p, q)
            assert torch.equal(a.state[p]["square_avg"], b.state[q]["square_avg"])
            assert ("momentum_buffer" in a.state[p]) == (momentum > 0)
            if momentum:
                assert torch.equal(a.state[p]["momentum_buffer"], b.state[q]["momentum_buffer"])
            assert int(a.state[p]["step"]) == int(b.state[q]["step"])


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_state_dict_loads_into_torch_rmsprop_and_back(momentum):
    torch.manual_seed(6)

    def make(cls, **kw):
        ps = [torch.nn.Parameter(torch.randn(9, 2)), torch.nn.Parameter(torch.randn(4))]
        return ps, cls(ps, lr=1e-2, momentum=momentum, weight_decay=0.01, **kw)

    grads = [[torch.randn(9, 2), torch.randn(4)] for _ in range(4)]

    def run(ps, opt, which):
        for k in which:
            for p, g in zip(ps, grads[k]):
                p.grad = g.clone()
            opt.step()

    ps_a, a = make(FusedRMSprop)
    run(ps_a, a, [0, 1])
    ps_b, b = make(torch.optim.RMSprop, foreach=False)
    with torch.no_grad():
        for p, q in zip(ps_a, ps_b):
            q.copy_(p)
    b.load_state_dict(copy.deepcopy(a.state_dict()))        # ours -> torch (load_state_dict does not copy the tensors)
    assert set(b.state[ps_b[0]]) == {"step", "square_avg"} | ({"momentum_buffer"} if momentum else set())
    run(ps_a, a, [2])
    run(ps_b, b, [2])
    assert all(torch.equal(p, q) for p, q in zip(ps_a, ps_b))
    ps_c, c = make(FusedRMSprop)
    with torch.no_grad():
        for p, q in zip(ps_b, ps_c):
            q.copy_(p)
    c.load_state_dict(copy.deepcopy(b.state_dict()))        # torch -> ours
    run(ps_b, b, [3])
    run(ps_c, c, [3])
    assert all(torch.equal(p, q) for p, q in zip(ps_b, ps_c))
    assert all(int(c.state[p]["step"]) == 4 for p in ps_c)


@pytest.mark.parametrize("cls", [FusedAdam, FusedRMSprop])
def test_torch_op_path_unscales_and_skips_like_the_kernels(cls):
    """Parameters the kernels do not take (here: CPU) with a caller-set scale and flag, host-resident counts: a power-of-two
    scale changes no bit, .grad comes back unscaled, and a set flag leaves everything, the count included, as it was."""
    torch.manual_seed(7)
    g = torch.randn(33)
    plain, scaled, skipped = (torch.nn.Parameter(torch.linspace(-1, 1, 33)) for _ in range(3))
    opts = [cls([p], weight_decay=0.01) for p in (plain, scaled, skipped)]
    plain.grad, scaled.grad, skipped.grad = g.clone(), g * 8.0, g * 8.0
    opts[1].grad_scale, opts[1].found_inf = torch.tensor(8.0), torch.tensor(0.0)
    opts[2].grad_scale, opts[2].found_inf = torch.tensor(8.0), torch.tensor(1.0)
    for o in opts:
        o.step()
    assert torch.equal(plain, scaled) and torch.equal(scaled.grad, g)
    for key, value in opts[0].state[plain].items():
        assert torch.equal(value, opts[1].state[scaled][key]), key
    assert torch.equal(skipped.detach(), torch.linspace(-1, 1, 33)) and torch.equal(skipped.grad, g * 8.0)
    assert not opts[2].state[skipped]                           # no state was born, no count advanced


def test_centered_is_refused():
    with pytest.raises(NotImplementedError):
        FusedRMSprop([torch.nn.Parameter(torch.zeros(3))], centered=True)


@pytest.mark.parametrize("cls", [FusedAdam, FusedRMSprop])
def test_amp_protocol_follows_capturable(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert not hasattr(cls(p, capturable=False), "_step_supports_amp_scaling")
    assert cls(p, capturable=True)._step_supports_amp_scaling is True
    # torch.amp.GradScaler.step inspects the signature and takes a deprecated path when it finds this keyword
    assert "grad_scaler" not in inspect.signature(cls(p, capturable=True).step).parameters


def test_ctypes_table_lists_the_new_symbols():
    assert "shacira_adam_step_multi_scaled" in _lib.SIGNATURES
    assert "shacira_rmsprop_step_multi" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["shacira_adam_step_multi_scaled"][1]) == len(_lib.SIGNATURES["shacira_adam_step_multi"][1]) + 2
    assert len(_lib.SIGNATURES["shacira_rmsprop_step_multi"][1]) == 15
