"""adam.hip at its edges against one Adam step in float64 (tests/adam_ref.py): both kernels, all three outputs.

`adam_multi_kernel` through FusedAdam: sizes at the float4 edge and at the 8192-element chunk edge, as own allocations and as
4-byte-aligned views into one flat buffer (what dist.FlatGradients hands over), more than 32 tensors (a second and a third
launch), empty tensors inside the list, two groups, lr = 0, a restored capturable count, zero_grad_in_step. `adam_step_kernel`
through the C-ABI (`shacira_adam_step`, `shacira_adam_step_capturable`), which nothing else calls: the float4 / scalar split, the
second trip of its grid-stride loop, 4-byte-aligned pointers, and agreement with the multi-tensor kernel bit for bit.

Bars, one step from the same fp32 state: exp_avg within 2^-22 (|b1 m0| + |(1 - b1) g'|), exp_avg_sq within 2^-22 (|b2 v0| +
|(1 - b2) g'^2|), p within 2^-23 |p0| + allowance * scale. `scale` is the update's size before exp_avg's terms cancel and the
allowance is four times what CPU torch.optim.Adam (fp32, foreach=False) misses the reference by on the same inputs, floor 2^-21
(adam_ref.update_allowance). Measured on the MI355X: on 4_195_331 elements torch's worst is 2.2e-7 of the scale (allowance
8.9e-7) and all three entries reach 2.5e-7 to 2.6e-7; on the multi-tensor sets the kernels' worst is 1.7e-7 to 1.9e-7 and on the
small single tensors at most 1.0e-7 (torch at most 1.2e-7), where the floor 4.8e-7 holds. In units of the cancelled update itself
torch is 3% to 13% off on 4M elements (the update vanishes where its error does not), which measures nothing; hence the scale."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 2, 3, 4, 5, 8191, 8192, 8193, 8195, 16386]
HYPER = [dict(lr=0.02, wd=0.0), dict(lr=1e-3, wd=0.01)]          # the two groups
B1, B2, EPS = 0.9, 0.999, 1e-8
SENTINEL = np.float32(-1234.5678)


def _state(rng, n):
    return ((rng.standard_normal(n) * 0.1).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.random(n) * 0.01).astype(np.float32))


class _Set:
    """Parameters with given state, each one an allocation of its own or four views into one flat fp32 buffer. The views of
    tensor k start at element offsets (k + 1, k + 2, k + 3, k) mod 4 for p, g, exp_avg, exp_avg_sq: over the tensors every
    role meets every misalignment. The gaps between the views hold a sentinel."""

    def __init__(self, sizes, as_view, rng, t, capturable=False, hyper=HYPER, **opt_kw):
        self.init = [_state(rng, n) for n in sizes]
        self.group = [k % len(hyper) for k in range(len(sizes))]
        self.hyper, self.t = hyper, t
        cursor, where = 0, []
        for k, n in enumerate(sizes):
            if not as_view[k]:
                where.append(None)
                continue
            starts = []
            for role in range(4):
                s = cursor + 2                                   # at least two sentinel elements before every view
                s += ((k + 1 + role) % 4 - s) % 4
                starts.append(s)
                cursor = s + n
            where.append(starts)
        host = np.full(cursor + 6, SENTINEL, np.float32)
        self.used = np.zeros(cursor + 6, bool)
        for k, starts in enumerate(where):
            if starts is not None:
                for s, a in zip(starts, self.init[k]):
                    host[s:s + a.shape[0]] = a
                    self.used[s:s + a.shape[0]] = True
        self.flat = torch.from_numpy(host).to(DEV)
        self.before = host.copy()
        self.params, self.moments = [], []
        for k, starts in enumerate(where):
            if starts is None:
                ts = [torch.from_numpy(a.copy()).to(DEV) for a in self.init[k]]
            else:
                ts = [self.flat[s:s + sizes[k]] for s in starts]
                assert all(x.data_ptr() % 16 == 4 * ((k + 1 + role) % 4) for role, x in enumerate(ts)) or sizes[k] == 0
            p = torch.nn.Parameter(ts[0])
            p.grad = ts[1]
            assert p.data_ptr() == ts[0].data_ptr()
            self.params.append(p)
            self.moments.append((ts[2], ts[3]))
        from shacira_amd.optim import FusedAdam
        groups = [dict(params=[p for p, g in zip(self.params, self.group) if g == i], lr=h["lr"], weight_decay=h["wd"])
                  for i, h in enumerate(hyper)]
        self.opt = FusedAdam(groups, betas=(B1, B2), eps=EPS, capturable=capturable, **opt_kw)
        count = torch.full((1,), t - 1, dtype=torch.int32, device=DEV) if capturable else None
        for p, (m, v) in zip(self.params, self.moments):
            self.opt.state[p] = {"step": count if capturable else torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}

    def step(self):
        self.opt.step()
        torch.cuda.synchronize()
        return self

    def check(self, grads_zeroed=False):
        """Every tensor against the reference, the gradients (kept, or cleared to exact zeros) and the bytes between the views."""
        worst = 0.0
        for i, h in enumerate(self.hyper):
            ks = [k for k, g in enumerate(self.group) if g == i]
            hyper = dict(lr=h["lr"], b1=B1, b2=B2, eps=EPS, wd=h["wd"])
            allowance, measured = adam_ref.update_allowance(*[np.concatenate([self.init[k][j] for k in ks]) for j in range(4)],
                                                            self.t, **hyper)
            for k in ks:
                p0, g0, m0, v0 = self.init[k]
                p_ref, m_ref, v_ref, scale = adam_ref.adam_step(p0, g0, m0, v0, self.t, **hyper)
                m_bar, v_bar = adam_ref.moment_bars(p0, g0, m0, v0, B1, B2, h["wd"])
                p, m, v = (x.detach().cpu().numpy() for x in (self.params[k], *self.moments[k]))
                assert np.all(np.abs(m - m_ref) <= m_bar), (k, "exp_avg")
                assert np.all(np.abs(v - v_ref) <= v_bar), (k, "exp_avg_sq")
                assert np.all(np.abs(p - p_ref) <= 2.0 ** -23 * np.abs(p0) + allowance * scale), (k, "p", allowance, measured)
                if p0.size:
                    worst = max(worst, float(adam_ref.update_error(p, p0, p_ref, scale).max()))
                    assert h["lr"] == 0 or np.any(p != p0)
                g = self.params[k].grad.cpu().numpy()
                assert (not g.any()) if grads_zeroed else np.array_equal(g, g0), (k, "grad")
        after = self.flat.cpu().numpy()
        assert np.array_equal(after.view(np.int32)[~self.used], self.before.view(np.int32)[~self.used]), "bytes between the views"
        return worst


@pytest.mark.parametrize("mode", ["own", "views", "all"])
def test_multi_tensor_step_at_the_vector_and_chunk_edges(mode):
    rng = np.random.default_rng(1)
    sizes, as_view = {"own": (SIZES, [False] * 10), "views": (SIZES, [True] * 10),
                      "all": (SIZES + SIZES, [False] * 10 + [True] * 10)}[mode]
    worst = _Set(sizes, as_view, rng, t=7).step().check()
    print(f"{mode}: worst p error {worst:.3g} of the update scale")


@pytest.mark.parametrize("count", [33, 65])
def test_more_than_32_tensors_take_further_launches(count):
    rng = np.random.default_rng(count)
    sizes = [1 + (7 * k) % 23 for k in range(count)]
    sizes[32] = 8193                                              # first tensor of the second launch: two chunks
    _Set(sizes, [k % 2 == 1 for k in range(count)], rng, t=3).step().check()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("view", [False, True])
def test_zero_element_parameter_with_a_gradient(where, view):
    rng = np.random.default_rng(9)
    sizes = [5, 8193, 3]
    sizes.insert({"first": 0, "middle": 2, "last": 3}[where], 0)
    s = _Set(sizes, [view] * 4, rng, t=2).step()
    s.check()
    assert int(s.opt.state[s.params[sizes.index(0)]]["step"]) == 2


def test_lr_zero_leaves_p_bit_identical():
    rng = np.random.default_rng(4)
    s = _Set(SIZES, [k % 2 == 0 for k in range(10)], rng, t=5, hyper=[dict(lr=0.0, wd=0.01), dict(lr=0.0, wd=0.0)]).step()
    s.check()                                                     # the moments still move
    for p, (p0, _, m0, _), (m, _) in zip(s.params, s.init, s.moments):
        assert np.array_equal(p.detach().cpu().numpy().view(np.int32), p0.view(np.int32))
        assert not np.array_equal(m.cpu().numpy(), m0)


def test_capturable_with_a_restored_count_of_a_million():
    """t = 10^6: b1^t and b2^t underflow to 0, both corrections are exactly 1 (computed on the device from the count)."""
    rng = np.random.default_rng(6)
    s = _Set(SIZES, [k % 2 == 1 for k in range(10)], rng, t=10 ** 6, capturable=True).step()
    s.check()
    assert all(int(s.opt.state[p]["step"].item()) == 10 ** 6 for p in s.params)


@pytest.mark.parametrize("capturable", [False, True])
def test_zero_grad_in_step_clears_every_element_and_nothing_else(capturable):
    rng = np.random.default_rng(8)
    s = _Set(SIZES + [0, 33], [True] * 12, rng, t=4, capturable=capturable, zero_grad_in_step=True).step()
    s.check(grads_zeroed=True)
    s2 = _Set(SIZES, [False] * 10, rng, t=4, capturable=capturable, zero_grad_in_step=True).step()
    s2.check(grads_zeroed=True)


# ------------------------------------------------------------------------------------------- the single-tensor entries (ctypes)
_GUARD = 4      # sentinel elements before and behind every array: 16 bytes, so offset 0 stays 16-byte aligned


def _arrays(init, offsets):
    out = []
    for a, off in zip(init, offsets):
        host = np.full(a.shape[0] + 2 * _GUARD + 3, SENTINEL, np.float32)
        host[_GUARD + off:_GUARD + off + a.shape[0]] = a
        buf = torch.from_numpy(host).to(DEV)
        view = buf[_GUARD + off:_GUARD + off + a.shape[0]]
        assert view.data_ptr() % 16 == 4 * off
        out.append((buf, view))
    return out


def _guards_intact(arrays, n, offsets):
    for (buf, _), off in zip(arrays, offsets):
        host = buf.cpu().numpy().view(np.int32)
        want = SENTINEL.view(np.int32)
        if not (np.all(host[:_GUARD + off] == want) and np.all(host[_GUARD + off + n:] == want)):
            return False
    return True


def _run_single(form, init, offsets, t, h, zero_grad=0):
    from shacira_amd import _lib
    L = _lib.lib()
    n = init[0].shape[0]
    arrays = _arrays(init, offsets)
    ptrs = [v.data_ptr() for _, v in arrays]
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    with torch.cuda.device(0):
        if form == "eager":
            rc = L.shacira_adam_step(n, *ptrs, h["lr"], B1, B2, EPS, h["wd"], t, zero_grad, stream)
        elif form == "capturable":
            count = torch.full((1,), t, dtype=torch.int32, device=DEV)
            rc = L.shacira_adam_step_capturable(n, *ptrs, h["lr"], B1, B2, EPS, h["wd"], count.data_ptr(), zero_grad, stream)
        else:
            one = lambda x: (ctypes.c_void_p * 1)(x)
            rc = L.shacira_adam_step_multi(1, (ctypes.c_int64 * 1)(n), *[one(x) for x in ptrs], (ctypes.c_float * 1)(h["lr"]),
                                           (ctypes.c_float * 1)(h["wd"]), B1, B2, EPS, t, None, zero_grad, stream)
        torch.cuda.synchronize()
    assert rc == 0, (form, rc)
    assert _guards_intact(arrays, n, offsets), (form, "wrote outside its arrays")
    return [v.cpu().numpy() for _, v in arrays]


_SINGLE = [(n, off) for n in (1, 3, 4, 5, 1023, 1024, 1027) for off in ((0, 0, 0, 0), (1, 2, 3, 1))] \
    + [(1027, off) for off in ((1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1))] \
    + [(4_194_304 + 1027, (0, 0, 0, 0)), (4_194_304 + 1027, (3, 1, 2, 0))]


@pytest.mark.parametrize("n,offsets", _SINGLE)
def test_single_tensor_entries_agree_with_the_reference_and_each_other(n, offsets):
    """`shacira_adam_step`, `shacira_adam_step_capturable` (count on the device) and `shacira_adam_step_multi` with one tensor,
    from the same state: each inside the bars, and p, exp_avg, exp_avg_sq bit-identical across the three (the kernels share the
    operation order; the corrections come from the host's pow in the eager form and the device's in the other two, and round
    to the same floats). 4_194_304 + 1027 elements take a second trip of the grid-stride loop at the 4096-block cap; the
    offsets are elements past a 16-byte boundary for p, g, exp_avg, exp_avg_sq."""
    rng = np.random.default_rng(n % 1000 + sum(offsets))
    init = _state(rng, n)
    t, h = 7, HYPER[1]
    hyper = dict(lr=h["lr"], b1=B1, b2=B2, eps=EPS, wd=h["wd"])
    p_ref, m_ref, v_ref, scale = adam_ref.adam_step(*init, t, **hyper)
    m_bar, v_bar = adam_ref.moment_bars(*init, B1, B2, h["wd"])
    allowance, measured = adam_ref.update_allowance(*init, t, **hyper)
    got = {form: _run_single(form, init, offsets, t, h) for form in ("eager", "capturable", "multi")}
    for form, (p, g, m, v) in got.items():
        worst = float(adam_ref.update_error(p, init[0], p_ref, scale).max())
        print(f"n={n} {form}: p error {worst:.3g} of the update scale (torch {measured:.3g}, allowance {allowance:.3g})")
        assert np.all(np.abs(m - m_ref) <= m_bar) and np.all(np.abs(v - v_ref) <= v_bar), form
        assert np.all(np.abs(p - p_ref) <= 2.0 ** -23 * np.abs(init[0]) + allowance * scale), form
        assert np.array_equal(g, init[1]) and np.any(p != init[0]), form
    for form in ("capturable", "multi"):
        for k, name in ((0, "p"), (2, "exp_avg"), (3, "exp_avg_sq")):
            assert np.array_equal(got[form][k].view(np.int32), got["eager"][k].view(np.int32)), (form, name)


@pytest.mark.parametrize("n,offsets", [(5, (1, 2, 3, 1)), (1027, (0, 0, 0, 0)), (1027, (2, 2, 2, 2))])
def test_single_tensor_zero_grad(n, offsets):
    rng = np.random.default_rng(n)
    init = _state(rng, n)
    for form in ("eager", "capturable"):
        p, g, m, v = _run_single(form, init, offsets, 3, HYPER[0], zero_grad=1)
        assert not g.any() and np.any(p != init[0]), form


def test_single_tensor_entries_refuse_wrong_arguments():
    from shacira_amd import _lib
    L = _lib.lib()
    x = [torch.zeros(8, device=DEV) for _ in range(4)]
    ptrs = [a.data_ptr() for a in x]
    count = torch.ones(1, dtype=torch.int32, device=DEV)
    ok = (0.01, B1, B2, EPS, 0.0)
    assert L.shacira_adam_step(8, *ptrs, *ok, 0, 0, None) == _lib.EINVAL                           # step = 0
    assert L.shacira_adam_step(8, *ptrs, 0.01, 1.0, B2, EPS, 0.0, 1, 0, None) == _lib.EINVAL       # beta1 = 1
    assert L.shacira_adam_step(8, *ptrs, 0.01, B1, 1.0, EPS, 0.0, 1, 0, None) == _lib.EINVAL       # beta2 = 1
    assert L.shacira_adam_step_capturable(8, *ptrs, 0.01, B1, 1.0, EPS, 0.0, count.data_ptr(), 0, None) == _lib.EINVAL
    assert L.shacira_adam_step_capturable(8, *ptrs, *ok, None, 0, None) == _lib.EINVAL             # no device count
    assert L.shacira_adam_step(-1, *ptrs, *ok, 1, 0, None) == _lib.EINVAL
    for k in range(4):                                                                             # a null pointer with n > 0
        bad = list(ptrs)
        bad[k] = None
        assert L.shacira_adam_step(8, *bad, *ok, 1, 0, None) == _lib.EINVAL
        assert L.shacira_adam_step_capturable(8, *bad, *ok, count.data_ptr(), 0, None) == _lib.EINVAL
    assert L.shacira_adam_step(0, None, None, None, None, *ok, 1, 0, None) == 0                    # ... but not with n = 0
    torch.cuda.synchronize()
    assert all(not a.any() for a in x)                                                             # nothing ran
