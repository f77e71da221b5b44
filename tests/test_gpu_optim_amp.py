"""The loss-scaled multi-tensor optimizer kernels (shacira_amd/csrc/adam.hip) through FusedAdam and FusedRMSprop, at the edges
tests/test_gpu_adam_edges.py walks -- the float4 edge, the 8192-element chunk edge, own allocations and 4-byte-aligned views
into one flat buffer with sentinels between them, an empty tensor inside the list, 70 tensors (three launches), two groups --
against one step in float64 (tests/adam_ref.py, tests/optim_amp_ref.py). The optimizers are driven the way
torch.amp.GradScaler drives them: `opt.grad_scale` and `opt.found_inf` bound to device tensors.

Bars, one step from the same fp32 state (adam_ref's rules): a state tensor within 2^-22 of the magnitudes that are added into
it, p within 2^-23 |p0| + allowance * scale, allowance = max(4 x CPU torch's worst error on the same inputs, 2^-21); with a
scale that is no power of two the reference steps g_scaled / S (the quotient in float64) and the p allowance is doubled, since
the fp32 quotient adds one rounding to the gradient. A power-of-two scale is exact, so there the bar is 0: every output
bit-identical to the step on the unscaled gradient."""
import functools
import math

import numpy as np
import pytest
import torch

import adam_ref
import optim_amp_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 2, 3, 4, 5, 8191, 8192, 8193, 8195, 16386]
WITH_EMPTY = SIZES[:5] + [0] + SIZES[5:]
HYPER = [dict(lr=0.02, wd=0.0), dict(lr=1e-3, wd=0.01)]          # the two groups
B1, B2, EPS = 0.9, 0.999, 1e-8
ALPHA = 0.99
MOMENTUM = {"adam": None, "rmsprop": 0.0, "rmsprop_m": 0.9}
KINDS = list(MOMENTUM)
SENTINEL = np.float32(-1234.5678)
# No gradient smaller than 0.01 = 2 x wd x (5 sigma of p): g' = g + wd p then never loses more than half of g to cancellation.
# The state bars are 2^-22 of the magnitudes ADDED, |(1 - b) g'| among them, and the fp32 product wd p inside g' carries a
# rounding of 2^-24 |wd p| that no kernel may avoid (the product is a rounding point of its own). Where the two terms cancel
# that rounding outweighs the bar whatever the kernel does: numpy's own fp32 restatement of the plain, unscaled RMSprop step
# is 1.60 bars off in momentum_buffer at one of 114 000 elements drawn without the floor (g = -0.00253, wd p = +0.00246).
G_FLOOR = np.float32(0.01)


def _state(rng, n, kind):
    """[p, g, first state, second state]: (exp_avg, exp_avg_sq) for Adam, (square_avg, momentum_buffer) for RMSprop, the
    buffer only with momentum."""
    p, g = (rng.standard_normal(n) * 0.1).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    g = np.where(np.abs(g) < G_FLOOR, np.copysign(G_FLOOR, g), g).astype(np.float32)
    signed, positive = (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.random(n) * 0.01).astype(np.float32)
    if kind == "adam":
        return [p, g, signed, positive]
    return [p, g, positive] + ([signed] if kind == "rmsprop_m" else [])


def _reference(kind, init, g64, t, h):
    """(p, [states], scale, [state bars]) in float64 for one tensor, stepping the float64 gradient g64."""
    if kind == "adam":
        p0, _, m0, v0 = init
        p, m, v, scale = adam_ref.adam_step(p0, g64, m0, v0, t, lr=h["lr"], b1=B1, b2=B2, eps=EPS, wd=h["wd"])
        return p, [m, v], scale, list(adam_ref.moment_bars(p0, g64, m0, v0, B1, B2, h["wd"]))
    p0, sq0, buf0 = init[0], init[2], init[3] if len(init) > 3 else None
    kw = dict(alpha=ALPHA, eps=EPS, wd=h["wd"], momentum=MOMENTUM[kind])
    p, sq, buf, scale = optim_amp_ref.rmsprop_step(p0, g64, sq0, buf0, h["lr"], **kw)
    sq_bar, buf_bar = optim_amp_ref.state_bars(p0, g64, sq0, buf0, **kw)
    return p, [sq] + ([buf] if buf is not None else []), scale, [sq_bar] + ([buf_bar] if buf is not None else [])


def _allowance(kind, init, g32, t, h):
    """adam_ref.update_allowance's rule on the concatenated tensors of one group: the yardstick is CPU torch."""
    if kind == "adam":
        return adam_ref.update_allowance(init[0], g32, init[2], init[3], t, lr=h["lr"], b1=B1, b2=B2, eps=EPS, wd=h["wd"])
    return optim_amp_ref.update_allowance(init[0], g32, init[2], init[3] if len(init) > 3 else None, lr=h["lr"], alpha=ALPHA,
                                          eps=EPS, wd=h["wd"], momentum=MOMENTUM[kind])


class _Set:
    """Parameters with given state, each one an allocation of its own or views into one flat fp32 buffer. The views of tensor
    k start at element offsets (k + 1 + role) mod 4 for role = p, g, first state, second state: over the tensors every role
    meets every misalignment. The gaps between the views hold a sentinel. `grad_mult`: the stored gradient is g * grad_mult
    (rounded to fp32), what a loss scaled by grad_mult leaves in .grad."""

    def __init__(self, kind, sizes, as_view, seed, t=7, capturable=False, grad_mult=None, hyper=HYPER, **opt_kw):
        rng = np.random.default_rng(seed)
        self.kind, self.sizes, self.hyper, self.t, self.capturable = kind, sizes, hyper, t, capturable
        self.init = [_state(rng, n, kind) for n in sizes]
        if grad_mult is not None:
            for s in self.init:
                s[1] = (s[1] * np.float32(grad_mult)).astype(np.float32)
        self.roles = len(self.init[0])
        self.group = [k % len(hyper) for k in range(len(sizes))]
        cursor, where = 0, []
        for k, n in enumerate(sizes):
            if not as_view[k]:
                where.append(None)
                continue
            starts = []
            for role in range(self.roles):
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
        self.params, self.tensors = [], []
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
            self.tensors.append(ts)
        from shacira_amd.optim import FusedAdam, FusedRMSprop
        groups = [dict(params=[p for p, g in zip(self.params, self.group) if g == i], lr=h["lr"], weight_decay=h["wd"])
                  for i, h in enumerate(hyper)]
        if kind == "adam":
            self.opt = FusedAdam(groups, betas=(B1, B2), eps=EPS, capturable=capturable, **opt_kw)
            names = ("exp_avg", "exp_avg_sq")
        else:
            self.opt = FusedRMSprop(groups, alpha=ALPHA, eps=EPS, momentum=MOMENTUM[kind], capturable=capturable, **opt_kw)
            names = ("square_avg", "momentum_buffer")
        self.count = torch.full((1,), t - 1, dtype=torch.int32, device=DEV) if capturable else None
        for p, ts in zip(self.params, self.tensors):
            self.opt.state[p] = {"step": self.count if capturable else torch.tensor(float(t - 1)),
                                 **{name: x for name, x in zip(names, ts[2:])}}

    def amp(self, grad_scale=None, found_inf=None):
        """Bind what GradScaler.step binds; persistent device tensors (a captured graph holds their addresses)."""
        if grad_scale is not None:
            self.opt.grad_scale = torch.full((), float(grad_scale), dtype=torch.float32, device=DEV)
        if found_inf is not None:
            self.opt.found_inf = torch.full((), float(found_inf), dtype=torch.float32, device=DEV)
        return self

    def set_grads(self, grads):
        for ts, g in zip(self.tensors, grads):
            ts[1].copy_(torch.from_numpy(g))

    def step(self):
        self.opt.step()
        torch.cuda.synchronize()
        return self

    def read(self):
        """[[p, g, states...] as numpy] per tensor."""
        return [[x.detach().cpu().numpy() for x in ts] for ts in self.tensors]

    def sentinels_intact(self):
        after = self.flat.cpu().numpy()
        return np.array_equal(after.view(np.int32)[~self.used], self.before.view(np.int32)[~self.used])

    def check(self, start=None, grad_scale=None, allowance_mult=1.0, grads="kept", t=None, parts=("state", "p", "grad")):
        """Every tensor against the reference stepped from `start` (default: the initial state) on the gradient start[k][1] /
        grad_scale; the gradients afterwards (kept, cleared to exact zeros, or the fp32 quotient); the bytes between the views."""
        start = self.init if start is None else start
        t = self.t if t is None else t
        got, worst, worst_state, failed = self.read(), 0.0, 0.0, []
        for i, h in enumerate(self.hyper):
            ks = [k for k, g in enumerate(self.group) if g == i]
            unscaled32 = {k: start[k][1] if grad_scale is None else start[k][1] / np.float32(grad_scale) for k in ks}
            cat = [np.concatenate([start[k][j] for k in ks]) for j in range(self.roles)]
            allowance, measured = _allowance(self.kind, cat, np.concatenate([unscaled32[k] for k in ks]), t, h)
            allowance *= allowance_mult
            for k in ks:
                g64 = start[k][1].astype(np.float64) / (1.0 if grad_scale is None else float(np.float32(grad_scale)))
                p_ref, s_ref, scale, bars = _reference(self.kind, start[k], g64, t, h)
                p0 = start[k][0]
                for j, (want, bar) in enumerate(zip(s_ref, bars)):
                    err = np.abs(got[k][2 + j] - want)
                    if p0.size:
                        worst_state = max(worst_state, float((err / np.where(bar > 0, bar, 1.0))[bar > 0].max(initial=0.0)))
                    if "state" in parts and not np.all(err <= bar):
                        failed.append((k, "state", j))
                if "p" in parts and not np.all(np.abs(got[k][0] - p_ref) <= 2.0 ** -23 * np.abs(p0) + allowance * scale):
                    failed.append((k, "p", allowance, measured))
                if p0.size:
                    worst = max(worst, float(adam_ref.update_error(got[k][0], p0, p_ref, scale).max()) / allowance)
                    if not np.any(got[k][0] != p0):
                        failed.append((k, "p did not move"))
                if grads == "zeroed":
                    ok = not got[k][1].any()
                else:   # the quotient is one correctly rounded fp32 division on either side
                    ok = np.array_equal(got[k][1].view(np.int32), unscaled32[k].view(np.int32))
                if "grad" in parts and not ok:
                    failed.append((k, "grad"))
        print(f"{self.kind}: worst state error {worst_state:.3f} of its bar, worst p error {worst:.3f} of its allowance")
        assert not failed, failed
        assert self.sentinels_intact(), "bytes between the views"
        return worst


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


MIXED = (WITH_EMPTY + WITH_EMPTY, [False] * 11 + [True] * 11)       # own allocations, then views


# ------------------------------------------------------------------------------------------------------- 1. RMSprop, unscaled
@pytest.mark.parametrize("kind", ["rmsprop", "rmsprop_m"])
@pytest.mark.parametrize("mode", ["own", "views"])
def test_rmsprop_step_at_the_vector_and_chunk_edges(kind, mode):
    _Set(kind, WITH_EMPTY, [mode == "views"] * 11, seed=1).step().check()


@pytest.mark.parametrize("kind", ["rmsprop", "rmsprop_m"])
def test_rmsprop_70_tensors_take_three_launches(kind):
    sizes = [1 + (7 * k) % 23 for k in range(70)]
    sizes[32] = 8193                                              # first tensor of the second launch: two chunks
    sizes[64] = 8195
    _Set(kind, sizes, [k % 2 == 1 for k in range(70)], seed=70).step().check()


@pytest.mark.parametrize("kind", ["rmsprop", "rmsprop_m"])
def test_rmsprop_zero_grad_in_step_clears_every_element_and_nothing_else(kind):
    _Set(kind, *MIXED, seed=8, zero_grad_in_step=True).step().check(grads="zeroed")


def test_rmsprop_entry_refuses_wrong_arguments():
    import ctypes
    from shacira_amd import _lib
    L = _lib.lib()
    x = [torch.zeros(8, device=DEV) for _ in range(4)]
    one = lambda v: (ctypes.c_void_p * 1)(v)
    n, f = (ctypes.c_int64 * 1)(8), (ctypes.c_float * 1)(0.01)
    p, g, sq, buf = (one(a.data_ptr()) for a in x)
    tail = (None, None, 0, None)
    assert L.shacira_rmsprop_step_multi(33, n, p, g, sq, buf, f, f, ALPHA, EPS, 0.0, *tail) == _lib.EINVAL
    assert L.shacira_rmsprop_step_multi(-1, n, p, g, sq, buf, f, f, ALPHA, EPS, 0.0, *tail) == _lib.EINVAL
    assert L.shacira_rmsprop_step_multi(1, n, None, g, sq, buf, f, f, ALPHA, EPS, 0.0, *tail) == _lib.EINVAL
    assert L.shacira_rmsprop_step_multi(1, n, p, g, sq, None, f, f, ALPHA, EPS, 0.9, *tail) == _lib.EINVAL   # momentum, no buffer
    assert L.shacira_rmsprop_step_multi(1, n, p, g, one(None), buf, f, f, ALPHA, EPS, 0.0, *tail) == _lib.EINVAL
    assert L.shacira_adam_step_multi_scaled(33, n, p, g, sq, buf, f, f, B1, B2, EPS, 1, None, 0, None, None, None) == _lib.EINVAL
    assert L.shacira_rmsprop_step_multi(0, None, None, None, None, None, None, None, ALPHA, EPS, 0.0, *tail) == 0
    torch.cuda.synchronize()
    assert all(not a.any() for a in x)                                                              # nothing ran


# ------------------------------------------------------------------------------------------- 2. a power-of-two scale is exact
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scale", [2.0 ** 16, 2.0 ** -3])
def test_power_of_two_scale_changes_no_bit(kind, scale):
    """Stepping g * S with grad_scale = S gives p and every state tensor bit-identical to stepping g without a scale, in both
    groups (wd = 0.01 included: the unscaled value is a rounding point of its own), and .grad comes back as g bit for bit."""
    plain = _Set(kind, *MIXED, seed=2).step()
    plain.check()
    scaled = _Set(kind, *MIXED, seed=2, grad_mult=scale).amp(grad_scale=scale).step()
    want, got = plain.read(), scaled.read()
    assert _bits_equal(want, got)                               # p, states, and the written-back gradient == g
    assert _bits_equal([[g] for _, g, *_ in got], [[s[1]] for s in plain.init])
    assert scaled.sentinels_intact()


# -------------------------------------------------------------------------------------------------- 3. non-power-of-two scale
@functools.lru_cache(maxsize=None)
def _stepped_at_1000(kind):
    return _Set(kind, *MIXED, seed=3, grad_mult=1000.0).amp(grad_scale=1000.0).step()


@pytest.mark.parametrize("kind", KINDS)
def test_scale_of_1000_keeps_p_within_the_doubled_allowance_and_writes_the_quotient_back(kind):
    _stepped_at_1000(kind).check(grad_scale=1000.0, allowance_mult=2.0, parts=("p", "grad"))


@pytest.mark.parametrize("kind", KINDS)
def test_scale_of_1000_keeps_the_state_within_the_single_step_bars(kind):
    """The state bars are the single-step bars, not widened; only the p allowance is doubled. The rounded quotient alone does
    not meet them: its 2^-24 enters g'^2 twice, and numpy's fp32 restatement of that kernel puts the worst exp_avg_sq element
    at 1.10 and the worst square_avg element at 1.30 of the bar (so did the first kernel on the MI355X). The kernels carry
    the division's remainder into the state beside the quotient (optim_chunk_step in adam.hip)."""
    _stepped_at_1000(kind).check(grad_scale=1000.0, allowance_mult=2.0, parts=("state",))


# --------------------------------------------------------------------------------------------------------------------- 4. skip
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("zero_grad", [False, True])
def test_found_inf_skips_the_whole_step(kind, zero_grad):
    s = _Set(kind, *MIXED, seed=4, capturable=True, grad_mult=65536.0, zero_grad_in_step=zero_grad)
    poisoned = [t[1].copy() for t in s.init]
    for k, g in enumerate(poisoned):                              # inf and nan where the scaler would have found them
        if g.size:
            g[0] = np.inf
            g[g.size // 2] = np.nan
            g[-1] = -np.inf
    s.set_grads(poisoned)
    s.amp(grad_scale=65536.0, found_inf=1.0).step()
    got = s.read()
    for k, init in enumerate(s.init):
        assert np.array_equal(got[k][0].view(np.int32), init[0].view(np.int32)), (k, "p")
        for j in range(2, s.roles):
            assert np.array_equal(got[k][j].view(np.int32), init[j].view(np.int32)), (k, "state", j)
        if zero_grad:
            assert np.array_equal(got[k][1].view(np.int32), np.zeros_like(init[1]).view(np.int32)), (k, "grad not cleared")
        else:
            assert np.array_equal(got[k][1].view(np.int32), poisoned[k].view(np.int32)), (k, "grad touched")
    assert int(s.count.item()) == s.t - 1
    # the bytes between the views: compare outside every view (the gradient views changed on purpose above)
    after = s.flat.cpu().numpy()
    assert np.array_equal(after.view(np.int32)[~s.used], s.before.view(np.int32)[~s.used])


@pytest.mark.parametrize("kind", KINDS)
def test_found_inf_zero_without_a_scale_equals_the_unscaled_entry(kind):
    plain = _Set(kind, *MIXED, seed=5, capturable=True).step()
    flagged = _Set(kind, *MIXED, seed=5, capturable=True).amp(found_inf=0.0).step()
    assert _bits_equal(plain.read(), flagged.read())
    assert flagged.sentinels_intact()
    assert int(plain.count.item()) == int(flagged.count.item()) == plain.t


# ------------------------------------------------------------------------------ 5. and 7. a skipped step and bias correction
SKIP_SIZES, SKIP_VIEWS = [5, 8193, 0, 33], [False, True, True, False]


def _three_gradients():
    rng = np.random.default_rng(57)
    return [[rng.standard_normal(n).astype(np.float32) for n in SKIP_SIZES] for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _eager_three_steps():
    """Capturable Adam from count 0, found_inf = 0, 1, 0: (the set, [state after each step], [count after each step])."""
    s = _Set("adam", SKIP_SIZES, SKIP_VIEWS, seed=5, t=1, capturable=True).amp(found_inf=0.0)
    states, counts = [], []
    for grads, flag in zip(_three_gradients(), (0.0, 1.0, 0.0)):
        s.set_grads(grads)
        s.opt.found_inf.fill_(flag)
        s.step()
        states.append(s.read())
        counts.append(int(s.count.item()))
    return s, states, counts


def test_a_skipped_step_does_not_advance_the_bias_correction():
    s, states, counts = _eager_three_steps()
    grads = _three_gradients()
    assert counts == [1, 1, 2]
    first = [[init[0], g] + init[2:] for init, g in zip(s.init, grads[0])]
    assert _bits_equal([t[:1] + t[2:] for t in states[0]], [t[:1] + t[2:] for t in states[1]])      # the skip moved nothing
    # each counted step from the fp32 state it started at: t = 1 from the initial state, t = 2 from the state after step 1
    _check_against(s, states[0], first, t=1)
    second = [[st[0], g] + st[2:] for st, g in zip(states[1], grads[2])]
    _check_against(s, states[2], second, t=2)


def _check_against(s, got, start, t):
    for i, h in enumerate(s.hyper):
        ks = [k for k, g in enumerate(s.group) if g == i]
        cat = [np.concatenate([start[k][j] for k in ks]) for j in range(s.roles)]
        allowance, measured = _allowance("adam", cat, cat[1], t, h)
        for k in ks:
            p_ref, s_ref, scale, bars = _reference("adam", start[k], start[k][1].astype(np.float64), t, h)
            for j, (want, bar) in enumerate(zip(s_ref, bars)):
                assert np.all(np.abs(got[k][2 + j] - want) <= bar), (t, k, "state", j)
            assert np.all(np.abs(got[k][0] - p_ref) <= 2.0 ** -23 * np.abs(start[k][0]) + allowance * scale), (t, k, "p", measured)


def test_graph_replay_of_the_scaled_step_equals_the_eager_run():
    """opt.step() captured once with found_inf bound to a persistent device tensor, replayed three times while the gradient
    and the flag are rewritten in place (finite, skip, finite): bit-identical to the eager run above, count included. One
    stream, no parallel branches."""
    _, want_states, want_counts = _eager_three_steps()
    warm = _Set("adam", SKIP_SIZES, SKIP_VIEWS, seed=5, t=1, capturable=True).amp(found_inf=0.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # every op of the step has run once before the capture
        warm.opt.step()
    torch.cuda.current_stream().wait_stream(side)
    s = _Set("adam", SKIP_SIZES, SKIP_VIEWS, seed=5, t=1, capturable=True).amp(found_inf=0.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.opt.step()
    torch.cuda.synchronize()
    assert int(s.count.item()) == 0                               # the capture ran nothing
    for grads, flag, want, count in zip(_three_gradients(), (0.0, 1.0, 0.0), want_states, want_counts):
        s.set_grads(grads)
        s.opt.found_inf.fill_(flag)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(s.read(), want)
        assert int(s.count.item()) == count
    assert s.sentinels_intact()


# -------------------------------------------------------------------------------------------- 6. the real torch.amp.GradScaler
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_grad_scaler_steps_without_a_read_back(kind):
    """Three scaler.step / update calls on one 8193-element parameter, the middle one with an inf in the gradient: it changes
    nothing, the scale halves once, the count ends at 2. Snapshots are device copies; the test's one sync is at the end.
    The first group's hyper-parameters (no weight decay): the first step starts from zero state, where a state bar is 2^-22 of
    the new term alone, and a g' = g + wd p whose two terms cancel carries the rounding of the fp32 product wd p, many times
    that (numpy's own fp32 arithmetic on these inputs: 3.7 and 7.1 bars at one element of 8193). Weight decay under a scale is
    what the tests above step, from states that do not vanish."""
    from shacira_amd.optim import FusedAdam, FusedRMSprop
    rng = np.random.default_rng(6)
    n = 8193
    p0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    w = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    w[1][4097] = np.inf
    h = HYPER[0]
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    if kind == "adam":
        opt = FusedAdam([p], lr=h["lr"], betas=(B1, B2), eps=EPS, weight_decay=h["wd"], capturable=True)
        names = ("exp_avg", "exp_avg_sq")
    else:
        opt = FusedRMSprop([p], lr=h["lr"], alpha=ALPHA, eps=EPS, weight_decay=h["wd"], capturable=True)
        names = ("square_avg",)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    weights = [torch.from_numpy(x).to(DEV) for x in w]
    snaps = []
    for wk in weights:
        opt.zero_grad(set_to_none=True)
        loss = (p * wk).sum()                                     # d loss / d p = wk; the scaled loss leaves 65536 wk in .grad
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        snaps.append([p.detach().clone(), p.grad.clone()] + [opt.state[p][name].clone() for name in names]
                     + [opt.state[p]["step"].clone()])
    torch.cuda.synchronize()
    snaps = [[x.cpu().numpy() for x in snap] for snap in snaps]
    assert [int(snap[-1][0]) for snap in snaps] == [1, 1, 2]
    assert scaler.get_scale() == 32768.0
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")      # bound for the duration of step() only
    zeros = [np.zeros(n, np.float32)] * len(names)
    starts = [[p0, w[0]] + zeros, None, [snaps[1][0], w[2]] + snaps[1][2:2 + len(names)]]
    for j in range(len(names) + 1):                               # the middle step: p and state as after the first
        a, b = snaps[0][0 if j == 0 else 1 + j], snaps[1][0 if j == 0 else 1 + j]
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for step, t in ((0, 1), (2, 2)):
        start = starts[step]
        allowance, measured = _allowance(kind, start, start[1], t, h)
        p_ref, s_ref, scale, bars = _reference(kind, start, start[1].astype(np.float64), t, h)
        got = snaps[step]
        for j, (want, bar) in enumerate(zip(s_ref, bars)):
            assert np.all(np.abs(got[2 + j] - want) <= bar), (step, "state", j)
        assert np.all(np.abs(got[0] - p_ref) <= 2.0 ** -23 * np.abs(start[0]) + allowance * scale), (step, "p", measured)
        assert np.array_equal(got[1].view(np.int32), start[1].view(np.int32))    # .grad came back unscaled: 65536 is exact


# ----------------------------------------------------------------------------------------------------------------- 8. harness
FIT = dict(steps=60, rays=256, samples_per_ray=8, codebook_bitwidth=12, max_grid_res=64, num_lods=4, val_points=4096)


@functools.lru_cache(maxsize=None)
def _fit(amp, optimizer, steps=60):
    from shacira_amd import harness
    out = harness.fit_field_3d(torch.device(DEV), **{**FIT, "steps": steps}, amp=amp, optimizer=optimizer)
    return {k: v for k, v in out.items() if k != "nef"}


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
def test_fit_field_3d_under_amp_keeps_half_of_the_fp32_gain(optimizer):
    """Wiring, not quality (fp16 tables carry about three digits): the AMP run gains at least half of the PSNR its fp32
    counterpart gains over the untrained model, and every skipped step is a scale back-off (growth_interval = 2000 is never
    reached in 60 steps, so the scale only halves)."""
    untrained = _fit(False, optimizer, steps=0)["psnr"]
    fp32, amp = _fit(False, optimizer), _fit(True, optimizer)
    print(f"{optimizer}: untrained {untrained:.3f} dB, fp32 {fp32['psnr']:.3f} dB, amp {amp['psnr']:.3f} dB, "
          f"skipped {amp['skipped_steps']}, final scale {amp['final_scale']}")
    assert math.isfinite(amp["loss"]) and math.isfinite(amp["psnr"])
    assert amp["skipped_steps"] == math.log2(65536.0 / amp["final_scale"])
    assert fp32["psnr"] > untrained
    assert amp["psnr"] - untrained >= 0.5 * (fp32["psnr"] - untrained)
