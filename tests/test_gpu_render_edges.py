"""render.hip at its edges, against the fp64 restatement in oracle/render.py: volume integration over per-ray offsets with empty
packs, pack lengths around the 64-sample chunk, every channel count the kernels dispatch on, optical depths with a wall behind
thin samples, non-finite inputs; the 'ray' marcher and the dense ray tracer at ragged workgroup fills, levels 0 to 8, samples on
the cube faces and non-finite rays. Bars are those of tests/test_gpu_render.py (tests/render_ref.py holds them; a CPU test
there shows fp32 arithmetic can meet them). Ids, counts, boundaries and everything about empty packs are exact."""
import ctypes

import numpy as np
import pytest
import torch

import render_ref as rr
from oracle import render as orr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# pack lengths per ray count: around the chunk of 64, empties first / last / two in a row
LAYOUTS = {1: [129], 2: [0, 63], 3: [64, 1, 0], 5: [65, 0, 0, 128, 257], 9: [0, 1, 63, 0, 0, 64, 129, 65, 0]}
TAIL = 3      # rows behind the last offset: no pack covers them (the capped emit's padding)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _oracle(feats, tau, ps, g_ray, g_w):
    f64, t64 = torch.from_numpy(feats).double().requires_grad_(), torch.from_numpy(tau).double().reshape(-1, 1).requires_grad_()
    ray, w = orr.exponential_integration_packed(f64, t64, ps)
    ((ray * torch.from_numpy(g_ray).double()).sum() + (w[:, 0] * torch.from_numpy(g_w).double()).sum()).backward()
    return ray.detach().numpy(), w.detach().numpy()[:, 0], f64.grad.numpy(), t64.grad.numpy()[:, 0]


def _hip(dev, feats, tau, ps, g_ray, g_w):
    from shacira_amd import render
    fd, td = torch.from_numpy(feats).to(dev).requires_grad_(), torch.from_numpy(tau).to(dev).reshape(-1, 1).requires_grad_()
    ray, w = render.exponential_integration(fd, td, None, pack_start=torch.from_numpy(ps).to(dev))
    ((ray * torch.from_numpy(g_ray).to(dev)).sum() + (w[:, 0] * torch.from_numpy(g_w).to(dev)).sum()).backward()
    return ray.detach().cpu().numpy(), w.detach().cpu().numpy()[:, 0], fd.grad.cpu().numpy(), td.grad.cpu().numpy()[:, 0]


def _inputs(rng, S, R, C):
    return (rng.random((S, C)).astype(np.float32), rng.standard_normal((R, C)).astype(np.float32),
            rng.standard_normal(S).astype(np.float32))


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 16])
@pytest.mark.parametrize("R", sorted(LAYOUTS))
def test_integration_over_offsets_with_empty_packs(dev, R, C):
    """Forward and backward over `pack_start=` for every layout and channel count; an empty pack gives a ray row and a
    `sum_reduce` row of exact zeros, rows no pack covers get weight 0 and a zero gradient."""
    from shacira_amd import render
    rng = np.random.default_rng(1000 * R + C)
    lens = LAYOUTS[R]
    ps, S = _offsets(lens), sum(lens) + TAIL
    feats, g_ray, g_w = _inputs(rng, S, R, C)
    tau = (rng.random(S) ** 3 * 2.0).astype(np.float32)
    want, got = _oracle(feats, tau, ps, g_ray, g_w), _hip(dev, feats, tau, ps, g_ray, g_w)
    assert got[0].shape == (R, C) and got[1].shape == (S,)
    rr.assert_forward_close(got[0], got[1], want[0], want[1])
    rr.assert_backward_close(got[2], got[3], want[2], want[3], ps)
    empty = np.array(lens) == 0
    assert not got[0][empty].any() and got[0][~empty].all()
    covered = int(ps[-1])
    assert not got[1][covered:].any() and not got[2][covered:].any() and not got[3][covered:].any()
    if C in (1, 5, 16):
        xs = rng.standard_normal((S, C)).astype(np.float32)
        xd, psd = torch.from_numpy(xs).to(dev).requires_grad_(), torch.from_numpy(ps).to(dev)
        out = render.sum_reduce(xd, None, pack_start=psd)
        np.testing.assert_allclose(out.detach().cpu().numpy(), orr.sum_reduce_packed(torch.from_numpy(xs), ps).numpy(),
                                   rtol=1e-5, atol=1e-5)
        assert not out.detach().cpu().numpy()[empty].any()
        (out * torch.from_numpy(g_ray).to(dev)).sum().backward()
        g_x = np.zeros((S, C), np.float32)
        for r in range(R):
            g_x[ps[r]:ps[r + 1]] = g_ray[r]
        assert np.array_equal(xd.grad.cpu().numpy(), g_x)            # broadcast of the row; zero behind the last offset


def test_more_than_sixteen_channels_is_refused(dev):
    from shacira_amd import render
    feats, tau = torch.rand(10, 17, device=dev), torch.rand(10, 1, device=dev)
    ps = torch.tensor([0, 4, 10], device=dev)
    with pytest.raises(RuntimeError):
        render.exponential_integration(feats, tau, None, pack_start=ps)
    with pytest.raises(RuntimeError):
        render.sum_reduce(feats, None, pack_start=ps)
    ray, _ = render.exponential_integration(feats[:, :16].contiguous(), tau, None, pack_start=ps)     # 16 is served
    assert tuple(ray.shape) == (2, 16)


def _family_call(rng, C):
    """One call: every tau family as a pack of its own, ordinary packs (and empties) around and between them."""
    fam = rr.tau_families(rng)
    taus, names = [], []
    for name in "abcdefg":
        n = int(rng.choice([1, 63, 65, 129]))
        taus += [(rng.random(n) ** 3 * 2.0).astype(np.float32), fam[name]]
        names += ["-", name]
        if name in "cf":
            taus.append(np.zeros(0, np.float32))
            names.append("0")
    taus.append((rng.random(64) ** 3 * 2.0).astype(np.float32))
    names.append("-")
    ps = _offsets([t.shape[0] for t in taus])
    tau = np.concatenate(taus)
    feats, g_ray, g_w = _inputs(rng, tau.shape[0], len(taus), C)
    return names, ps, tau, feats, g_ray, g_w


@pytest.mark.parametrize("C", [3, 16])
def test_integration_on_the_tau_families(dev, C):
    """(a) rand^3 * 2, (b) log-uniform 1e-6 .. 1e3, (c) zeros with one 1.0 at sample 70, (d) 40 x 1e-3, 1e3, 20 x 1e-3, (e) 138 x
    1e-3 then 1e3, (f) 63 x 2e-4 then 2e4, (g) 100 x 3e-3 -- one pack each inside one call. No family had to be narrowed: the
    fp32 restatement of the backward stays under a tenth of the g_tau bar on (b), (d) and (f) (tests/test_oracle_render.py).
    Measured on the MI355X, in units of the bars: with the exclusive prefix formed as `incl - t` (the kernels before this test)
    the weights of (d) are 2.2 over, those of (f) 87 (the wall samples, 2e-5 and 9e-4 off), g_tau of (f) 160 to 330, of (e) 1.2 and
    of (b) 1.8e4 at C = 16; with the neighbour lane's prefix nothing is above 0.4."""
    rng = np.random.default_rng(50 + C)
    names, ps, tau, feats, g_ray, g_w = _family_call(rng, C)
    want, got = _oracle(feats, tau, ps, g_ray, g_w), _hip(dev, feats, tau, ps, g_ray, g_w)
    for r, name in enumerate(names):                   # the figures first, family by family
        b, e = int(ps[r]), int(ps[r + 1])
        if name not in "-0":
            rel = np.abs(got[1][b:e] - want[1][b:e]) / (1e-7 + 1e-5 * np.abs(want[1][b:e]))
            ray = np.abs(got[0][r] - want[0][r]) / (1e-6 + 1e-5 * np.abs(want[0][r]))
            gt = np.abs(got[3][b:e] - want[3][b:e]) / (2e-6 * np.abs(want[3][b:e]).max() + 1e-4 * np.abs(want[3][b:e]))
            print(f"family {name} C={C}: weights {rel.max():.3f} rays {ray.max():.3f} g_tau {gt.max():.3f} of the bar")
    rr.assert_forward_close(got[0], got[1], want[0], want[1])
    rr.assert_backward_close(got[2], got[3], want[2], want[3], ps)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_non_finite_tau_stays_inside_its_pack(dev, poison):
    """A NaN or +inf optical depth in one pack: every other pack's rays, weights and gradients are bit-identical to the run
    without it. +inf is a legitimate opaque sample: its weight is the transmittance that is left, everything behind it in
    the pack weighs 0 (no gradient is asserted for that pack)."""
    rng = np.random.default_rng(77)
    lens = [65, 130, 0, 64, 7]
    ps, S, C = _offsets(lens), sum(lens), 4
    feats, g_ray, g_w = _inputs(rng, S, len(lens), C)
    tau = (rng.random(S) ** 3 * 0.2).astype(np.float32)
    clean = _hip(dev, feats, tau, ps, g_ray, g_w)
    bad = tau.copy()
    at = int(ps[1]) + 70                                   # second chunk of pack 1
    bad[at] = poison
    dirty = _hip(dev, feats, bad, ps, g_ray, g_w)
    b, e = int(ps[1]), int(ps[2])
    others = np.r_[0:b, e:S]
    assert np.array_equal(np.delete(dirty[0], 1, 0), np.delete(clean[0], 1, 0))
    for k in (1, 2, 3):
        assert np.array_equal(dirty[k][others], clean[k][others]), k
    if np.isinf(poison):
        t64 = tau[b:e].astype(np.float64)
        T = np.exp(-np.concatenate([[0.0], np.cumsum(t64)[:-1]]))
        w = T * (1.0 - np.exp(-t64))
        w[70], w[71:] = T[70], 0.0
        np.testing.assert_allclose(dirty[1][b:e], w, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(dirty[0][1], (w[:, None] * feats[b:e].astype(np.float64)).sum(0), rtol=1e-5, atol=1e-6)
    else:
        assert np.isnan(dirty[0][1]).all() and np.isnan(dirty[1][at:e]).all() and np.isfinite(dirty[1][b:at]).all()


def test_backward_with_a_null_grad_weights(dev):
    """`shacira_pack_integrate_backward(..., grad_weights = NULL, ...)` equals the autograd path fed a zero g_w, bit for bit."""
    from shacira_amd import _lib
    rng = np.random.default_rng(5)
    lens = [0, 65, 1, 129, 0]
    ps, S, C = _offsets(lens), sum(lens), 5
    feats, g_ray, _ = _inputs(rng, S, len(lens), C)
    tau = (rng.random(S) ** 3 * 2.0).astype(np.float32)
    _, _, g_f, g_t = _hip(dev, feats, tau, ps, g_ray, np.zeros(S, np.float32))
    fd, td, psd, grd = (torch.from_numpy(a).to(dev) for a in (feats, tau, ps, g_ray))
    out_f, out_t = torch.zeros_like(fd), torch.zeros_like(td)
    rc = _lib.lib().shacira_pack_integrate_backward(S, len(lens), C, fd.data_ptr(), td.data_ptr(), psd.data_ptr(), grd.data_ptr(),
                                                    None, out_f.data_ptr(), out_t.data_ptr(),
                                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out_f.cpu().numpy(), g_f) and np.array_equal(out_t.cpu().numpy(), g_t) and g_t.any()


# ------------------------------------------------------------------------------------------------------------------ the marcher
def _rays(rng, n, aim=0.5):
    o = rng.standard_normal((n, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = (rng.random((n, 3)) - 0.5) * 2.0 * aim - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(o.astype(np.float32)), torch.from_numpy(d.astype(np.float32))


_occ_cache = {}


def _random_occupancy(level):
    if level not in _occ_cache:
        G = 1 << level
        occ = torch.from_numpy(np.random.default_rng(level).random((G, G, G), dtype=np.float32) < 0.3)
        if level == 0:
            occ[:] = True
        _occ_cache[level] = occ
    return _occ_cache[level]


_MARCH_LEVELS = [0, 1, 5, 8]


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("N", [1, 3, 5, 257])
def test_raymarch_ray_ragged_sizes_and_levels(dev, N, ns):
    """Ray counts that leave the last 4-ray workgroup partly filled, sample counts around the 64-lane chunk, levels 0 / 1 / 5 /
    8 in turn: compared with the reference's Python exactly as tests/test_gpu_render.py does."""
    from shacira_amd import render
    level = _MARCH_LEVELS[([1, 3, 5, 257].index(N) + [1, 63, 64, 65, 130].index(ns)) % 4]
    rng = np.random.default_rng(N * 1000 + ns)
    G = 1 << level
    o, d = _rays(rng, N)
    occ = _random_occupancy(level)
    jit = torch.from_numpy(rng.random((N, ns)).astype(np.float32))
    near, far = 1.5, 4.5
    full = torch.ones((G, G, G), dtype=torch.bool)
    r_all, s_all, dep_all, del_all, b_all, off_all = [t.cpu() for t in render.raymarch_ray(
        o.to(dev), d.to(dev), near, far, full.to(dev), level, ns, jit.to(dev))]
    ro, so, do, dlo, bo = orr.raymarch_ray(o, d, near, far, full, level, ns, jit)
    assert torch.equal(r_all, ro)
    assert torch.equal(off_all[1:] - off_all[:-1], torch.bincount(r_all, minlength=N)) and off_all[0] == 0
    assert bool((s_all.abs() <= 1.0).all())
    np.testing.assert_allclose(dep_all.numpy(), do.numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(del_all.numpy(), dlo.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(s_all.numpy(), so.numpy(), rtol=1e-5, atol=1e-6)
    assert torch.equal(b_all, bo)
    r, s, dep, dl, b, off = [t.cpu() for t in render.raymarch_ray(o.to(dev), d.to(dev), near, far, occ.to(dev), level, ns,
                                                                  jit.to(dev))]
    assert torch.equal(off[1:] - off[:-1], torch.bincount(r, minlength=N))
    keep = orr.query_dense(occ, s_all, level)
    assert torch.equal(r, r_all[keep]) and torch.equal(b, orr.mark_pack_boundaries(r))
    assert torch.equal(s, s_all[keep]) and torch.equal(dep, dep_all[keep]) and torch.equal(dl, del_all[keep])
    none = render.raymarch_ray(o.to(dev), d.to(dev), near, far, torch.zeros_like(full).to(dev), level, ns, jit.to(dev))
    assert none[0].numel() == 0 and none[4].numel() == 0 and not none[5].any()


def test_raymarch_ray_non_finite_rays_emit_nothing(dev):
    """`quantize_axis` answers -1 unless 0 <= floor(G (x + 1) / 2) < G, and every comparison with a NaN is false while +-inf
    fails one side: a sample of a ray with a NaN or infinite origin or direction has no cell. Such rays get empty packs and the
    rays around them keep exactly the rows they have without them."""
    from shacira_amd import render
    rng = np.random.default_rng(21)
    level, ns, N = 5, 65, 9
    o, d = _rays(rng, N)
    bad = {1: ("o", float("nan")), 3: ("o", float("inf")), 4: ("d", float("nan")), 6: ("d", float("-inf")), 8: ("o", float("-inf"))}
    ob, db = o.clone(), d.clone()
    for r, (which, val) in bad.items():
        (ob if which == "o" else db)[r, r % 3] = val
    occ = torch.ones((32, 32, 32), dtype=torch.bool)
    jit = torch.from_numpy(rng.random((N, ns)).astype(np.float32))
    good = [r for r in range(N) if r not in bad]
    ref = [t.cpu() for t in render.raymarch_ray(o[good].to(dev), d[good].to(dev), 1.5, 4.5, occ.to(dev), level, ns,
                                                jit[good].to(dev))]
    got = [t.cpu() for t in render.raymarch_ray(ob.to(dev), db.to(dev), 1.5, 4.5, occ.to(dev), level, ns, jit.to(dev))]
    counts = got[5][1:] - got[5][:-1]
    assert not counts[list(bad)].any() and counts[good].all()
    assert torch.equal(got[0], torch.tensor(good)[ref[0]])
    for k in (1, 2, 3, 4):
        assert torch.equal(got[k], ref[k]), k
    ro = orr.raymarch_ray(ob, db, 1.5, 4.5, occ, level, ns, jit)[0]
    assert torch.equal(got[0], ro)


def test_raymarch_ray_samples_on_the_cube_faces(dev):
    """Axis-aligned rays, no jitter, near = 1, far = 3, five samples from x = -2 (or +2): the linspace nodes land on x = -1, -0.5,
    0, 0.5, 1 exactly. x = -1.0 lies in cell 0, x = 1.0 in no cell (floor(G * 2 / 2) = G is out of range)."""
    from shacira_amd import render
    level, ns = 2, 5
    o = torch.tensor([[-2.0, 0.1, 0.2], [2.0, 0.1, 0.2]])
    d = torch.tensor([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    jit = torch.zeros(2, ns)
    full = torch.ones(4, 4, 4, dtype=torch.bool)
    r, s, dep, dl, b, off = [t.cpu() for t in render.raymarch_ray(o.to(dev), d.to(dev), 1.0, 3.0, full.to(dev), level, ns,
                                                                  jit.to(dev))]
    assert off.tolist() == [0, 4, 8] and r.tolist() == [0] * 4 + [1] * 4
    assert s[:, 0].tolist() == [-1.0, -0.5, 0.0, 0.5, 0.5, 0.0, -0.5, -1.0]
    assert dep[:, 0].tolist() == [1.0, 1.5, 2.0, 2.5, 1.5, 2.0, 2.5, 3.0]
    assert dl[:, 0].tolist() == [0.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5] and b.tolist() == [True, False, False, False] * 2
    ro, so, do, dlo, bo = orr.raymarch_ray(o, d, 1.0, 3.0, full, level, ns, jit)
    assert torch.equal(r, ro) and torch.equal(s, so) and torch.equal(b, bo)
    only0 = torch.zeros_like(full)
    only0[0, 2, 2] = True                                  # y = 0.1, z = 0.2 -> cells 2, 2; x = -1.0 -> cell 0
    r, s, *_ = [t.cpu() for t in render.raymarch_ray(o.to(dev), d.to(dev), 1.0, 3.0, only0.to(dev), level, ns, jit.to(dev))]
    assert r.tolist() == [0, 1] and s[:, 0].tolist() == [-1.0, -1.0]
    last = torch.zeros_like(full)
    last[3, 2, 2] = True                                   # the cell under the +1 face holds x = 0.5, never x = 1.0
    r, s, *_ = [t.cpu() for t in render.raymarch_ray(o.to(dev), d.to(dev), 1.0, 3.0, last.to(dev), level, ns, jit.to(dev))]
    assert r.tolist() == [0, 1] and s[:, 0].tolist() == [0.5, 0.5]


@pytest.mark.parametrize("cap", [0, 1])
def test_capped_emit_with_room_for_nothing_or_one(dev, cap):
    from shacira_amd import render
    rng = np.random.default_rng(31)
    N, level, ns = 5, 3, 65
    o, d = _rays(rng, N)
    occ = torch.ones((8, 8, 8), dtype=torch.bool).to(dev)
    jit = torch.from_numpy(rng.random((N, ns)).astype(np.float32)).to(dev)
    args = (o.to(dev), d.to(dev), 1.5, 4.5, occ, level, ns, jit)
    r, s, dep, dl, b, off = render.raymarch_ray(*args)
    rc, sc, depc, dlc, bc, offc, total = render.raymarch_ray(*args, capacity=cap)
    assert int(total) == r.shape[0] > 1 and rc.shape[0] == cap and tuple(sc.shape) == (cap, 3)
    assert torch.equal(rc, r[:cap]) and torch.equal(sc, s[:cap]) and torch.equal(depc, dep[:cap])
    assert torch.equal(dlc, dl[:cap]) and torch.equal(bc, b[:cap]) and torch.equal(offc, off.clamp(max=cap))
    feats = torch.rand(cap, 3, device=dev, requires_grad=True)            # and the clamped offsets integrate
    ray, w = render.exponential_integration(feats, torch.rand(cap, 1, device=dev), None, pack_start=offc)
    assert tuple(ray.shape) == (N, 3) and int((ray != 0).any(dim=1).sum()) == cap


# --------------------------------------------------------------------------------------------------------------- the ray tracer
_AXIS_OFFSETS = (0.3, -0.2, 0.1)      # where the axis-aligned special rays cross the other two axes


def _cell(x, G):
    return int(np.floor((x + 1.0) * 0.5 * G))


def _trace_occupancy(level):
    """The cells of the main diagonal are always occupied. Levels up to 3: the rest random, 40% full. Level 8: the cell
    lines the axis-aligned and the in-plane special rays run along plus a 40% full block of 16^3 cells at the centre -- few
    enough cells for the brute-force oracle, which tests every ray against every occupied cell."""
    G = 1 << level
    rng = np.random.default_rng(40 + level)
    i = torch.arange(G)
    if level < 8:
        occ = torch.from_numpy(rng.random((G, G, G)) < 0.4)
        occ[i, i, i] = True
        return occ
    occ = torch.zeros((G, G, G), dtype=torch.bool)
    occ[i, i, i] = True
    cx, cy, cz = (_cell(v, G) for v in _AXIS_OFFSETS)
    occ[:, cy, cz] = occ[cx, :, cz] = occ[cx, cy, :] = True
    occ[_cell(0.0, G), :, _cell(0.3, G)] = True
    lo = G // 2 - 8
    occ[lo:lo + 16, lo:lo + 16, lo:lo + 16] |= torch.from_numpy(rng.random((16, 16, 16)) < 0.4)
    return occ


def _special_rays():
    s3 = 3.0 ** -0.5
    rays = [((-2.0, -2.0, -2.0), (s3, s3, s3))]                                     # the full diagonal: 3 G cell steps
    for a in range(3):                                                               # along each axis, both ways
        for sign in (1.0, -1.0):
            o, d = list(_AXIS_OFFSETS), [0.0, 0.0, 0.0]
            o[a], d[a] = -3.0 * sign, sign
            rays.append((tuple(o), tuple(d)))
    rays.append(((0.0, -3.0, 0.3), (0.0, 1.0, 0.0)))                                 # inside a cell-boundary plane
    rays.append(((-1.0, 0.3, 0.2), (0.9701425, 0.19402850, 0.14552138)))             # starts on a face of the cube
    rays.append(((0.0, 0.0, 0.0), (0.30151134, 0.90453403, -0.30151134)))            # starts inside, on a cell corner
    return rays


def _trace_rays(N, level, seed):
    """N rays towards the cube, the special ones first (tests/golden/make_grid_walk.py records the same rays)."""
    rng = np.random.default_rng(seed)
    o, d = _rays(rng, N)
    if level == 8:                                       # every sixth ray aims at the occupied block in the centre
        ob, db = _rays(rng, N, aim=1.0 / 16)
        o[::6], d[::6] = ob[::6], db[::6]
    for k, (so, sd) in enumerate(_special_rays()[:N]):
        o[k], d[k] = torch.tensor(so), torch.tensor(sd)
    return o, d


@pytest.mark.parametrize("N,level,seed", [(1, 0, 300), (1, 8, 300), (255, 1, 300), (256, 3, 300), (257, 8, 303), (600, 3, 300),
                                          (600, 0, 300)])
def test_raytrace_dense_ragged_sizes_levels_and_special_rays(dev, N, level, seed):
    """One workgroup partly filled, exactly filled, one ray over, and three workgroups; levels 0 / 1 / 3 / 8. The first rays
    are the special ones (`_special_rays`); the diagonal at level 8 takes 3 * 256 steps of the 3 G + 3 the walk allows and
    must report all 256 cells. Compared with the brute-force slab test, grazing contacts (< 1e-4) dropped on both sides; the
    seeds are ones for which no contact of the oracle is within 2e-5 of that length -- the absolute term of the depth bar; the
    walk adds a cell's length to its exit depth at every step, and after 128 steps at level 8 an interval's length is up to
    1.2e-5 off -- so the rule cannot split the two sides."""
    from shacira_amd import _lib, render
    o, d = _trace_rays(N, level, seed)
    occ = _trace_occupancy(level)
    ridx, pidx, depth = [t.cpu() for t in render.raytrace_dense(o.to(dev), d.to(dev), occ.to(dev), level)]
    # the count pass agrees with the emit pass
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    od, dd, occd = o.to(dev), d.to(dev), occ.to(torch.uint8).to(dev)
    assert _lib.lib().shacira_raytrace_dense_count(N, od.data_ptr(), dd.data_ptr(), occd.data_ptr(), level, counts.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    assert int(counts.sum()) == ridx.shape[0] and torch.equal(counts.cpu().long(), torch.bincount(ridx.long(), minlength=N))
    # depth order within a ray
    same = ridx[1:] == ridx[:-1]
    assert bool((ridx[1:] >= ridx[:-1]).all()) and bool((depth[1:, 0][same] >= depth[:-1, 0][same]).all())
    assert bool((depth[:, 1] >= depth[:, 0]).all()) and bool((depth[:, 0] >= 0).all())
    ro, co, do = orr.raytrace_dense(o, d, occ, level)
    keep, keep_o = (depth[:, 1] - depth[:, 0]) > 1e-4, (do[:, 1] - do[:, 0]) > 1e-4
    assert not (((do[:, 1] - do[:, 0]) - 1e-4).abs() < 2e-5).any(), "test input: a contact sits on the grazing threshold"
    ridx, pidx, depth = ridx[keep], pidx[keep], depth[keep]
    ro, co, do = ro[keep_o], co[keep_o], do[keep_o]
    assert torch.equal(ridx.long(), ro)
    morton = torch.zeros(co.shape[0], dtype=torch.long)
    for b in range(level):
        morton |= (((co[:, 0] >> b) & 1) << (3 * b + 2)) | (((co[:, 1] >> b) & 1) << (3 * b + 1)) \
            | (((co[:, 2] >> b) & 1) << (3 * b))
    assert torch.equal(pidx.long(), morton)
    np.testing.assert_allclose(depth.numpy(), do.numpy(), rtol=1e-4, atol=2e-5)
    assert int((ridx == 0).sum()) >= (1 << level)                     # the diagonal met every cell on its way
    if level == 8 and N >= 8:                                         # the six axis rays and the in-plane ray: whole lines
        assert [int((ridx == k).sum()) for k in range(1, 8)] == [256] * 7
