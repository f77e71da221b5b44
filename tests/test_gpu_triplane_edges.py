"""The triplane kernels (triplane.hip) and the block counting sort under them (block_sort.h) at their coordinate, shape and
sort edges, against the fp64 restatement (tests/triplane_ref.py, fp32 index math: the kernels' weights exactly).

Coordinates come from tests/grid_edge_cases.py: texel lines of every LOD of the call out to k in [-3R, 4R] with their fp32
neighbours, +-1, +-(1 - 2^-24), zeros, denormals, far values up to 1e6, uniform draws in +-8, NaN, +-inf and 3e38, mixed per
axis within a sample. Magnitudes with floorf(index / span) >= 2^24 are left out: the parity of the kernel's (int) cast is
not defined there (3e38 is therefore used only where every LOD of the call has R >= 4, where its index overflows to inf).
Each batch is proven, from the restatement alone, to hold at least 100 samples with flips >= 2, 100 with a negative
unnormalised index and an odd flip, 100 with an in-bounds corner of weight exactly 0 and 32 whose reflected index is
exactly 0 or R; a batch smaller than 1537 samples is the head of a 1537-sample batch that is, and from 511 samples on the
head itself holds these minima scaled by N / 1537.

Bounds (eps = fp32 epsilon, u = 2^-24, L = LODs of the call), on every sample and every texel:
  forward        |got - ref| <= 4 L eps sum|w v|; both ``triplane_layout`` values, bitwise equal to each other
  plane gradient |got - ref| <= 1.01 (count + 1) u A + (count + 1) 2^-126 per texel, with count the in-bounds corner
                 contributions of the texel and A = sum |w g| (``triplane_ref.backward_scale``): fp32 summation in any
                 order of count once-rounded products is off by at most count u A to first order, 1.01 covers the second
                 order while count u <= 0.02 (asserted), and the last term allows float atomics that flush denormal partial
                 sums. got == 0 exactly where A == 0. The level-maximum bar of test_gpu_triplane.py holds as well.
  coordinates    64 eps gscale + 1e-6; exactly 0 on every axis whose d(index)/d(coord) is 0 at every LOD; same bits twice
The worst error / bound ratio of each case is printed (pytest -s): profiles/triplane.md records them.
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_edge_cases as ge
import triplane_ref as tr

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
U = 2.0 ** -24
TINY = 2.0 ** -126

SHAPES = [(f, lods, n) for f, lods, sizes in ge.TRIPLANE_CASES for n in sizes]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _planes(fdim, lods, seed, dev):
    """per LOD [fmx, fmy, fmz] as fp32 numpy [F, S, S], and the same as the operator's NCHW device tensors."""
    gen = torch.Generator(device=dev).manual_seed(seed)         # drawn on the device: the LOD-10 planes are 63 M values
    planes = [torch.randn((1, fdim, (1 << l) + 1, (1 << l) + 1), generator=gen, device=dev) for l in lods for _ in range(3)]
    return [[planes[3 * l + p][0].cpu().numpy() for p in range(3)] for l in range(len(lods))], planes


def _edge_batch(lods, n):
    full = ge.triplane_coords(lods, n, 1000 + n)
    ge.assert_triplane_reach(full, lods, n)
    return np.ascontiguousarray(full[:n])


def _grad_output(fdim, lods, n, summed, seed):
    return np.random.default_rng(seed).standard_normal((n, 3 * fdim * (1 if summed else len(lods))), dtype=np.float32)


def _check_planes(grads, gref, scale, lods, tag):
    """every texel of every plane against the per-texel bound; -> (worst error / bound, the denormal term was needed).
    Texels that no corner touches (count == 0) are compared on the device: exactly zero, every one of them; the touched
    ones, a small set, are gathered and compared in fp64 on the host."""
    worst, denormal = 0.0, False
    for l in range(len(lods)):
        for p in range(3):
            g = grads[3 * l + p][0]
            want_all = gref[l][p]
            count_all, asum_all = scale[l][p]
            assert tuple(g.shape) == want_all.shape and float(count_all.max(initial=0)) * U <= 0.02
            touched = count_all > 0
            ys, xs = np.nonzero(touched)
            stray = ((g != 0) | torch.isnan(g)).any(0) & ~torch.from_numpy(touched).to(g.device)
            assert not bool(stray.any()), (tag, l, p, "a texel nothing contributes to is not zero")
            ty, tx = torch.from_numpy(ys).to(g.device), torch.from_numpy(xs).to(g.device)
            got = g[:, ty, tx].cpu().numpy().astype(np.float64)                  # [F, touched texels]
            want, asum, count = want_all[:, ys, xs], asum_all[:, ys, xs], count_all[ys, xs]
            assert not np.isnan(got).any(), (tag, l, p)
            rounding = 1.01 * (count + 1)[None] * U * asum
            bound = rounding + (count + 1)[None] * TINY
            err = np.abs(got - want)
            worst = max(worst, float((err / bound).max(initial=0)))
            denormal |= bool((err > rounding).any())
            assert np.all(got[asum == 0] == 0), (tag, l, p, "a texel with only zero contributions is not zero")
            bad = err > bound
            assert not bad.any(), (tag, l, p, int(bad.sum()), float((err / bound).max()))
            level_max = float(np.abs(want).max(initial=0))                       # untouched texels: error exactly 0
            assert float(err.max(initial=0)) <= 1e-5 * max(level_max, 1e-30), (tag, l, p)
    return worst, denormal


@pytest.mark.parametrize("summed", [True, False], ids=["sum", "cat"])
@pytest.mark.parametrize("fdim,lods,n", SHAPES)
def test_forward_on_edge_coordinates_in_both_layouts(dev, fdim, lods, n, summed):
    from shacira_amd import _lib, hip_ops
    from shacira_amd.wisp.ops.triplane import triplane_torch
    host, planes = _planes(fdim, lods, fdim * 1000 + n, dev)
    cn = _edge_batch(lods, n)
    coords = torch.from_numpy(cn).to(dev)
    outs = []
    for layout in (0, 1):
        _lib.set_option("triplane_layout", layout)
        try:
            outs.append(hip_ops.triplane_forward(coords, lods, planes, summed))
        finally:
            _lib.set_option("triplane_layout", -1)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref = tr.forward(cn, host, summed, index_dtype=np.float32)
    scale = tr.abs_forward(cn, host, summed, index_dtype=np.float32)
    for got in outs:
        g = got.cpu().double().numpy()
        assert not np.isnan(g).any()
        err = np.abs(g - ref)
        print(f"forward F={fdim} lods={list(lods)} N={n}: worst {float((err / np.maximum(scale, 1e-30)).max() / EPS):.2f} "
              f"eps sum|w v| (bound {4 * len(lods)})")
        assert np.all(err <= 4 * len(lods) * EPS * scale + 1e-30)
    want = triplane_torch(coords, planes, len(lods), summed)
    assert torch.allclose(outs[1], want, rtol=0, atol=1e-4, equal_nan=True)


@pytest.mark.parametrize("summed", [True, False], ids=["sum", "cat"])
@pytest.mark.parametrize("fdim,lods,n", SHAPES)
def test_gradients_on_edge_coordinates_per_texel(dev, fdim, lods, n, summed):
    from shacira_amd import hip_ops
    host, planes = _planes(fdim, lods, fdim * 1000 + n, dev)
    cn = _edge_batch(lods, n)
    coords = torch.from_numpy(cn).to(dev)
    go = _grad_output(fdim, lods, n, summed, 7 + n)
    gt = torch.from_numpy(go).to(dev)
    grads, gc = hip_ops.triplane_backward(coords, lods, fdim, gt, summed, planes=planes, need_coords=True)
    gref, gcref, gscale = tr.backward(cn, host, go, summed, index_dtype=np.float32)
    sides = [(1 << l) + 1 for l in lods]
    scale = tr.backward_scale(cn, sides, fdim, go, summed, index_dtype=np.float32)
    tag = (fdim, lods, n, summed)
    worst, denormal = _check_planes(grads, gref, scale, lods, tag)
    print(f"plane gradient F={fdim} lods={list(lods)} N={n} {'sum' if summed else 'cat'}: worst error / bound "
          f"{worst:.3f}; denormal term needed: {denormal}")
    # coordinate gradient
    g = gc.cpu().double().numpy()
    assert not np.isnan(g).any()
    dead = np.ones((n, 3), dtype=bool)
    for S in sides:
        dead &= tr.coord_mult(cn, S, np.float32) == 0
    assert n < ge.MIN_BATCH or int(dead.sum()) >= 32
    assert np.all(g[dead] == 0), "an axis clipped at a border at every LOD has a non-zero gradient"
    err = np.abs(g - gcref)
    assert np.all(err <= 64 * EPS * gscale + 1e-6), float((err - 64 * EPS * gscale).max())
    _, gc2 = hip_ops.triplane_backward(coords, lods, fdim, gt, summed, planes=planes, need_planes=False, need_coords=True)
    assert torch.equal(gc.view(torch.int32), gc2.view(torch.int32))


SKEW_N = 1537
EDGE = 1.0 - 2.0 ** -10      # inside the texel cell next to the border at every LOD <= 10: the first / last sort block


def _skew_batch(kind):
    c = np.empty((SKEW_N, 3), dtype=np.float32)
    if kind == "interior":
        c[:] = [0.3137, -0.7071, 0.1234]
    elif kind == "lattice":
        c[:] = [-0.5, 0.25, 0.75]          # on a texel line of every LOD >= 3, on every axis
    elif kind == "corner":
        c[:] = [1.0, 1.0, 1.0]
    else:
        c[:SKEW_N // 2] = -EDGE
        c[SKEW_N // 2:] = EDGE
    return c


@pytest.mark.parametrize("kind", ["interior", "lattice", "corner", "halves"])
@pytest.mark.parametrize("fdim,lods", [(4, (5, 6, 7, 8)), (8, (3, 9))])
def test_skewed_batches_through_the_sort(dev, fdim, lods, kind):
    """Every sample in one sort block (many units of one bin, every other bin empty), or only the first and the last bin."""
    from shacira_amd import hip_ops
    cn = _skew_batch(kind)
    sides = [(1 << l) + 1 for l in lods]
    host = [[np.zeros((fdim, S, S), dtype=np.float32)] * 3 for S in sides]      # the plane gradient reads no plane
    perm = np.random.default_rng(3).permutation(SKEW_N)
    for summed in (True, False):
        go = _grad_output(fdim, lods, SKEW_N, summed, 11)
        gref, _, _ = tr.backward(cn, host, go, summed, index_dtype=np.float32)
        scale = tr.backward_scale(cn, sides, fdim, go, summed, index_dtype=np.float32)
        for l in range(len(lods)):
            for p in range(3):
                texels = int((scale[l][p][1].max(0) > 0).sum())
                assert 1 <= texels <= (8 if kind == "halves" else 4), (l, p, texels)
        for order in (np.arange(SKEW_N), perm):
            coords = torch.from_numpy(np.ascontiguousarray(cn[order])).to(dev)
            gt = torch.from_numpy(np.ascontiguousarray(go[order])).to(dev)
            grads, _ = hip_ops.triplane_backward(coords, lods, fdim, gt, summed)
            worst, denormal = _check_planes(grads, gref, scale, lods, (fdim, lods, kind, summed))
            print(f"skew {kind} F={fdim} lods={list(lods)} {'sum' if summed else 'cat'}: worst error / bound {worst:.3f}; "
                  f"denormal term needed: {denormal}")


@pytest.mark.parametrize("fdim,lods,n", [(4, (5, 6, 7, 8), (1 << 14) + 3), (8, (3, 9), 20011)])
def test_backward_in_a_stale_workspace_of_exactly_the_queried_size(dev, fdim, lods, n):
    """Through the C ABI: the workspace holds 0xFF in every byte, is exactly as long as the query says and has 4096 guard
    bytes behind it; the gradients (prefilled, too) are within the bound and the guard is untouched."""
    from shacira_amd import _lib
    L = _lib.lib()
    cn = _edge_batch(lods, n)
    coords = torch.from_numpy(cn).to(dev)
    go = _grad_output(fdim, lods, n, True, 5)
    gt = torch.from_numpy(go).to(dev)
    la = (ctypes.c_int32 * len(lods))(*lods)
    need = int(L.shacira_triplane_backward_workspace_bytes(n, len(lods), la, fdim, 1, _lib.TRIPLANE_GRAD_PLANES))
    assert need >= 4 * n
    buf = torch.empty(need + 4096, dtype=torch.uint8, device=dev)
    buf[:need] = 0xFF
    buf[need:] = 0x5A
    sides = [(1 << l) + 1 for l in lods]
    grads = [torch.full((1, fdim, S, S), 7.0, device=dev) for S in sides for _ in range(3)]
    ptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    rc = L.shacira_triplane_backward(n, len(lods), la, fdim, ctypes.c_void_p(coords.data_ptr()), None,
                                     ctypes.c_void_p(gt.data_ptr()), 1, _lib.TRIPLANE_GRAD_PLANES, ptrs, None,
                                     ctypes.c_void_p(buf.data_ptr()), need,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[need:] == 0x5A).all()), "the backward wrote behind its workspace"
    host = [[np.zeros((fdim, S, S), dtype=np.float32)] * 3 for S in sides]
    gref, _, _ = tr.backward(cn, host, go, True, index_dtype=np.float32)
    scale = tr.backward_scale(cn, sides, fdim, go, True, index_dtype=np.float32)
    worst, _ = _check_planes(grads, gref, scale, lods, (fdim, lods, n, "workspace"))
    print(f"stale exact workspace F={fdim} lods={list(lods)} N={n}: {need} bytes, worst error / bound {worst:.3f}")
