"""The octree kernels (octree.hip) and the block counting sort under them (block_sort.h) at their coordinate, level,
occupancy and sort edges, against the fp64 restatement (tests/octree_ref.py).

Coordinates come from tests/grid_edge_cases.py: the cell faces c = -1 + 2k/G of every level of the call with their fp32
neighbours, -1 (inside, t = 0), the first fp32 value below -1 (outside; -1 - 2^-24 itself is no fp32 number), 1 - 2^-24
(c + 1 rounds to 2: outside), zeros, denormals, +-1.3, 3e38, NaN and +-inf -- each proven by ``octree_ref.locate`` to land
where this says before a kernel runs. The N = 1537 batch of every case holds every one of these values, one per row with
the other two axes inside an occupied cell (asserted on the coordinates that go to the device); shorter batches hold an
evenly spaced part. The rest mixes them per axis with draws inside the cube and samples inside occupied cells (on their
faces, too), so that a single occupied cell is hit.

Bounds (eps = fp32 epsilon, u = 2^-24, L = levels of the call), on every sample and every table entry:
  forward         (16 + L) eps sum|w||v|, exact zeros where no level is occupied (test_gpu_octree.py)
  table gradient  |got - ref| <= 1.01 (count + 1) u A + (count + 1) 2^-126 per entry, count = the corner contributions of
                  the row and A = sum |w g| (``octree_ref.backward_scale``); the reference sums in fp64 the products of the
                  kernel's own fp32 weights (``weight_dtype=np.float32``: 1 - t and the x, y, z product rounded to fp32),
                  which is what the bound's "count once-rounded products" presumes. got == 0 exactly where A == 0 and on
                  the padding row. The level-maximum bar of test_gpu_octree.py holds as well. Because this reference
                  repeats the kernel's weight arithmetic, it does not by itself catch a wrong weight formula: the forward
                  check above, whose weights are fp64 products of t and 1 - t, does, and must stay.
  coordinates     (8 F L + 8) eps gscale + 1e-6, the same bits on a second run
Level 10 is not run here: its index bit grids take about 400 MB.
"""
import ctypes

import numpy as np
import pytest
import torch

import grid_edge_cases as ge
import octree_ref as oref

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
U = 2.0 ** -24
TINY = 2.0 ** -126

PARAMS = [(lv, f, occ) for lv, f, occs in ge.OCTREE_CASES for occ in occs]
BATCHES = (1, 511, 512, 513, 1537, "one cell", "halves")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_INDEX = {}


def _cells(occ, level):
    G = 1 << level
    if occ == "dense":
        return oref._all_cells(level)
    if occ == "shell":
        return oref.shell_cells(level)
    return np.full((1, 3), G - 1 if occ == "far" else 0, dtype=np.int64)


def _index(occ, levels):
    """(index, occupied cells of the finest level); dense and shell come from test_gpu_octree.py's cache of built indices."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.ops.octree import build_octree_index
    from test_gpu_octree import _index as shared_index
    key = (occ, tuple(levels))
    if key not in _INDEX:
        fine = max(levels)
        cells = _cells(occ, fine)
        if occ in ("dense", "shell"):
            _INDEX[key] = (shared_index(occ, sorted(set(levels))), cells)
        else:
            blas = OctreeAS.from_quantized_points(torch.from_numpy(cells), fine)
            _INDEX[key] = (build_octree_index(blas, sorted(set(levels))), cells)
    return _INDEX[key]


def _batch(kind, levels, cells, seed):
    if isinstance(kind, int):
        return ge.octree_coords(levels, cells, kind, seed)
    rng = np.random.default_rng(seed)
    G = 1 << max(levels)
    n = 1537
    u = rng.uniform(0, 1, (n, 3))
    u[rng.integers(0, 4, (n, 3)) == 0] = 0.0                       # on the cell's lower faces: t = 0, still inside
    if kind == "one cell":
        cell = np.broadcast_to(cells[len(cells) // 2], (n, 3))
    else:
        # The first and the last occupied cell in the sort's block order (x slowest, z fastest: the lexicographic order of
        # the cells), so that only the first and the last populated bin hold samples and both halves hit. A single occupied
        # cell would make that one bin: there the cube's two corner cells are taken, one of which is the occupied one.
        order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
        lo, hi = (cells[order[0]], cells[order[-1]]) if len(cells) > 1 else (np.zeros(3, np.int64), np.full(3, G - 1))
        cell = np.where(np.arange(n)[:, None] < n // 2, lo[None], hi[None])
    c = (-1.0 + 2.0 * (cell + u) / G).astype(np.float32)
    return np.where(c >= 1, np.nextafter(np.float32(1), np.float32(0)), c).astype(np.float32)


def _check_tables(grads, ref, scale, levels, tag):
    worst, denormal = 0.0, False
    for l in range(len(levels)):
        got = grads[l].cpu().numpy().astype(np.float64)
        want = ref[l]
        count, asum = scale[l]
        assert got.shape == want.shape and not np.isnan(got).any(), (tag, l)
        assert float(count.max(initial=0)) * U <= 0.02
        assert np.all(got[-1] == 0) and count[-1] == 0, (tag, l, "the padding row")
        rounding = 1.01 * (count + 1)[:, None] * U * asum
        bound = rounding + (count + 1)[:, None] * TINY
        err = np.abs(got - want)
        worst = max(worst, float((err / bound).max()))
        denormal |= bool((err > rounding).any())
        assert np.all(got[asum == 0] == 0), (tag, l, "an entry nothing contributes to is not zero")
        bad = err > bound
        assert not bad.any(), (tag, l, int(bad.sum()), float((err / bound).max()))
        assert float(err.max()) <= 1e-5 * float(np.abs(want).max()), (tag, l)
    return worst, denormal


def _np_index(index, levels):
    """(level_points per level, their keys sorted once for the batch loop; trinkets per level)."""
    return ([oref.SortedCells(index[l].level_points.cpu().numpy(), l) for l in levels],
            [index[l].trinkets.cpu().numpy() for l in levels])


def _tables(index, levels, fdim, seed, dev):
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal((index[l].rows + 1, fdim), dtype=np.float32) for l in levels]
    return host, [torch.from_numpy(t).to(dev) for t in host]


def test_special_values_land_where_the_suite_says():
    ge.assert_octree_landing(sorted({l for lv, _, _ in ge.OCTREE_CASES for l in lv}))


@pytest.mark.parametrize("levels,fdim,occ", PARAMS)
def test_forward_and_gradients_on_edge_coordinates(dev, levels, fdim, occ):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.ops.octree import octree_torch
    levels = list(levels)
    ge.assert_octree_landing(levels)
    index, cells = _index(occ, levels)
    li = [index[l].to(dev) for l in levels]
    lp, trk = _np_index(index, levels)
    host, tables = _tables(index, levels, fdim, fdim + len(cells), dev)
    L = len(levels)
    K = 8 * fdim * L + 8
    worst_f = worst_t = worst_c = 0.0
    denormal = False
    for b, kind in enumerate(BATCHES):
        cn = _batch(kind, levels, cells, 100 + b)
        n = cn.shape[0]
        coords = torch.from_numpy(cn).to(dev)
        hits = int(oref.hit_any(cn, levels, lp).sum())
        assert n < 511 or hits >= n // 8, (kind, hits)             # the batch reaches occupied cells
        if kind == 1537:                                           # ... and holds every special value of the suite
            ge.assert_octree_pool_present(cn, levels)
        for summed in (True, False):
            tag = (kind, "sum" if summed else "cat")
            # forward, every sample
            got = hip_ops.octree_forward(coords, li, tables, summed)
            assert got.shape == (n, fdim * (1 if summed else L))
            g = got.cpu().double().numpy()
            ref = oref.forward(cn, levels, lp, trk, host, summed)
            fscale = oref.abs_forward(cn, levels, lp, trk, host, summed)
            err = np.abs(g - ref)
            assert not np.isnan(g).any() and np.all(err <= (16 + L) * EPS * fscale), tag
            assert np.all(g[fscale == 0] == 0), tag
            worst_f = max(worst_f, float((err / np.maximum(fscale, 1e-30)).max() / EPS))
            assert float((got - octree_torch(coords, levels, tables, index, summed)).abs().max()) <= 1e-4, tag
            # gradients
            go = np.random.default_rng(7 + b).standard_normal(g.shape, dtype=np.float32)
            gt = torch.from_numpy(go).to(dev)
            grads, gc = hip_ops.octree_backward(coords, li, fdim, gt, summed, features=tables, need_features=True,
                                                need_coords=True)
            rt, rc, rs = oref.backward(cn, levels, lp, trk, host, go, summed, weight_dtype=np.float32)
            scale = oref.backward_scale(cn, levels, lp, trk, [t.shape[0] for t in host], go, summed)
            w, d = _check_tables(grads, rt, scale, levels, tag)
            worst_t, denormal = max(worst_t, w), denormal or d
            gcn = gc.cpu().double().numpy()
            cerr = np.abs(gcn - rc)
            assert not np.isnan(gcn).any() and np.all(cerr <= K * EPS * rs + 1e-6), tag
            assert np.all(gcn[rs == 0] == 0), tag
            worst_c = max(worst_c, float((cerr / (EPS * rs + 1e-30)).max()))
            _, gc2 = hip_ops.octree_backward(coords, li, fdim, gt, summed, features=tables, need_features=False,
                                             need_coords=True)
            assert torch.equal(gc.view(torch.int32), gc2.view(torch.int32)), tag
    print(f"octree levels={levels} F={fdim} {occ}: forward worst {worst_f:.2f} eps (bound {16 + L}); table gradient worst "
          f"error / bound {worst_t:.3f}, denormal term needed: {denormal}; coordinate gradient worst {worst_c:.2f} eps gscale "
          f"(K = {K})")


@pytest.mark.parametrize("levels,fdim,occ", [((5, 6, 7, 8), 5, "shell"), ((0, 1), 2, "dense"), ((3, 7), 3, "far")])
def test_backward_in_a_stale_workspace_of_exactly_the_queried_size(dev, levels, fdim, occ):
    """Through the C ABI: the workspace holds 0xFF in every byte, is exactly as long as the query says and has 4096 guard
    bytes behind it; the gradients (prefilled, too) are within the bound and the guard is untouched."""
    from shacira_amd import _lib, hip_ops
    lib = _lib.lib()
    levels = list(levels)
    index, cells = _index(occ, levels)
    li = [index[l].to(dev) for l in levels]
    lp, trk = _np_index(index, levels)
    n = 1537
    cn = ge.octree_coords(levels, cells, n, 55)
    coords = torch.from_numpy(cn).to(dev)
    go = np.random.default_rng(56).standard_normal((n, fdim), dtype=np.float32)
    gt = torch.from_numpy(go).to(dev)
    la, rows, ci, oc = hip_ops._octree_arrays(li)
    need = int(lib.shacira_octree_backward_workspace_bytes(n, len(levels), la, fdim, 1, _lib.OCTREE_GRAD_FEATURES))
    assert need >= 4 * n
    buf = torch.empty(need + 4096, dtype=torch.uint8, device=dev)
    buf[:need] = 0xFF
    buf[need:] = 0x5A
    grads = [torch.full((index[l].rows + 1, fdim), 7.0, device=dev) for l in levels]
    ptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    rc = lib.shacira_octree_backward(n, len(levels), la, fdim, ctypes.c_void_p(coords.data_ptr()), None, rows, ci, oc,
                                     ctypes.c_void_p(gt.data_ptr()), 1, _lib.OCTREE_GRAD_FEATURES, ptrs, None,
                                     ctypes.c_void_p(buf.data_ptr()), need,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[need:] == 0x5A).all()), "the backward wrote behind its workspace"
    zeros = [np.zeros((index[l].rows + 1, fdim), dtype=np.float32) for l in levels]
    rt, _, _ = oref.backward(cn, levels, lp, trk, zeros, go, True, weight_dtype=np.float32)
    scale = oref.backward_scale(cn, levels, lp, trk, [z.shape[0] for z in zeros], go, True)
    assert sum(int(c.sum()) for c, _ in scale) >= n
    worst, _ = _check_tables(grads, rt, scale, levels, (levels, occ, "workspace"))
    print(f"stale exact workspace levels={levels} F={fdim} {occ}: {need} bytes, worst error / bound {worst:.3f}")
