"""The coordinate gradient of the hash-grid operator, without a GPU: the fp64 restatement (tests/coord_grad_ref.py) against
autograd through the torch oracle and against central differences, its clamp / NaN rules, and the validation codes of the
new C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import CONFIGS, table_layout
from coord_grad_ref import assert_close, coord_grad, fractions
from oracle.hashgrid_torch import hashgrid_forward


def _setup(dim, res, bw, N, F=2, seed=0, dtype=np.float32):
    sizes, first, T = table_layout(res, bw, dim)
    rng = np.random.default_rng(seed)
    coords = rng.uniform(-0.95, 0.95, (N, dim)).astype(np.float32)
    table = (rng.standard_normal((T, F)) * 0.1).astype(dtype)
    go = rng.standard_normal((N, len(res) * F)).astype(np.float32)
    return first, coords, table, go


def _interior(coords, res, margin):
    """Samples whose fraction on every level and axis keeps `margin` from the cell boundaries."""
    keep = np.ones(coords.shape[0], dtype=bool)
    for r in res:
        frac, _, slope = fractions(coords, r)
        keep &= ((frac > margin) & (frac < 1 - margin) & (slope > 0)).all(1)
    return keep


@pytest.mark.parametrize("name,F", [("A", 2), ("A", 4), ("D", 2)])
def test_restatement_matches_autograd_through_the_torch_oracle(name, F):
    dim, res, bw = CONFIGS[name]
    if name == "D":
        res, bw = res[:6], 14      # (a small 3-D table: dense and hashed levels, CPU-sized)
    first, coords, table, go = _setup(dim, res, bw, 300, F)
    c = torch.from_numpy(coords).requires_grad_(True)
    feats = hashgrid_forward(c, torch.from_numpy(table), first, res, bw)
    feats.backward(torch.from_numpy(go))
    ref, bound = coord_grad(coords, table, first, res, bw, go)
    keep = _interior(coords, res, 1e-4)       # (autograd of torch.minimum splits the gradient at a tie)
    assert keep.sum() > 250
    assert_close(c.grad.numpy()[keep], ref[keep], bound[keep], rel=1e-5, what="autograd")


def _forward64(coords64, table, first, res, bw):
    """fp64 forward (fp64 transform and weights; the rows of the kernels) for central differences."""
    N, dim = coords64.shape
    out = []
    from oracle.hashgrid_torch import corner_rows_and_weights
    for l, r in enumerate(res):
        rows, _ = corner_rows_and_weights(torch.from_numpy(coords64.astype(np.float32)), int(r), 2 ** bw)
        rows = rows.numpy() + int(first[l])
        x = np.clip(r * (coords64 * 0.5 + 0.5), 0.0, r - 1.0 - 1e-5)
        fr = x - np.floor(x)
        acc = 0.0
        for k in range(1 << dim):
            w = np.ones(N)
            for a in range(dim):
                w = w * (fr[:, a] if k & (1 << (dim - 1 - a)) else 1.0 - fr[:, a])
            acc = acc + w[:, None] * table[rows[:, k]]
        out.append(acc)
    return np.concatenate(out, 1)


@pytest.mark.parametrize("name", ["A", "D"])
def test_restatement_matches_central_differences_on_an_fp64_table(name):
    dim, res, bw = CONFIGS[name]
    if name == "D":
        res, bw = res[:5], 14
    first, coords, table, go = _setup(dim, res, bw, 400, 2, seed=3, dtype=np.float64)
    # the rows of a sample must not change within +-h: keep samples away from every cell boundary
    keep = _interior(coords, res, 2e-3)
    coords = coords[keep]
    go = go[keep]
    assert coords.shape[0] > 100
    ref, _ = coord_grad(coords, table, first, res, bw, go)
    h = 1e-7
    fd = np.zeros_like(ref)
    c64 = coords.astype(np.float64)
    for a in range(dim):
        e = np.zeros(dim)
        e[a] = h
        fp = (_forward64(c64 + e, table, first, res, bw) * go).sum(1)
        fm = (_forward64(c64 - e, table, first, res, bw) * go).sum(1)
        fd[:, a] = (fp - fm) / (2 * h)
    scale = np.abs(ref).max()
    np.testing.assert_allclose(ref, fd, rtol=2e-4, atol=2e-5 * scale)


def test_clamped_axes_and_nan_give_zero_and_the_lower_end_passes():
    dim, res, bw = CONFIGS["A"]
    first, coords, table, go = _setup(dim, res, bw, 6)
    coords[0] = (2.5, 0.3)        # x clamped above
    coords[1] = (0.2, -9.0)       # y clamped below
    coords[2] = (np.nan, 0.1)     # NaN x
    coords[3] = (1.0, 0.4)        # +1: u = res > hi, clamped
    coords[4] = (-1.0, 0.4)       # -1: u = 0, inside (both ends inclusive)
    coords[5] = (np.float32(-1.0) + np.float32(2.0 ** -23), 0.4)
    grad, _ = coord_grad(coords, table, first, res, bw, go)
    assert grad[0, 0] == 0 and grad[1, 1] == 0 and grad[2, 0] == 0 and grad[3, 0] == 0
    assert grad[0, 1] != 0 and grad[1, 0] != 0 and grad[2, 1] != 0 and grad[3, 1] != 0
    for r in res:
        assert fractions(coords[4:5], r)[2][0, 0] == 0.5 * r
    # at c = -1 the slope is the one-sided value of the first cell: that of a point just inside it
    go[5] = go[4]
    assert grad[4, 0] != 0
    np.testing.assert_allclose(coord_grad(coords[4:6], table, first, res, bw, go[4:6])[0][:, 0],
                               [grad[4, 0]] * 2, rtol=1e-4)


def test_coords_backward_entry_points_validate_without_a_gpu():
    from shacira_amd import _lib
    L = _lib.lib()
    res = (ctypes.c_int32 * 2)(16, 32)
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first or N == 0
    cb = L.shacira_hashgrid_coords_backward

    def call(dim=2, n=5, lods=2, F=2, bw=8, first=one, coords=one, table=one, go=one, dt=0, out=one, plan=None,
             plan_bytes=0):
        return cb(dim, n, lods, F, bw, res, first, 10, coords, table, go, dt, out, plan, plan_bytes, None, 0, None)

    assert call(dim=4) == _lib.EINVAL
    assert call(lods=0) == _lib.EINVAL
    assert call(lods=33) == _lib.EINVAL
    assert call(F=3) == _lib.EODD
    assert call(bw=31) == _lib.EINVAL
    assert call(dt=7) == _lib.EDTYPE
    assert call(n=-1) == _lib.EINVAL
    for k in ("first", "coords", "table", "go", "out"):
        assert call(**{k: None}) == _lib.EINVAL, k
    assert call(n=0, coords=None, out=None) == 0
    assert L.shacira_hashgrid_coords_backward_workspace_bytes(2, 5, 2, 2, 8, res, 10, 0) == 0
    # option values: -1, 0, 3, 8
    for v in (0, 3, 8, -1):
        assert L.shacira_set_option(b"coord_variant", v) == 0
    assert _lib.get_option("coord_variant") == -1
    for v in (1, 2, 6, 9):
        assert L.shacira_set_option(b"coord_variant", v) == _lib.EINVAL
