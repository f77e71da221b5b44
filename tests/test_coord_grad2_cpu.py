"""The backward of the hash-grid coordinate gradient, without a GPU: the fp64 restatement (tests/coord_grad2_ref.py) against
the double backward of autograd through the torch oracle, its clamp / NaN rules, and the validation codes of the two C entry
points."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import CONFIGS, table_layout
from coord_grad2_ref import coord_grad2, dense_table_grad
from coord_grad_ref import assert_close, fractions
from oracle.hashgrid_torch import hashgrid_forward


def _setup(dim, res, bw, N, F=2, seed=0):
    sizes, first, T = table_layout(res, bw, dim)
    rng = np.random.default_rng(seed)
    coords = rng.uniform(-0.95, 0.95, (N, dim)).astype(np.float32)
    table = (rng.standard_normal((T, F)) * 0.1).astype(np.float32)
    go = rng.standard_normal((N, len(res) * F)).astype(np.float32)
    v = rng.standard_normal((N, dim)).astype(np.float32)
    return first, coords, table, go, v


def _interior(coords, res, margin):
    keep = np.ones(coords.shape[0], dtype=bool)
    for r in res:
        frac, _, slope = fractions(coords, r)
        keep &= ((frac > margin) & (frac < 1 - margin) & (slope > 0)).all(1)
    return keep


@pytest.mark.parametrize("name,F", [("A", 2), ("A", 4), ("D", 2)])
def test_restatement_matches_the_double_backward_of_autograd_through_the_torch_oracle(name, F):
    dim, res, bw = CONFIGS[name]
    if name == "D":
        res, bw = res[:6], 14      # (a small 3-D table: dense and hashed levels, CPU-sized)
    first, coords, table, go, v = _setup(dim, res, bw, 300, F)
    keep = _interior(coords, res, 1e-4)       # (autograd of torch.minimum splits the gradient at a tie)
    assert keep.sum() >= 250
    coords, go, v = coords[keep], go[keep], v[keep]
    c = torch.from_numpy(coords).requires_grad_(True)
    t = torch.from_numpy(table).requires_grad_(True)
    g = torch.from_numpy(go).requires_grad_(True)
    feats = hashgrid_forward(c, t, first, res, bw)
    (gc,) = torch.autograd.grad(feats, c, g, create_graph=True)
    d_g, d_t, d_c = torch.autograd.grad((gc * torch.from_numpy(v)).sum(), [g, t, c])
    ref = coord_grad2(coords, table, first, res, bw, go, v)
    assert_close(d_g.numpy(), ref["ggo"], ref["ggo_bound"], rel=1e-5, what="grad_grad_output")
    assert_close(d_c.numpy(), ref["gc"], ref["gc_bound"], rel=1e-5, what="grad_coords")
    dense = dense_table_grad(ref, table.shape[0])
    edges = list(first) + [table.shape[0]]
    for l in range(len(res)):
        a, b = d_t.numpy()[edges[l]:edges[l + 1]].astype(np.float64), dense[edges[l]:edges[l + 1]]
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), f"level {l}"


def test_clamped_axes_and_nan_contribute_nothing_and_the_lower_end_passes():
    dim, res, bw = CONFIGS["A"]
    first, coords, table, go, v = _setup(dim, res, bw, 6)
    coords[0] = (2.5, 0.3)        # x clamped above
    coords[1] = (0.2, -9.0)       # y clamped below
    coords[2] = (np.nan, 0.1)     # NaN x
    coords[3] = (1.0, 0.4)        # +1: u = res > hi, clamped
    coords[4] = (-1.0, 0.4)       # -1: u = 0, inside (both ends inclusive)
    coords[5] = (0.3, 0.4)
    F, L, T = 2, len(res), table.shape[0]
    full = coord_grad2(coords, table, first, res, bw, go, v)
    # (3) needs both slopes: a sample with one clamped axis gets nothing at all; -1 passes
    for n in range(4):
        assert full["gc"][n].tolist() == [0.0, 0.0], n
    assert (full["gc"][4] != 0).all() and (full["gc"][5] != 0).all()
    # (1) and (2): the clamped axis drops out -- the results are those of v with that component zeroed, and for a sample
    # whose only live direction is the clamped axis they vanish
    for n, axis in ((0, 0), (1, 1), (2, 0), (3, 0)):
        one = slice(n, n + 1)
        v0 = v[one].copy()
        v0[0, axis] = 0.0
        a = coord_grad2(coords[one], table, first, res, bw, go[one], v[one])
        b = coord_grad2(coords[one], table, first, res, bw, go[one], v0)
        assert np.array_equal(a["ggo"], b["ggo"]) and np.array_equal(a["vals"], b["vals"]), n
        assert np.abs(a["ggo"]).max() > 0
        only = np.zeros((1, dim), dtype=np.float32)
        only[0, axis] = 1.0
        z = coord_grad2(coords[one], table, first, res, bw, go[one], only)
        assert not z["ggo"].any() and not z["vals"].any() and not z["gc"].any(), n
    live = np.zeros((1, dim), dtype=np.float32)
    live[0, 0] = 1.0
    p = coord_grad2(coords[4:5], table, first, res, bw, go[4:5], live)
    assert p["ggo"].any() and p["vals"].any() and p["gc"][0, 1] != 0
    assert dense_table_grad(full, T).shape == (T, F) and full["ggo"].shape == (6, L * F)


def test_coords_backward2_entry_points_validate_without_a_gpu():
    from shacira_amd import _lib
    L = _lib.lib()
    res = (ctypes.c_int32 * 2)(16, 32)
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first or there is nothing to do
    fn = L.shacira_hashgrid_coords_backward2
    query = L.shacira_hashgrid_coords_backward2_workspace_bytes

    def call(dim=2, n=5, lods=2, F=2, bw=8, res=res, first=one, rows=10, coords=one, table=one, go=one, v=one, dt=_lib.F32,
             ggo=one, gcb=one, gc=one, plan=None, plan_bytes=0, ws=None, ws_bytes=0):
        return fn(dim, n, lods, F, bw, res, first, rows, coords, table, go, v, dt, ggo, gcb, gc, plan, plan_bytes, ws,
                  ws_bytes, None)

    assert call(dim=4) == _lib.EINVAL
    assert call(dim=1) == _lib.EINVAL
    assert call(lods=0) == _lib.EINVAL
    assert call(lods=33) == _lib.EINVAL
    assert call(F=3) == _lib.EODD
    assert call(bw=31) == _lib.EINVAL
    assert call(dt=_lib.F64) == _lib.EDTYPE        # fp64 tables are first order only
    assert call(dt=7) == _lib.EDTYPE
    assert call(n=-1) == _lib.EINVAL
    # NULL operands
    for k in ("first", "coords", "v"):
        assert call(**{k: None}) == _lib.EINVAL, k
    assert call(ggo=None, gcb=None, gc=None) == _lib.EINVAL                 # nothing requested
    assert call(table=None) == _lib.EINVAL and call(go=None) == _lib.EINVAL
    assert call(table=None, gcb=None) == _lib.EINVAL                        # (1) and (3) read the table
    assert call(go=None, ggo=None) == _lib.EINVAL                           # (2) and (3) read grad_output
    assert call(go=None, gc=None) == _lib.EINVAL
    # fp16: grad_codebook accumulates in an fp32 image in the workspace
    assert query(2, 5, 2, 2, 8, res, 10, _lib.F16) == 10 * 2 * 4
    assert query(2, 5, 2, 2, 8, res, 10, _lib.F32) == 0
    assert query(4, 5, 2, 2, 8, res, 10, _lib.F16) == 0                     # invalid shapes: 0, like the other queries
    assert call(dt=_lib.F16) == _lib.EWORKSPACE
    assert call(dt=_lib.F16, ws=one, ws_bytes=79) == _lib.EWORKSPACE
    # a short plan for a batch that has one (config D at 2^18 samples sorts)
    dim, resD, bw = CONFIGS["D"]
    _, _, T = table_layout(resD, bw, dim)
    arr = (ctypes.c_int32 * len(resD))(*resD)
    assert L.shacira_hashgrid_plan_bytes(dim, 1 << 18, len(resD), 2, bw, arr, T, _lib.F32) > 16
    assert call(dim=dim, n=1 << 18, lods=len(resD), bw=bw, res=arr, rows=T, plan=one, plan_bytes=16) == _lib.EWORKSPACE
    # num_coords == 0: nothing to do (a requested grad_codebook of an empty table has nothing to zero)
    assert call(n=0, coords=None, table=None, go=None, v=None, gcb=None) == 0
    assert call(n=0, rows=0) == 0
