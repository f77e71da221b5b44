"""The forward's sample sort in two launches (psort_partition: tile-major runs + count matrices; psort_local: column sweep,
gather, ranking): the PLAN it leaves behind, read back through the layout of carve_plan (hashgrid_tiled.hip), at the sizes
where the sort changes its path -- one tile / a chunk edge, just over the 8 192 records one workgroup keeps, the smallest batch
sorted by rule, more than 256 tiles, two chunks per tile -- and on batches its bins are not sized for. The plan is checked as a
format (header, permutation, exact coordinate copies, monotone block offsets, sub-cell order inside the blocks of bins that are
not over-full); forward features are bit-equal to the unsorted variant, the planned backward agrees with the plain one within
the bar of test_gpu_plan.py. Reference semantics: wisp/csrc/ops/hashgrid_interpolate_cuda.cu:47-109 (order-independent)."""
import numpy as np
import pytest
import torch

from conftest import CONFIGS, table_layout
from test_gpu_parity import RTOL, _assert_grad_close, _ops, dev  # noqa: F401

pytestmark = pytest.mark.gpu

MAGIC = 0x53484354
TARGET_PER_BLOCK, MAX_BLOCKS, MAX_AXIS, MAX_COARSE, LOCAL_CAP, SUB_BITS = 352, 4096, 64, 256, 8192, 2
RULE_N = {3: 1 << 18, 2: 3 << 16}          # tiled_supported: batches sorted by rule (tables >= 8 MB, F = 2)

SIZES = [1, 63, 4095, 4096, 4097, 8193, (1 << 18) + 5, (1 << 20) + 4097, (1 << 21) + 1]
KINDS = ["one_block", "blob", "slab", "pm1", "nan"]
CASES = [(n, "uniform") for n in SIZES] + [(n, k) for n in (8193, (1 << 18) + 5) for k in KINDS]


def _grid(dim, n):
    """make_sort_plan of hashgrid_tiled.hip: blocks per axis and the coarse-bin shift of a batch of n samples."""
    want = n / TARGET_PER_BLOCK
    clampi = lambda v: min(max(int(v + 0.5), 1), MAX_AXIS)   # noqa: E731
    nb = [1, 1, 1]
    if dim == 3:
        m = min(clampi(np.cbrt(want / 2.0)), 12)
        z = clampi(want / (m * m))
        while m * m * z > MAX_BLOCKS:
            z -= 1
        nb = [m, m, z]
    else:
        m = clampi(np.sqrt(want / 2.0))
        y = clampi(want / m)
        while m * y > MAX_BLOCKS:
            y -= 1
        nb = [m, y, 1]
    num_blocks = nb[0] * nb[1] * nb[2]
    shift = 0
    while ((num_blocks + (1 << shift) - 1) >> shift) > MAX_COARSE:
        shift += 1
    return nb, num_blocks, shift


def _keys(xyz, dim, nb):
    """block_key and the sub-cell key of the local pass, in the kernel's fp32 arithmetic (no contraction)."""
    key = torch.zeros(xyz.shape[0], dtype=torch.int64, device=xyz.device)
    sub = torch.zeros_like(key)
    stride = 1
    for a in range(dim):
        u = (xyz[:, a] + 1.0) * np.float32(0.5 * nb[a])
        q = torch.where(~(u < nb[a]), torch.full_like(u, nb[a] - 1), torch.where(~(u >= 0), torch.zeros_like(u), u.floor()))
        key += q.to(torch.int64) * stride
        stride *= nb[a]
        fr = torch.nan_to_num(u - u.floor(), nan=0.0)
        s = (fr * (1 << SUB_BITS)).to(torch.int64).clamp(0, (1 << SUB_BITS) - 1)
        sub |= s << (a * SUB_BITS)
    return key, sub


def _coords(dim, n, kind, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    if kind == "one_block":
        c[:] = (0.123 + rng.uniform(-0.01, 0.01, c.shape)).astype(np.float32)
    elif kind == "blob":
        c[:] = np.clip(rng.normal(0.2, 0.07, c.shape), -1.0, 1.0).astype(np.float32)
        c[::7] = rng.uniform(-1.0, 1.0, c[::7].shape).astype(np.float32)
    elif kind == "slab":                     # 1 % of the cube's side along the last axis
        c[:, dim - 1] = (0.31 + rng.uniform(0.0, 0.02, n)).astype(np.float32)
    elif kind == "pm1":
        c[:] = np.where(rng.integers(0, 2, c.shape) == 1, 1.0, -1.0).astype(np.float32)
    elif kind == "nan":
        c[rng.integers(0, n, 7)] = np.nan
        c[n // 2, 0] = np.nan
    return c


@pytest.fixture(scope="module")
def tables(dev):
    """Config D's (3-D) and config Bp's (2-D) tables, uploaded once."""
    out = {}
    for dim, name in ((3, "D"), (2, "Bp")):
        _, res, bw = CONFIGS[name]
        sizes, first, T = table_layout(res, bw, dim)
        g = torch.Generator(device=dev).manual_seed(5 + dim)
        out[dim] = (res, bw, sizes, first, T, torch.randn((T, 2), generator=g, device=dev) * 0.01,
                    torch.from_numpy(first).to(dev))
    return out


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n,kind", CASES)
def test_two_pass_sort_plan_forward_and_backward(dev, tables, dim, n, kind):
    from shacira_amd import _lib
    ops = _ops()
    res, bw, sizes, first, T, tt, tf = tables[dim]
    L = len(res)
    tc = torch.from_numpy(_coords(dim, n, kind, seed=n % 1000 + dim)).to(dev)
    tg = torch.randn((n, 2 * L), generator=torch.Generator(device=dev).manual_seed(n % 977), device=dev)
    fwd = ops.hashgrid_interpolate_cuda if dim == 3 else ops.hashgrid_interpolate2d_cuda
    _lib.set_option("tiled", 0)
    try:
        assert ops.hashgrid_plan_bytes(dim, n, T, torch.float32, res, bw, 2) == 0
        feats_plain = fwd(tc, tt, tf, res, bw)
    finally:
        _lib.set_option("tiled", -1)
    grad_plain = ops.hashgrid_backward(dim, tc, tg, T, torch.float32, tf, res, bw, 2)
    forced = n < RULE_N[dim]
    if forced:
        _lib.set_option("fwd_variant", 8)
    _lib.set_option("bwd_brick", 1)           # as test_gpu_plan.py: the brick pass wherever the shape allows it
    try:
        plan = ops.hashgrid_plan_buffer(dim, tc, tt, res, bw)
        assert plan is not None, "this shape must sort"
        plan.fill_(0xA5)
        feats = fwd(tc, tt, tf, res, bw, plan=plan)
        grad = ops.hashgrid_backward(dim, tc, tg, T, torch.float32, tf, res, bw, 2, plan=plan)
    finally:
        _lib.set_option("bwd_brick", -1)
        if forced:
            _lib.set_option("fwd_variant", -1)
    torch.cuda.synchronize()

    # ---- the plan as a format (carve_plan: header 256 B | sorted4 [n] | block_start [num_blocks + 1], 256-byte aligned)
    nb, num_blocks, shift = _grid(dim, n)
    o_bs = 256 + (16 * n + 255) // 256 * 256
    assert plan.numel() >= o_bs + 4 * (num_blocks + 1)
    header = plan[:12].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert header.tolist() == [MAGIC, num_blocks, n]
    rec = plan[256:256 + 16 * n].view(torch.float32).view(n, 4)
    idx = rec[:, 3].contiguous().view(torch.int32).to(torch.int64)
    assert torch.equal(torch.sort(idx).values, torch.arange(n, device=dev)), "index field is not a permutation of 0..n-1"
    want = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    want[:, :dim] = tc[idx]
    assert torch.equal(rec[:, :3].contiguous().view(torch.int32), want.view(torch.int32)), "records are not exact copies"
    bs = plan[o_bs:o_bs + 4 * (num_blocks + 1)].view(torch.int32).to(torch.int64)
    assert int(bs[0]) == 0 and int(bs[-1]) == n and bool((bs[1:] >= bs[:-1]).all())
    key, sub = _keys(rec[:, :3], dim, nb)
    pos = torch.arange(n, device=dev)
    assert bool(((bs[key] <= pos) & (pos < bs[key + 1])).all()), "a record lies outside the range of its block"
    bin_tot = torch.bincount(key >> shift, minlength=MAX_COARSE)
    ordered = (bin_tot[key >> shift] <= LOCAL_CAP) & ~torch.isnan(rec[:, :dim]).any(1)
    cell = (key * (1 << (SUB_BITS * dim)) + sub)[ordered]
    assert bool((cell[1:] >= cell[:-1]).all()), "sub-cell order broken inside a bin that is not over-full"

    # ---- what is computed in that order
    assert torch.equal(feats.view(torch.int32), feats_plain.view(torch.int32)), "forward differs from the unsorted variant"
    _assert_grad_close(grad.cpu().numpy(), grad_plain.double().cpu().numpy(), first, sizes, rtol=RTOL)
