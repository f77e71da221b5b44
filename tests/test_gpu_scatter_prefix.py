"""Where the scatter pass of the binned backward puts its (tile, bucket) runs: the bucket scan lays them out in tile order
(a prefix over the scatter tiles of the padded run lengths, bwd_bin_front.h scan_run_offsets) and the scatter workgroups load
`bucket base + offset` instead of drawing a place from a cursor. A misplaced run overwrites another run's items or leaves a
hole of stale units inside a bucket, so every case compares `hip_ops.hashgrid_backward` with the fp64-accumulating oracle at the
bar of tests/test_gpu_parity.py (`_assert_grad_close`: rtol 1e-5 + atol 1e-5 x the level's maximum; fp16 tables: that file's
2e-3, the rounding of the half-precision output). Shapes: the smallest at which the placement can go wrong -- several scatter
tiles, several buckets per hashed level, partial last tiles, empty and over-full buckets, every item format.
Reference semantics: wisp/csrc/ops/hashgrid_interpolate_cuda.cu:143-221."""
import numpy as np
import pytest
import torch

from conftest import CONFIGS, geo, table_layout
from oracle import hashgrid_c as oc
from test_gpu_parity import RTOL, _assert_grad_close, _ops, _problem, dev  # noqa: F401

pytestmark = pytest.mark.gpu

# 3-D, L8, bw14: two dense levels, six hashed ones of 16 384 rows = four buckets each with the 64 KiB images of small batches
RES8, BW8 = geo(16, 256, 8), 14
TILE = 1024          # samples per scatter tile, 3-D
COUNT_TILE = 128     # samples per counting tile of the fused front kernel at these batch sizes (eight counting rows per tile)


def _backward_close(dev, dim, res, bw, coords, go, first, sizes, T, F=2, dtype=torch.float32, plan=None):
    ops = _ops()
    tc = torch.from_numpy(coords).to(dev)
    tf = torch.from_numpy(first).to(dev)
    tg = torch.from_numpy(go).to(dev).to(dtype)
    grad = ops.hashgrid_backward(dim, tc, tg, T, dtype, tf, res, bw, F, plan=plan)
    torch.cuda.synchronize()
    go_seen = go.astype(np.float16).astype(np.float32) if dtype == torch.float16 else go
    ref = oc.backward(coords, go_seen, (T, F), first, res, bw)
    _assert_grad_close(grad.float().cpu().numpy(), ref, first, sizes, rtol=RTOL if dtype == torch.float32 else 2e-3)
    return grad


def test_partial_last_scatter_tile(dev):
    """15 whole scatter tiles and one of 77 samples (a single counting row): the last tile's offset + its padded count must
    meet the bucket's total from the counting pass."""
    n = 3 * TILE + 77 + 12 * TILE
    sizes, first, T, coords, table, go = _problem(3, RES8, BW8, n, seed=11)
    _backward_close(dev, 3, RES8, BW8, coords, go, first, sizes, T)


def test_partial_last_counting_tile(dev):
    """The last scatter tile has all of its counting rows, the last of them partial (78 of 128 samples)."""
    n = 13 * TILE - (COUNT_TILE - 78)
    assert n % COUNT_TILE == 78 and (n + COUNT_TILE - 1) // COUNT_TILE == 13 * (TILE // COUNT_TILE)
    sizes, first, T, coords, table, go = _problem(3, RES8, BW8, n, seed=12)
    _backward_close(dev, 3, RES8, BW8, coords, go, first, sizes, T)


def test_over_full_buckets(dev):
    """Every sample in one cell of the finest level: one bucket per level receives everything -- the largest prefix, buckets cut
    into several work units -- and every other bucket of the level stays empty."""
    n = 3 * TILE + 77 + 12 * TILE
    sizes, first, T, coords, table, go = _problem(3, RES8, BW8, n, seed=13, edge=False)
    rng = np.random.default_rng(14)
    cell = 2.0 / RES8[-1]
    coords[:] = (np.array([0.31, -0.27, 0.11]) + rng.uniform(0.1, 0.4, (n, 3)) * cell * 0.5).astype(np.float32)
    _backward_close(dev, 3, RES8, BW8, coords, go, first, sizes, T)


def test_empty_buckets_and_zero_length_runs(dev):
    """Half the samples on one z-plane (the first half of the batch: whole tiles that touch one z-slab bucket of a dense level),
    half of those on one (y, z) line as well (tiles that touch a few buckets of a hashed level), the rest uniform: columns of
    the count matrix with zero-length runs between non-empty ones, and a 1-sample last tile."""
    n = 12 * TILE + 1
    sizes, first, T, coords, table, go = _problem(3, RES8, BW8, n, seed=15, edge=False)
    coords[: n // 2, 2] = np.float32(0.4321)
    coords[: n // 4, 1] = np.float32(-0.1234)
    _backward_close(dev, 3, RES8, BW8, coords, go, first, sizes, T)


def test_pad_arithmetic_on_the_planned_path(dev):
    """The smallest batch that takes the plan (2^18 samples, config D's table): sorted samples, 12-byte units in runs padded to
    16 units, two counting rows per scatter tile. The whole table is compared (the C oracle takes about a second)."""
    ops = _ops()
    dim, res, bw = CONFIGS["D"]
    n = 1 << 18
    sizes, first, T, coords, table, go = _problem(dim, res, bw, n, seed=16)
    tc, tt, tf = (torch.from_numpy(a).to(dev) for a in (coords, table, first))
    plan = ops.hashgrid_plan_buffer(dim, tc, tt, res, bw)
    assert plan is not None
    ops.hashgrid_interpolate_cuda(tc, tt, tf, res, bw, plan=plan)
    _backward_close(dev, dim, res, bw, coords, go, first, sizes, T, plan=plan)


def test_padded_runs_of_16_byte_units(dev):
    """The smallest plain call whose runs are padded (2^17 samples: fixed-point images, 16-byte units in runs of 4; 128 scatter
    tiles of four counting rows each), three samples past the last whole tile."""
    n = (1 << 17) + 3
    sizes, first, T, coords, table, go = _problem(3, RES8, BW8, n, seed=19)
    _backward_close(dev, 3, RES8, BW8, coords, go, first, sizes, T)


def test_more_counting_rows_than_one_sweep(dev):
    """The bucket scan walks 64 x 32 = 2 048 counting rows per sweep and carries a column's sum into the next one. A table of
    24 levels with F = 4 counts in tiles of 128 samples (its staging image leaves no room for larger ones), so 2^18 + 1 029
    samples are 2 057 counting rows: a second sweep of nine rows -- one whole scatter tile and a one-row last tile."""
    res, bw, F = geo(16, 512, 24), 14, 4
    n = (1 << 18) + TILE + 5
    assert (n + COUNT_TILE - 1) // COUNT_TILE == 2048 + 9
    sizes, first, T, coords, table, go = _problem(3, res, bw, n, F=F, seed=20)
    _backward_close(dev, 3, res, bw, coords, go, first, sizes, T, F=F)


@pytest.mark.parametrize("case", ["2d_bw19", "fp16_f2", "f4", "f4_fp16"])
def test_other_item_formats(dev, case):
    """One call per template instantiation of the scatter kernel that the cases above do not reach, at its smallest binned
    batch: 2-D (2 048-sample tiles), 8-byte half-precision items (never padded), 24-byte items (staging windows), 16-byte half
    items of F = 4. Batches below 2^17 samples: exact runs (pad = 1) in every format; padded runs are the two cases above and
    the planned one."""
    dim, res, bw, F, dtype, n = {
        "2d_bw19": (*CONFIGS["Bp"], 2, torch.float32, 16384 + 5),
        "fp16_f2": (3, RES8, BW8, 2, torch.float16, 12288 + 5),
        "f4": (3, RES8, BW8, 4, torch.float32, 16384 + 5),
        "f4_fp16": (3, RES8, BW8, 4, torch.float16, 16384 + 5),
    }[case]
    sizes, first, T, coords, table, go = _problem(dim, res, bw, n, F=F, seed=17)
    _backward_close(dev, dim, res, bw, coords, go, first, sizes, T, F=F, dtype=dtype)


def test_sub_batches(dev):
    """One call split into sub-batches of two scatter tiles (option bin_batch_mib, as in tests/test_gpu_plan.py): the
    standalone counting pass writes one row per scatter tile, and every sub-batch lays out its own runs."""
    from shacira_amd import _lib
    n = 3 * TILE + 77 + 12 * TILE
    sizes, first, T, coords, table, go = _problem(3, RES8, BW8, n, seed=18)
    _lib.set_option("bin_batch_mib", 1)
    try:
        _backward_close(dev, 3, RES8, BW8, coords, go, first, sizes, T)
    finally:
        _lib.set_option("bin_batch_mib", 1536)
