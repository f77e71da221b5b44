"""The dense-grid ray walk (shacira_amd/csrc/grid_walk.h) under its two visitors, ``raytrace_dense`` and ``spc_first_hit``, on
the MI355X against tests/golden/grid_walk.npz: what the kernels computed, on the same inputs, at the commit the file names
(tests/golden/make_grid_walk.py), when each kernel still carried a walk of its own. Everything is exact, depths bit for bit:
tests/test_gpu_spc.py compares the two visitors with each other, which no longer says anything about the arithmetic they share.
tests/test_spc_cpu.py holds the numpy restatement to the same file."""
import ctypes
import os

import numpy as np
import pytest
import torch

import spc_ref as S
from shacira_amd import _lib, hip_ops, render

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_walk.npz"))
DENSE = [(1, 0), (1, 8), (255, 1), (256, 3), (257, 8), (600, 3)]
KINDS = ("empty", "dense", "first", "last", "random")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def test_the_fixture_is_whole():
    assert len(str(GOLD["commit"])) == 40
    assert sum(k.endswith(".ridx") for k in GOLD.files) == len(DENSE) and sum(k.endswith(".hit") for k in GOLD.files) == 75


@pytest.mark.parametrize("N,level", DENSE)
def test_raytrace_dense_equals_the_recording(dev, N, level):
    g = lambda name: GOLD[f"dense.{N}.{level}.{name}"]
    o, d = torch.from_numpy(g("origins")).to(dev), torch.from_numpy(g("dirs")).to(dev)
    assert o.shape == (N, 3)
    occ = torch.from_numpy(S.occupancy_from_bits(g("bits"), level)).to(dev)
    ridx, pidx, depth = render.raytrace_dense(o, d, occ, level)
    counts = torch.full((N,), -1, dtype=torch.int32, device=dev)
    occ8 = occ.to(torch.uint8).contiguous()
    assert _lib.lib().shacira_raytrace_dense_count(N, o.data_ptr(), d.data_ptr(), occ8.data_ptr(), level, counts.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), g("counts"))
    assert np.array_equal(ridx.cpu().numpy(), g("ridx")) and np.array_equal(pidx.cpu().numpy(), g("pidx"))
    assert depth.shape == g("depth").shape
    assert np.array_equal(_bits(depth[:, 0]), g("depth")[:, 0].view(np.int32))
    assert np.array_equal(_bits(depth[:, 1]), g("depth")[:, 1].view(np.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("level", [1, 2, 5])
def test_first_hit_equals_the_recording(dev, level, kind):
    from shacira_amd.wisp.ops.spc.structured import pack_occupancy
    key = f"hit.{level}.{kind}."
    words = pack_occupancy(torch.from_numpy(S.occupancy_from_bits(GOLD[key + "bits"], level)).to(dev))
    rank_h, cells = S.rank_ref(words.cpu().numpy().view(np.uint32))
    colors = torch.from_numpy(GOLD[key + "colors"]).to(dev)
    assert colors.shape == (cells, 4)
    rank = torch.from_numpy(rank_h).to(dev)
    for N in (1, 63, 64, 65, 257):
        g = lambda name: GOLD[f"{key}{N}.{name}"]
        o, d = torch.from_numpy(g("origins")).to(dev), torch.from_numpy(g("dirs")).to(dev)
        assert o.shape == (N, 3)
        if N >= 63:                     # the four rays that are not finite and the zero directions are among them
            assert (~np.isfinite(g("origins")).all(axis=1) | ~np.isfinite(g("dirs")).all(axis=1)).sum() == 4
            assert (g("dirs") == 0).all(axis=1).sum() == 2
        calls = [(None, None)] + ([(rank, colors)] if cells else [])          # without colours, and with them
        for rk, col in calls:
            depth, hit, pidx, rgb = hip_ops.spc_first_hit(o, d, level, words, rk, col)
            assert np.array_equal(hit.cpu().numpy(), g("hit")) and np.array_equal(pidx.cpu().numpy(), g("pidx"))
            assert np.array_equal(_bits(depth), g("depth").view(np.int32))
            if col is None:
                assert rgb is None
            else:
                assert np.array_equal(_bits(rgb), g("rgb").view(np.int32))
