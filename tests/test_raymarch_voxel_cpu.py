"""The seeded voxel march on the host (no GPU): the restated jitter (tests/raymarch_voxel_ref.py; the GPU test ties the kernel to
it bit for bit), the library surface of the new entry points, and the argument checks that precede any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_sample_ref as M
import raymarch_voxel_ref as V
from conftest import ROOT
from shacira_amd import _lib

NEW = ("shacira_raymarch_voxel_workspace_bytes", "shacira_raymarch_voxel_emit")


def test_philox_of_the_restatement_reproduces_the_known_answers():
    assert V.philox4x32_10 is M.philox4x32_10
    for counter, key, want in M.KNOWN_ANSWERS:
        assert tuple(int(x) for x in V.philox4x32_10(*counter, *key)) == want
    # the jitter word is word j & 3 of the call on (r, i, j >> 2, step) under the two halves of the seed
    c, k, want = M.KNOWN_ANSWERS[2]
    for lane in range(4):
        got = V.jitter_words(seed=(k[1] << 32) | k[0], step=c[3], r=c[0], i=c[1], j=4 * c[2] + lane)
        assert int(got) == want[lane]


def test_jitter_lies_in_the_unit_interval_and_every_input_moves_it():
    rng = np.random.default_rng(0)
    ridx = np.sort(rng.integers(0, 50, 400))
    jit = V.jitter(seed=99, step=3, ridx=ridx, num_samples=37)
    assert jit.dtype == np.float32 and jit.shape == (400, 37)
    assert (jit >= 0).all() and (jit < 1).all() and len(np.unique(jit)) > 0.99 * jit.size
    assert abs(float(jit.mean()) - 0.5) < 0.01
    base = dict(seed=5, step=7, r=11, i=2, j=9)
    w0 = int(V.jitter_words(**base))
    for name, other in (("seed", 6), ("seed", 5 | (1 << 32)), ("step", 8), ("r", 12), ("i", 3), ("j", 10), ("j", 13)):
        assert int(V.jitter_words(**dict(base, **{name: other}))) != w0, name
    # unit(): the top 24 bits, so 0xFFFFFFFF stays below 1
    assert float(M.unit(np.uint32(0xFFFFFFFF))) == 1.0 - 2.0 ** -24 and float(M.unit(np.uint32(0xFF))) == 0.0


def test_five_samples_take_four_words_of_one_call_and_the_first_of_the_next():
    seed, step, r, i = 0x0123456789ABCDEF, 4, 6, 1
    ridx = np.array([6, 6, 7])                                     # nugget 1 of ray 6 is row 1
    jit = V.jitter(seed, step, ridx, num_samples=5)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    call0, call1 = M.philox4x32_10(r, i, 0, step, k0, k1), M.philox4x32_10(r, i, 1, step, k0, k1)
    want = [call0[0], call0[1], call0[2], call0[3], call1[0]]
    assert [float(x) for x in jit[1]] == [float(M.unit(w)) for w in want]
    assert V.nugget_index(np.array([2, 2, 2, 5, 9, 9])).tolist() == [0, 1, 2, 0, 0, 1]


_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float}


def _declared(name, header):
    m = re.search(r"SHACIRA_API\s+(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else _CTYPES[a.replace("const ", "").split()[0]])
    return _CTYPES[m.group(1)], args


def test_library_surface():
    header = open(os.path.join(ROOT, "include", "shacira_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header and hasattr(handle, name) and name in _lib.SIGNATURES
        res, args = _declared(name, header)
        assert _lib.SIGNATURES[name] == (res, args), name
    assert _lib.lib().shacira_abi_version() == 11                 # additive entry points do not move the ABI
    for word in ("Philox4x32-10", "(r, i, j >> 2", "step_dev"):   # the counter layout is part of the contract
        assert word in header, word


def test_entry_point_validates_before_it_launches():
    """The pointers are never dereferenced: every call returns before a HIP call."""
    L = _lib.lib()
    one = ctypes.c_void_p(64)

    def emit(n=1, ns=4, o=one, d=one, occ=one, level=3, offsets=one, cap=8, ws=one, ws_bytes=1 << 20, out=one):
        return L.shacira_raymarch_voxel_emit(n, ns, o, d, occ, level, offsets, 7, 0, None, cap, ws, ws_bytes, out, out, out,
                                             out, out, None)

    assert emit(n=0) == 0 and emit(cap=0) == 0                   # nothing to do: success, nothing launched
    assert emit(n=0, o=None, d=None, occ=None, offsets=None, ws=None, out=None) == 0
    assert emit(n=1 << 32) == _lib.EINVAL and emit(n=-1) == _lib.EINVAL
    assert emit(ns=0) == _lib.EINVAL and emit(cap=-1) == _lib.EINVAL and emit(level=11) == _lib.EINVAL
    assert emit(o=None) == _lib.EINVAL and emit(offsets=None) == _lib.EINVAL and emit(out=None) == _lib.EINVAL
    assert emit(ws=None) == _lib.EWORKSPACE and emit(cap=9, ws_bytes=35) == _lib.EWORKSPACE
    assert L.shacira_raymarch_voxel_workspace_bytes(9, 4) == 36   # 3 nuggets (the third cut) x 12 bytes
    assert L.shacira_raymarch_voxel_workspace_bytes(8, 4) == 24 and L.shacira_raymarch_voxel_workspace_bytes(0, 4) == 0


def test_python_argument_checks():
    from shacira_amd import render
    from shacira_amd.wisp.accelstructs import AxisAlignedBBoxAS, OctreeAS
    from shacira_amd.wisp.core import Rays
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render.raymarch_voxel(o, d, torch.ones(2, 2, 2, dtype=torch.bool), 1, 4, seed=1)
    rays = Rays(o, d, dist_min=0.0, dist_max=4.0)
    for blas in (OctreeAS.make_dense(1), AxisAlignedBBoxAS()):
        with pytest.raises(ValueError, match="seed"):
            blas.raymarch(rays, "ray", 4, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # the seeded voxel march is the HIP one: no torch chain
        OctreeAS.make_dense(1).raymarch(rays, "voxel", 4, seed=1)
