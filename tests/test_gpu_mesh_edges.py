"""compute_sdf and closest_point on the MI355X at their edges: ``hip_ops.mesh_sdf`` and ``hip_ops.mesh_closest`` (signed and
unsigned) of mesh_sdf.hip against the numpy restatements (tests/mesh_sdf_ref.py, tests/mesh_closest_ref.py) on the inputs of
tests/mesh_edge_cases.py, by the rules of test_gpu_mesh_sdf.py and test_gpu_mesh_closest.py: every row compared, the fp32 bit
patterns of sdf, dist and hit, tidx exactly. No tolerance anywhere. What each case is and why it bites is
tests/test_mesh_edges_cpu.py's subject; wall times are in profiles/mesh_edges.md.

  special positions   points exactly on faces, edges, vertices and symmetry planes and one ulp to either side: the sign of a
                      zero under copysignf, s == 2, E0 == E1, u == 0, u + v == 1, t == 0, d2 == 0 and ties between triangles
                      (the kernel precomputes records, drops the literal-zero terms of dot(dir, q) and merges chunks with
                      atomics on bit patterns: only such inputs can tell that from the contract)
  partitions          N around the 256 lanes and 512 points of a workgroup; T around the chunk granule; T = one pass exactly
                      and one more; one chunk per pass over two passes (the accumulator is fed by passes alone)
  slivers             normals that are denormal, tiny or exactly zero
  non-finite          what the contract specifies for NaN, infinite and overflowing rows, and only that
"""
import numpy as np
import pytest
import torch

import mesh_closest_ref as cref
import mesh_edge_cases as me
import mesh_sdf_ref as ref
from mesh_sdf_ref import _POINTS, _bits, _triangles

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _device_calls(points, tri, dev):
    """(sdf, signed closest, unsigned closest) of the kernels as numpy, shapes and types checked."""
    from shacira_amd import hip_ops
    n = points.shape[0]
    p, t = torch.from_numpy(points).to(dev), torch.from_numpy(tri).to(dev)
    sdf = hip_ops.mesh_sdf(p, t)
    assert sdf.dtype == torch.float32 and tuple(sdf.shape) == (n,) and sdf.device == dev
    out = [sdf.cpu().numpy()]
    for signed in (True, False):
        dist, hit, tidx = hip_ops.mesh_closest(p, t, signed=signed)
        assert dist.dtype == torch.float32 and tuple(dist.shape) == (n,) and dist.device == dev
        assert hit.dtype == torch.float32 and tuple(hit.shape) == (n, 3) and hit.device == dev
        assert tidx.dtype == torch.int32 and tuple(tidx.shape) == (n,) and tidx.device == dev
        out.append((dist.cpu().numpy(), hit.cpu().numpy(), tidx.cpu().numpy()))
    return tuple(out)


def _restatements(points, tri):
    """(sdf, signed closest, unsigned closest) of the contract."""
    return (ref.mesh_sdf_ref(points, tri), cref.mesh_closest_ref(points, tri, signed=True),
            cref.mesh_closest_ref(points, tri, signed=False))


def _same(got, want, rows=slice(None)):
    assert np.array_equal(_bits(got[0][rows]), _bits(want[0][rows]))
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(_bits(g[0][rows]), _bits(w[0][rows]))
        assert np.array_equal(_bits(g[1][rows]), _bits(w[1][rows]))
        assert np.array_equal(g[2][rows], w[2][rows])


_WANT = {}


def _want(key, points, tri):
    """The restatements of (points, tri), computed once per key and shared; a point's row does not depend on the others."""
    if key not in _WANT:
        _WANT[key] = _restatements(points, tri)
    return _WANT[key]


def _rows(want, n):
    return (want[0][:n],) + tuple(tuple(x[:n] for x in w) for w in want[1:])


# ---- special positions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["cube", "cube x6", "ico2"])
def test_special_positions(dev, mesh):
    points, tri = me.special_points(mesh), _triangles(mesh)
    want = _want(("special", mesh), points, tri)
    assert (want[0] == 0).any() and (want[0] < 0).any() and (want[0] > 0).any()
    if mesh == "cube x6":                                        # every tie across the chunks goes to the first copy
        assert tri.shape[0] == 72 and int(want[1][2].max()) < 12 and int(want[1][2].min()) >= 0
    _same(_device_calls(points, tri, dev), want)


# ---- partitions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", me.BLOCK_SIZES)
def test_point_counts_around_a_workgroup(dev, n):
    tri = _triangles("soup")
    want = _want("blocks", _POINTS[:me.BLOCK_SIZES[-1]], tri)
    _same(_device_calls(_POINTS[:n], tri, dev), _rows(want, n))


@pytest.mark.parametrize("n", [65, 3])
@pytest.mark.parametrize("T", me.SOUP_SIZES)
def test_triangle_counts_around_the_chunk_granule(dev, T, n):
    tri = me.soup_of(T)
    assert tri.shape[0] == T
    want = _want(("granule", T), _POINTS[:65], tri)
    _same(_device_calls(_POINTS[:n], tri, dev), _rows(want, n))


@pytest.mark.parametrize("extra", [0, 1])
def test_one_pass_exactly_and_one_triangle_more(dev, extra):
    tri, points = me.pass_mesh(extra), me.pass_points()
    assert tri.shape[0] == me.PASS + extra and points.shape[0] == 65
    want = _want(("pass", extra), points, tri)
    if extra:                                                    # the last triangle, alone in its pass, wins the aimed point
        assert want[1][2][64] == me.PASS and want[2][2][64] == me.PASS and (want[1][2][:64] < me.PASS).all()
    _same(_device_calls(points, tri, dev), want)


def test_one_chunk_per_pass_over_two_passes(dev):
    """N = 2047 * 512 + 1 is the smallest N for which mesh_chunks() takes one chunk whatever T (kMeshTargetBlocks = 2048
    workgroups of 512 points; the constant is local to mesh_sdf.hip, hence restated here): with PASS + 1 triangles the
    accumulators are fed by two passes of one chunk each, the second holding one triangle."""
    from shacira_amd import hip_ops
    points, subset = me.one_chunk_points()
    tri = me.pass_mesh(1)
    n = points.shape[0]
    assert n == 2047 * 512 + 1 and tri.shape[0] == me.PASS + 1
    # the restatement's signed call is its unsigned one with the sign of its sdf: put together here, the stabbing runs once
    want_sdf, unsigned = ref.mesh_sdf_ref(points[subset], tri), cref.mesh_closest_ref(points[subset], tri, signed=False)
    want = (want_sdf, (np.where(np.signbit(want_sdf), -unsigned[0], unsigned[0]),) + unsigned[1:], unsigned)
    assert want[2][2][2] == me.PASS                              # row N - 1 is won by the second pass
    p, t = torch.from_numpy(points).to(dev), torch.from_numpy(tri).to(dev)
    sdf = hip_ops.mesh_sdf(p, t)
    got = [sdf.cpu().numpy()[subset]]
    for signed in (True, False):
        dist, hit, tidx = hip_ops.mesh_closest(p, t, signed=signed)
        assert torch.equal(dist.view(torch.int32), (sdf if signed else sdf.abs()).view(torch.int32))      # all N rows
        got.append((dist.cpu().numpy()[subset], hit.cpu().numpy()[subset], tidx.cpu().numpy()[subset]))
        assert int(tidx.min()) >= 0 and int(tidx.max()) == me.PASS
    _same(tuple(got), want)


# ---- slivers ----------------------------------------------------------------------------------------------------------------
def test_slivers_in_a_soup(dev):
    tri, index = me.sliver_mesh()
    points = me.sliver_points()
    want = _restatements(points, tri)
    got = _device_calls(points, tri, dev)
    _same(got, want)
    for _, _, tidx in got[1:]:                                   # a build that flushed denormals would drop the first
        assert (tidx == index["needle 1e-20"]).any() and (tidx == index["needle 1e-12"]).any()
        assert (tidx == index["near-collinear"]).any() and not (tidx == index["collinear"]).any()


# ---- non-finite -------------------------------------------------------------------------------------------------------------
def test_non_finite_points_and_triangles(dev):
    """The closest-point contract fixes the unsigned call on every row: a NaN or infinite d2 never wins, and a row without a
    winner gives dist = +inf, tidx = -1, hit = p (a NaN matches a NaN). The sign of such a row, and every sign once a vertex
    is not finite, is unspecified and stays unasserted. Nothing may fault: every call's output is read back."""
    points, soup, tri, finite = me.non_finite()
    # non-finite triangles and points: the unsigned call on every row; the signed calls by their magnitude on the finite rows
    want = cref.mesh_closest_ref(points, tri, signed=False)
    sdf, signed, unsigned = _device_calls(points, tri, dev)
    assert np.array_equal(_bits(unsigned[0]), _bits(want[0])) and np.array_equal(unsigned[2], want[2])
    assert np.array_equal(unsigned[1], want[1], equal_nan=True)
    assert np.array_equal(_bits(unsigned[1][finite]), _bits(want[1][finite]))
    assert np.isposinf(unsigned[0][~finite]).all() and (unsigned[2][~finite] == -1).all()
    assert np.array_equal(_bits(np.abs(sdf[finite])), _bits(want[0][finite]))
    assert np.array_equal(_bits(np.abs(signed[0][finite])), _bits(want[0][finite]))
    assert np.array_equal(_bits(signed[1][finite]), _bits(want[1][finite]))
    assert np.array_equal(signed[2][finite], want[2][finite])
    # finite triangles, the same points: every finite row of all three calls
    _same(_device_calls(points, soup, dev), _restatements(points, soup), finite)
    got = _device_calls(points, soup, dev)[2]
    want = cref.mesh_closest_ref(points, soup, signed=False)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1], equal_nan=True)
