"""compute_sdf on the MI355X: the fused HIP kernel of mesh_sdf.hip against the numpy restatement of its contract
(tests/mesh_sdf_ref.py). Equality is BITWISE (np.array_equal on the fp32 bit patterns) and every point is compared: the
contract fixes the operation sequence, and the minimum and the stab flags are order-free, so no partition of the triangles may
change a bit.

The restatement is evaluated once per mesh for the largest batch and sliced for the smaller ones (a point's value does not
depend on the other points). Analytic bound of the 2^20 + 3 case: |sdf - box distance| <= 4 eps, as in test_mesh_cpu.py.
Kernel constants (include/shacira_hip.h): triangle passes of SHACIRA_MESH_SDF_PASS_TRIANGLES, chunk lengths that are multiples
of SHACIRA_MESH_SDF_CHUNK_GRANULE.
"""
import numpy as np
import pytest
import torch

import mesh_sdf_ref as ref
from mesh_sdf_ref import SIZES, _POINTS, _bits, _triangles

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_CASES = {}


def _case(name):
    """(triangles, restatement of _POINTS against them), computed once."""
    if name not in _CASES:
        tri = _triangles(name)
        _CASES[name] = (tri, ref.mesh_sdf_ref(_POINTS, tri))
    return _CASES[name]


def _gpu(points, tri, dev):
    from shacira_amd import hip_ops
    out = hip_ops.mesh_sdf(torch.from_numpy(points).to(dev), torch.from_numpy(tri).to(dev))
    assert out.dtype == torch.float32 and tuple(out.shape) == (points.shape[0],) and out.device == dev
    return out.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mesh,count", [("one", 1), ("cube", 12), ("soup", 37), ("ico2", 320)])
def test_kernel_equals_the_restatement_bitwise(dev, mesh, count, n):
    tri, want = _case(mesh)
    assert tri.shape[0] == count
    got = _gpu(_POINTS[:n], tri, dev)
    assert np.array_equal(_bits(got), _bits(want[:n]))


def test_chunk_tail_across_two_passes(dev):
    from shacira_amd import _lib
    tri = _triangles("ico5+1")
    T = tri.shape[0]
    assert T > _lib.MESH_SDF_PASS_TRIANGLES and T % _lib.MESH_SDF_CHUNK_GRANULE == 1
    assert (T - _lib.MESH_SDF_PASS_TRIANGLES) % _lib.MESH_SDF_CHUNK_GRANULE == 1
    points = _POINTS[:65]
    want = ref.mesh_sdf_ref(points, tri)
    assert (want < 0).any() and (want > 0).any()
    assert np.array_equal(_bits(_gpu(points, tri, dev)), _bits(want))


def test_few_points_many_triangles(dev):
    tri = _triangles("ico4")
    assert tri.shape[0] == 5120
    points = np.asarray([[0.05, -0.1, 0.2], [0.9, 0.8, -0.7], [0.0, 0.0, 0.7]], dtype=np.float32)
    want = ref.mesh_sdf_ref(points, tri)
    assert want[0] < 0 < want[1]
    assert np.array_equal(_bits(_gpu(points, tri, dev)), _bits(want))


def test_million_points_against_the_cube(dev):
    n = (1 << 20) + 3
    points = np.random.default_rng(22).uniform(-1, 1, (n, 3)).astype(np.float32)
    tri = _triangles("cube")
    got = _gpu(points, tri, dev)
    exact = ref.box_sdf(points, 0.5)
    err = float(np.abs(got.astype(np.float64) - exact).max())
    print(f"2^20 + 3 points: max |sdf - box| = {err:.3e} (bound {4 * EPS:.3e})")
    assert err <= 4 * EPS
    off = exact != 0
    assert np.array_equal(np.sign(got[off]), np.sign(exact[off]))
    subset = np.random.default_rng(23).choice(n, 4096, replace=False)
    subset[:3] = (0, n - 2, n - 1)
    assert np.array_equal(_bits(got[subset]), _bits(ref.mesh_sdf_ref(points[subset], tri)))


def test_runs_repeat_and_stale_scratch_is_harmless(dev):
    from shacira_amd import hip_ops
    tri, want = _case("ico2")
    p = torch.from_numpy(_POINTS).to(dev)
    t = torch.from_numpy(tri).to(dev)
    first = hip_ops.mesh_sdf(p, t)
    second = hip_ops.mesh_sdf(p, t)
    assert torch.equal(first, second)
    # the cached scratch buffer the next call will be handed, filled with 0xFF (records, minima and flags alike)
    nbytes = int(hip_ops._lib.lib().shacira_mesh_sdf_workspace_bytes(p.shape[0], t.shape[0]))
    ws = hip_ops._workspace(dev, nbytes)
    assert ws is not None and ws.numel() >= nbytes
    ws.fill_(0xFF)
    third = hip_ops.mesh_sdf(p, t)
    assert hip_ops._workspace(dev, nbytes) is ws
    assert torch.equal(first, third)
    assert np.array_equal(_bits(third.cpu().numpy()), _bits(want))


def test_operand_conversion_and_host_path_agree(dev):
    from shacira_amd.wisp.ops.mesh import compute_sdf
    V, F = ref.icosphere(2, 0.7)
    _, want = _case("ico2")
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    wide = torch.zeros((1000, 6), dtype=torch.float32, device=dev)
    wide[:, ::2] = torch.from_numpy(_POINTS[:1000]).to(dev)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    got = compute_sdf(Vd, Fd, view)
    assert tuple(got.shape) == (1000, 1) and got.device == dev and got.dtype == torch.float32
    assert np.array_equal(_bits(got[:, 0].cpu().numpy()), _bits(want[:1000]))
    got64 = compute_sdf(Vd, Fd, torch.from_numpy(_POINTS[:1000]).to(dev).double(), split_size=7)
    assert got64.device == dev and torch.equal(got64, got)
    # mesh on the host, points on the device: the result lives where the points live
    mixed = compute_sdf(torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(_POINTS[:1000]).to(dev))
    assert mixed.device == dev and torch.equal(mixed, got)
    host = compute_sdf(torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(_POINTS[:1000]))
    assert host.device.type == "cpu" and torch.equal(host, got.cpu())


def test_graph_capture_replays_the_eager_bits(dev):
    from shacira_amd import hip_ops
    tri, want = _case("ico2")
    p = torch.from_numpy(_POINTS).to(dev)
    t = torch.from_numpy(tri).to(dev)
    eager = hip_ops.mesh_sdf(p, t).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip_ops.mesh_sdf(p, t)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip_ops.mesh_sdf(p, t)
    for _ in range(2):
        captured.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)
    assert np.array_equal(_bits(eager.cpu().numpy()), _bits(want))


def test_empty_batch_and_empty_mesh(dev):
    from shacira_amd.wisp.ops.mesh import compute_sdf
    V, F = ref.cube(0.5)
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    none = compute_sdf(Vd, Fd, torch.zeros((0, 3), device=dev))
    assert tuple(none.shape) == (0, 1) and none.device == dev and none.dtype == torch.float32
    inf = compute_sdf(Vd, Fd[:0], torch.from_numpy(_POINTS[:65]).to(dev))
    assert tuple(inf.shape) == (65, 1) and bool(torch.isposinf(inf).all())


def test_point_sample_then_compute_sdf(dev):
    from shacira_amd.wisp.ops.mesh import compute_sdf, point_sample
    torch.manual_seed(4)
    V, F = ref.icosphere(2, 0.7)
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    n = 500
    points = point_sample(Vd, Fd, ["trace", "near", "rand"], n)
    assert tuple(points.shape) == (3 * n, 3) and points.device == dev
    sdf = compute_sdf(Vd, Fd, points)
    assert tuple(sdf.shape) == (3 * n, 1) and bool(torch.isfinite(sdf).all())
    on = float(sdf[:n].abs().max())
    print(f"'trace' samples: max |sdf| = {on:.3e} (bound {8 * EPS:.3e})")
    assert on <= 8 * EPS
    assert float(sdf[n:2 * n].abs().max()) < 0.1 and float(sdf[2 * n:].abs().max()) > 0.1
    want = ref.mesh_sdf_ref(points.cpu().numpy(), V[F])
    assert np.array_equal(_bits(sdf[:, 0].cpu().numpy()), _bits(want))
