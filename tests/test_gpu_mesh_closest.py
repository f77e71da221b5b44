"""closest_point on the MI355X: the fused HIP kernels of shacira_mesh_closest (mesh_sdf.hip) against the numpy restatement of
the contract (tests/mesh_closest_ref.py). Equality is BITWISE on dist and hit (the fp32 bit patterns) and exact on tidx, and
every point is compared: the contract fixes the operation sequence, and the argmin with its lowest-index tie rule, the minimum
and the stab flags are order-free, so no partition of the triangles over lanes, chunks or passes may change a bit.

The restatement is evaluated once per (mesh, signed) for the largest batch and sliced for the smaller ones. How the
restatement itself stands against exact geometry is test_mesh_closest_cpu.py's subject. Kernel constants
(include/shacira_hip.h): triangle passes of SHACIRA_MESH_SDF_PASS_TRIANGLES, chunk lengths that are multiples of
SHACIRA_MESH_SDF_CHUNK_GRANULE. closest_tex on the device against its host result: <= 16 eps, the bound of the CPU file.
"""
import numpy as np
import pytest
import torch

import mesh_closest_ref as cref
import mesh_sdf_ref as ref
from mesh_sdf_ref import SIZES, _POINTS, _bits, _triangles

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
SIGNED = (True, False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_CASES = {}


def _case(name, signed):
    """(triangles, restatement of _POINTS against them), computed once."""
    if (name, signed) not in _CASES:
        tri = _triangles(name)
        _CASES[name, signed] = (tri, cref.mesh_closest_ref(_POINTS, tri, signed=signed))
    return _CASES[name, signed]


def _gpu(points, tri, dev, signed):
    from shacira_amd import hip_ops
    n = points.shape[0]
    dist, hit, tidx = hip_ops.mesh_closest(torch.from_numpy(points).to(dev), torch.from_numpy(tri).to(dev), signed=signed)
    assert dist.dtype == torch.float32 and tuple(dist.shape) == (n,) and dist.device == dev
    assert hit.dtype == torch.float32 and tuple(hit.shape) == (n, 3) and hit.device == dev
    assert tidx.dtype == torch.int32 and tuple(tidx.shape) == (n,) and tidx.device == dev
    return dist.cpu().numpy(), hit.cpu().numpy(), tidx.cpu().numpy()


def _same(got, want, rows=slice(None)):
    assert np.array_equal(_bits(got[0]), _bits(want[0][rows]))
    assert np.array_equal(_bits(got[1]), _bits(want[1][rows]))
    assert np.array_equal(got[2], want[2][rows])


@pytest.mark.parametrize("signed", SIGNED)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mesh,count", [("one", 1), ("cube", 12), ("soup", 37), ("ico2", 320)])
def test_kernel_equals_the_restatement_bitwise(dev, mesh, count, n, signed):
    tri, want = _case(mesh, signed)
    assert tri.shape[0] == count
    _same(_gpu(_POINTS[:n], tri, dev, signed), want, slice(0, n))


@pytest.mark.parametrize("signed", SIGNED)
def test_chunk_tail_across_two_passes(dev, signed):
    from shacira_amd import _lib
    tri = _triangles("ico5+1")
    T = tri.shape[0]
    assert T == 20481 and T > _lib.MESH_SDF_PASS_TRIANGLES and T % _lib.MESH_SDF_CHUNK_GRANULE == 1
    points = _POINTS[:65]
    want = cref.mesh_closest_ref(points, tri, signed=signed)
    # winners in both passes: the index is the mesh-wide one
    assert (want[2] >= _lib.MESH_SDF_PASS_TRIANGLES).any() and (want[2] < _lib.MESH_SDF_PASS_TRIANGLES).any()
    assert int(want[2].max()) < T - 1
    _same(_gpu(points, tri, dev, signed), want)


@pytest.mark.parametrize("signed", SIGNED)
def test_few_points_many_triangles(dev, signed):
    tri = _triangles("ico4")
    assert tri.shape[0] == 5120
    points = np.asarray([[0.05, -0.1, 0.2], [0.9, 0.8, -0.7], [0.0, 0.0, 0.7]], dtype=np.float32)
    want = cref.mesh_closest_ref(points, tri, signed=signed)
    if signed:
        assert want[0][0] < 0 < want[0][1]
    _same(_gpu(points, tri, dev, signed), want)


@pytest.mark.parametrize("signed", SIGNED)
@pytest.mark.parametrize("n", [65, 4099])
def test_ties_across_chunks(dev, n, signed):
    tri, want = _case("cube x6", signed)
    assert tri.shape[0] == 72 and int(want[2].max()) < 12 and int(want[2].min()) >= 0
    _same(_gpu(_POINTS[:n], tri, dev, signed), want, slice(0, n))


def test_million_points_against_the_cube(dev):
    from shacira_amd import hip_ops
    n = (1 << 20) + 3
    points = np.random.default_rng(22).uniform(-1, 1, (n, 3)).astype(np.float32)
    tri = _triangles("cube")
    p, t = torch.from_numpy(points).to(dev), torch.from_numpy(tri).to(dev)
    sdf = hip_ops.mesh_sdf(p, t)
    subset = np.random.default_rng(23).choice(n, 4096, replace=False)
    subset[:3] = (0, n - 2, n - 1)
    for signed in SIGNED:
        dist, hit, tidx = hip_ops.mesh_closest(p, t, signed=signed)
        assert torch.equal(dist.view(torch.int32), (sdf if signed else sdf.abs()).view(torch.int32))
        got = (dist.cpu().numpy()[subset], hit.cpu().numpy()[subset], tidx.cpu().numpy()[subset])
        _same(got, cref.mesh_closest_ref(points[subset], tri, signed=signed))


@pytest.mark.parametrize("signed", SIGNED)
def test_runs_repeat_and_stale_scratch_is_harmless(dev, signed):
    from shacira_amd import _lib, hip_ops
    tri, want = _case("ico2", signed)
    p = torch.from_numpy(_POINTS).to(dev)
    t = torch.from_numpy(tri).to(dev)
    first = hip_ops.mesh_closest(p, t, signed=signed)
    second = hip_ops.mesh_closest(p, t, signed=signed)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    # the cached scratch buffer the next call will be handed, filled with 0xFF (records, keys and flags alike)
    nbytes = int(_lib.lib().shacira_mesh_closest_workspace_bytes(p.shape[0], t.shape[0], int(signed)))
    ws = hip_ops._workspace(dev, nbytes)
    assert ws is not None and ws.numel() >= nbytes
    ws.fill_(0xFF)
    third = hip_ops.mesh_closest(p, t, signed=signed)
    assert hip_ops._workspace(dev, nbytes) is ws
    assert all(torch.equal(a, b) for a, b in zip(first, third))
    _same(tuple(x.cpu().numpy() for x in third), want)


@pytest.mark.parametrize("signed", SIGNED)
def test_graph_capture_replays_the_eager_bits(dev, signed):
    from shacira_amd import hip_ops
    tri, want = _case("ico2", signed)
    p = torch.from_numpy(_POINTS).to(dev)
    t = torch.from_numpy(tri).to(dev)
    eager = tuple(x.clone() for x in hip_ops.mesh_closest(p, t, signed=signed))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip_ops.mesh_closest(p, t, signed=signed)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip_ops.mesh_closest(p, t, signed=signed)
    for _ in range(2):
        for x in captured:
            x.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))
    _same(tuple(x.cpu().numpy() for x in eager), want)


@pytest.mark.parametrize("signed", SIGNED)
def test_host_path_and_device_path_agree(dev, signed):
    from shacira_amd.wisp.ops.mesh import closest_point
    V, F = ref.icosphere(2, 0.7)
    _, want = _case("ico2", signed)
    Vh, Fh, ph = torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(_POINTS[:1000])
    host = closest_point(Vh, Fh, ph, signed=signed)
    device = closest_point(Vh.to(dev), Fh.to(dev), ph.to(dev), signed=signed)
    mixed = closest_point(Vh, Fh, ph.to(dev).double(), signed=signed)          # the results live where the points live
    for got in (device, mixed):
        assert tuple(got[0].shape) == (1000, 1) and tuple(got[1].shape) == (1000, 3) and tuple(got[2].shape) == (1000,)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
        assert all(x.device == dev for x in got)
        assert torch.equal(got[0].cpu().view(torch.int32), host[0].view(torch.int32))
        assert torch.equal(got[1].cpu().view(torch.int32), host[1].view(torch.int32))
        assert torch.equal(got[2].cpu(), host[2])
    _same((device[0][:, 0].cpu().numpy(), device[1].cpu().numpy(), device[2].cpu().numpy()), want, slice(0, 1000))


def test_empty_batch_and_no_candidate(dev):
    from shacira_amd.wisp.ops.mesh import closest_point
    V, F = ref.cube(0.5)
    Vd, Fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    p = torch.from_numpy(_POINTS[:65]).to(dev)
    dist, hit, tidx = closest_point(Vd, Fd, torch.zeros((0, 3), device=dev))
    assert tuple(dist.shape) == (0, 1) and tuple(hit.shape) == (0, 3) and tuple(tidx.shape) == (0,)
    degenerate = torch.tensor([[0, 0, 1], [2, 2, 2]], device=dev)
    for faces in (Fd[:0], degenerate):
        for signed in SIGNED:
            dist, hit, tidx = closest_point(Vd, faces, p, signed=signed)
            assert bool(torch.isposinf(dist).all()) and bool((tidx == -1).all()) and torch.equal(hit, p)


def test_closest_tex_on_device_equals_the_host(dev):
    from shacira_amd.wisp.ops.mesh import closest_tex
    V, F, TV, TF, mats, colours, texture = cref.textured_cube()
    points, quad = cref.face_points()
    host = closest_tex(*(torch.from_numpy(x) for x in (V, F, TV, TF)), mats, torch.from_numpy(points))
    got = closest_tex(*(torch.from_numpy(x).to(dev) for x in (V, F, TV, TF)), mats, torch.from_numpy(points).to(dev))
    assert all(x.device == dev for x in got)
    err = float((got[0].cpu() - host[0]).abs().max())
    print(f"closest_tex: max |device rgb - host rgb| = {err / EPS:.2f} eps (bound 16 eps)")
    assert err <= 16 * EPS
    assert torch.equal(got[1].cpu(), host[1]) and torch.equal(got[2].cpu(), host[2])
    cref.check_closest_tex(got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), points, quad, colours, texture)


def test_neural_sdf_tex_on_a_hash_grid(dev):
    from shacira_amd.wisp.models.grids import HashGrid
    from shacira_amd.wisp.models.nefs import NeuralSDFTex
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(feature_dim=2, num_lods=4, multiscale_type="cat", resolution_dim=3, feature_std=0.1,
                                   codebook_bitwidth=10, min_grid_res=4, max_grid_res=32, blas_level=3)
    nef = NeuralSDFTex(grid, embedder_type="positional", pos_multires=4, hidden_dim=16, num_layers=1).to(dev)
    x = torch.rand(257, 3, device=dev) * 2 - 1
    out = nef(coords=x)
    assert set(out) == {"rgb", "sdf"}
    assert tuple(out["rgb"].shape) == (257, 3) and tuple(out["sdf"].shape) == (257, 1)
    assert float(out["rgb"].min()) > 0 and float(out["rgb"].max()) < 1
    assert torch.equal(nef(channels="sdf", coords=x), out["sdf"])
    assert torch.equal(nef.get_forward_function("rgb")(x, pidx=None), out["rgb"])
    packed = nef(coords=x[:256].reshape(64, 4, 3))
    assert tuple(packed["rgb"].shape) == (64, 4, 3) and tuple(packed["sdf"].shape) == (64, 4, 1)
    (out["rgb"].square().mean() + out["sdf"].square().mean()).backward()
    assert float(grid.codebook.grad.abs().sum()) > 0
    for name, param in nef.decoder.named_parameters():
        assert param.grad is not None and bool(torch.isfinite(param.grad).all()), name
    assert float(nef.decoder.lout.weight.grad.abs().sum()) > 0
