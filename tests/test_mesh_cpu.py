"""wisp.ops.mesh without a GPU: the two C entry points' validation, ``compute_sdf`` on host tensors against the numpy
restatement (tests/mesh_sdf_ref.py) bit for bit, analytic anchors of the contract itself, OBJ loading, normalisation and the
samplers.

Bounds (eps = fp32 epsilon):
  cube, half-edge 0.5    |sdf - box distance| <= 4 eps (values are below 1: 4 eps of 1); measured 1.0e-7. The sign equals the
                         analytic sign at every point off the surface.
  icosphere level 3      R = 0.6, r_in = smallest face-plane distance, r_out = largest vertex norm (fp64, from the mesh):
                         |sdf - (|p| - R)| <= (r_out - r_in) + 1e-6 (the surface lies between the two spheres; measured
                         2.70e-3 against 2.72e-3); |p| < r_in is negative, |p| > r_out positive. No point is excluded.
  surface samples        unsigned distance <= 8 eps of the mesh scale (1): three roundings in the barycentric weights, three
                         products and two sums, against a face whose plane the distance is measured from.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_sdf_ref as ref
from conftest import ROOT
from mesh_sdf_ref import _bits
from shacira_amd import _lib
from shacira_amd.wisp.ops import mesh as mesh_ops

EPS = float(np.finfo(np.float32).eps)


def _sdf(V, F, points, **kw):
    out = mesh_ops.compute_sdf(torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(points), **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (points.shape[0], 1) and out.device.type == "cpu"
    return out.numpy()[:, 0]


def _soup_mesh(tri):
    return tri.reshape(-1, 3), np.arange(tri.shape[0] * 3, dtype=np.int64).reshape(-1, 3)


@pytest.fixture(scope="module")
def cube_case():
    V, F = ref.cube(0.5)
    rng = np.random.default_rng(11)
    points = np.concatenate([rng.uniform(-1, 1, (4096, 3)).astype(np.float32), ref.lattice(9)])
    return V, F, points, ref.mesh_sdf_ref(points, V[F])


# ---- the C entry points ---------------------------------------------------------------------------------------------------
def test_library_exports_the_mesh_sdf_symbols():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "shacira_mesh_sdf") and hasattr(handle, "shacira_mesh_sdf_workspace_bytes")
    text = open(os.path.join(ROOT, "include", "shacira_hip.h")).read()
    assert f"#define SHACIRA_MESH_SDF_PASS_TRIANGLES {_lib.MESH_SDF_PASS_TRIANGLES}\n" in text
    assert f"#define SHACIRA_MESH_SDF_CHUNK_GRANULE {_lib.MESH_SDF_CHUNK_GRANULE}\n" in text


def test_mesh_sdf_validation_codes():
    L = _lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first, or N == 0
    f, q = L.shacira_mesh_sdf, L.shacira_mesh_sdf_workspace_bytes
    big = 1 << 30
    assert f(-1, 4, one, one, one, one, big, None) == _lib.EINVAL
    assert f(4, -1, one, one, one, one, big, None) == _lib.EINVAL
    assert f(1 << 31, 4, one, one, one, one, big, None) == _lib.EINVAL
    assert f(4, 4, None, one, one, one, big, None) == _lib.EINVAL
    assert f(4, 4, one, None, one, one, big, None) == _lib.EINVAL
    assert f(4, 4, one, one, None, one, big, None) == _lib.EINVAL
    assert f(4, 4, one, one, one, None, big, None) == _lib.EWORKSPACE
    assert f(4, 4, one, one, one, one, q(4, 4) - 1, None) == _lib.EWORKSPACE
    assert f(0, 4, one, one, one, None, 0, None) == 0                       # N == 0: nothing to do, nothing launched
    assert f(0, 0, None, None, None, None, 0, None) == 0
    assert q(0, 100) == 0 and q(100, 0) == 0 and q(-1, 5) == 0
    record = 352
    assert q(1, 1) == record + 8
    assert q(1000, 37) == 37 * record + 8000
    # the records of one pass only, whatever T; 8 bytes per point
    P = _lib.MESH_SDF_PASS_TRIANGLES
    assert q(1000, P) == q(1000, 10 * P) == P * record + 8000
    sizes = [q(n, 5000) for n in (1, 2, 63, 64, 65, 4099, 1 << 20, (1 << 20) + 3)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)          # monotone in N


# ---- compute_sdf on host tensors = the restatement, bit for bit -----------------------------------------------------------
def test_compute_sdf_soup_bitwise():
    tri = ref.soup(37, seed=3)
    V, F = _soup_mesh(tri)
    points = np.random.default_rng(5).uniform(-1, 1, (500, 3)).astype(np.float32)
    want = ref.mesh_sdf_ref(points, tri)
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(_sdf(V, F, points)), _bits(want))


def test_compute_sdf_cube_bitwise(cube_case):
    V, F, points, want = cube_case
    assert np.array_equal(_bits(_sdf(V, F, points)), _bits(want))


def test_compute_sdf_icosphere_bitwise():
    V, F = ref.icosphere(2)
    points = np.random.default_rng(6).uniform(-1, 1, (2048, 3)).astype(np.float32)
    want = ref.mesh_sdf_ref(points, V[F])
    assert (want < 0).any() and (want > 0).any()
    assert np.array_equal(_bits(_sdf(V, F, points)), _bits(want))


# ---- analytic anchors -------------------------------------------------------------------------------------------------------
def test_cube_matches_the_box_distance(cube_case):
    V, F, points, got = cube_case
    exact = ref.box_sdf(points, 0.5)
    err = float(np.abs(got.astype(np.float64) - exact).max())
    print(f"cube: max |sdf - box| = {err:.3e} (bound {4 * EPS:.3e})")
    assert err <= 4 * EPS
    off = exact != 0
    assert off.sum() > 4000 and (~off).sum() > 0
    assert np.array_equal(np.sign(got[off]), np.sign(exact[off]))


def test_icosphere_lies_between_its_two_spheres():
    R = 0.6
    V, F = ref.icosphere(3, R)
    T = V.astype(np.float64)[F]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    r_in = float(np.abs((n * T[:, 0]).sum(axis=1)).min())
    r_out = float(np.linalg.norm(V.astype(np.float64), axis=1).max())
    points = np.random.default_rng(7).uniform(-1, 1, (4096, 3)).astype(np.float32)
    got = _sdf(V, F, points).astype(np.float64)
    norm = np.linalg.norm(points.astype(np.float64), axis=1)
    err = float(np.abs(got - (norm - R)).max())
    print(f"icosphere 3: max |sdf - (|p| - R)| = {err:.4e} (bound {(r_out - r_in) + 1e-6:.4e})")
    assert err <= (r_out - r_in) + 1e-6
    assert (norm < r_in).sum() > 100 and (norm > r_out).sum() > 100
    assert (got[norm < r_in] < 0).all()
    assert (got[norm > r_out] > 0).all()


# ---- other cases ------------------------------------------------------------------------------------------------------------
def test_empty_mesh_empty_batch_and_split_size(cube_case):
    V, F, points, want = cube_case
    none = _sdf(V, F[:0], points[:17])
    assert np.isposinf(none).all()
    empty = mesh_ops.compute_sdf(torch.from_numpy(V), torch.from_numpy(F), torch.zeros((0, 3)))
    assert tuple(empty.shape) == (0, 1) and empty.dtype == torch.float32
    assert np.array_equal(_bits(_sdf(V, F, points[:300], split_size=7)), _bits(want[:300]))


def test_device_operands_are_required_by_hip_ops():
    from shacira_amd import hip_ops
    with pytest.raises(RuntimeError, match="HIP"):
        hip_ops.mesh_sdf(torch.zeros(4, 3), torch.zeros(2, 3, 3))


# ---- load_obj ---------------------------------------------------------------------------------------------------------------
def test_load_obj_quads_slashes_and_negative_indices(tmp_path, cube_case):
    V, _, points, want = cube_case
    lines = ["# a cube: quads, i/j/k, i//k, i/j and negative indices", "mtllib none.mtl", "o cube"]
    lines += [f"v {x:.1f} {y:.1f} {z:.1f}" for x, y, z in V.tolist()]
    lines += ["vt 0.0 0.0", "vn 0.0 0.0 1.0", "s off"]
    lines += ["f 1/1/1 2/1/1 4/1/1 3/1/1",            # quads of ref.cube, 1-based
              "f 5//1 7//1 8//1 6//1",
              "f 1/1 5/1 6/1 2/1",
              "f 3 4 8 7",
              "f -8 -6 -2 -4",                         # = 1 3 7 5
              "f -7/1/1 -3/1/1 -1/1/1 -5/1/1"]         # = 2 6 8 4
    path = tmp_path / "cube.obj"
    path.write_text("\n".join(lines) + "\n")
    Vl, Fl = mesh_ops.load_obj(str(path))
    assert Vl.dtype == torch.float32 and tuple(Vl.shape) == (8, 3)
    assert Fl.dtype == torch.long and tuple(Fl.shape) == (12, 3)
    assert np.array_equal(Vl.numpy(), V)
    _, Fc = ref.cube(0.5)
    assert np.array_equal(Fl.numpy(), Fc)
    got = mesh_ops.compute_sdf(Vl, Fl, torch.from_numpy(points[:1000])).numpy()[:, 0]
    assert np.array_equal(_bits(got), _bits(want[:1000]))
    with pytest.raises(NotImplementedError, match="texture"):
        mesh_ops.load_obj(str(path), load_materials=True)


# ---- normalize --------------------------------------------------------------------------------------------------------------
def test_normalize_modes():
    rng = np.random.default_rng(8)
    V = torch.from_numpy((rng.uniform(-1, 1, (200, 3)) * [3.0, 1.0, 0.5] + [5.0, -2.0, 1.0]).astype(np.float32))
    F = torch.from_numpy(rng.integers(0, 200, (50, 3)))
    keep = V.clone()
    Vs, Fs = mesh_ops.normalize(V, F, "sphere")
    assert Fs is F and torch.equal(V, keep)
    assert abs(float(Vs.norm(dim=1).max()) - 1.0) <= 4 * EPS
    assert float(((Vs.max(dim=0).values + Vs.min(dim=0).values) / 2).abs().max()) <= 4 * EPS
    Va, _ = mesh_ops.normalize(V, F, "aabb")
    span = Va.max(dim=0).values - Va.min(dim=0).values
    assert float(Va.min()) == -1.0 and float(Va.max()) == 1.0 and int(span.argmax()) == 0
    assert torch.equal(Va.min(dim=0).values, torch.full((3,), -1.0))
    Vp, _ = mesh_ops.normalize(V, F, "planar")
    assert float(Vp[:, 0].min()) == -1.0 and float(Vp[:, 0].max()) == 1.0
    assert float(Vp[:, 2].min()) == -1.0 and float(Vp[:, 2].max()) == 1.0 and float(Vp[:, 1].min()) == 0.0
    Vn, Fn = mesh_ops.normalize(V, F, "none")
    assert Vn is V and Fn is F
    with pytest.raises(ValueError):
        mesh_ops.normalize(V, F, "cube")


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def test_surface_samples_lie_on_their_faces():
    torch.manual_seed(0)
    V, F = ref.icosphere(1)
    samples, normals = mesh_ops.sample_surface(torch.from_numpy(V), torch.from_numpy(F), 2000)
    assert tuple(samples.shape) == (2000, 3) and tuple(normals.shape) == (2000, 3) and samples.dtype == torch.float32
    dist = ref.mesh_sdf_ref(samples.numpy(), V[F], unsigned=True)
    print(f"surface samples: max distance {float(dist.max()):.3e} (bound {8 * EPS:.3e})")
    assert float(dist.max()) <= 8 * EPS
    # the normals are those of faces of the mesh (unnormalised: twice the area long)
    tri = V[F]
    fn = np.cross(tri[:, 0] - tri[:, 1], tri[:, 1] - tri[:, 2])
    gap = np.abs(normals.numpy()[:50, None, :] - fn[None]).max(axis=2).min(axis=1)
    assert float(gap.max()) <= 4 * EPS


def test_faces_are_drawn_in_proportion_to_their_areas():
    torch.manual_seed(1)
    # areas 3 : 1 in the plane z = 0, split by x = 0
    V = torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-6.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    F = torch.tensor([[0, 1, 2], [0, 3, 1]])
    n = 40000
    samples, _ = mesh_ops.sample_surface(V, F, n)
    share = float((samples[:, 0] < 0).float().mean())
    sigma = (0.75 * 0.25 / n) ** 0.5
    assert abs(share - 0.75) <= 5 * sigma, share
    fidx, fn = mesh_ops.random_face(V, F, 100)
    assert tuple(fidx.shape) == (100, 3) and tuple(fn.shape) == (100, 3)
    probs = mesh_ops.area_weighted_distribution(V, F).probs
    assert torch.allclose(probs, torch.tensor([0.75, 0.25]), atol=1e-6)
    assert torch.equal(mesh_ops.per_face_normals(V, F), torch.tensor([[0.0, 0.0, 6.0], [0.0, 0.0, 2.0]]))


def test_near_surface_uniform_and_point_sample():
    torch.manual_seed(2)
    # one large triangle in z = 0: the z offset of a near-surface sample is the noise itself
    V = torch.tensor([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    F = torch.tensor([[0, 1, 2]])
    for variance in (0.01, 0.1):
        near = mesh_ops.sample_near_surface(V, F, 20000, variance=variance)
        assert tuple(near.shape) == (20000, 3)
        assert abs(float(near[:, 2].std()) / variance - 1.0) <= 0.05
    uni = mesh_ops.sample_uniform(5000)
    assert tuple(uni.shape) == (5000, 3) and float(uni.min()) >= -1.0 and float(uni.max()) <= 1.0
    assert float(uni.min()) < -0.99 and float(uni.max()) > 0.99
    pts = mesh_ops.point_sample(V, F, ["trace", "near", "rand"], 300)
    assert tuple(pts.shape) == (900, 3) and pts.dtype == torch.float32
    assert float(pts[:300, 2].abs().max()) == 0.0 and float(pts[300:600, 2].abs().max()) > 0.0
    with pytest.raises(ValueError):
        mesh_ops.point_sample(V, F, ["grid"], 3)


# ---- aliases ----------------------------------------------------------------------------------------------------------------
def test_wisp_alias_exposes_the_mesh_package():
    import sys
    import shacira_amd.wisp as mirror
    saved = {k: v for k, v in sys.modules.items() if k == "wisp" or k.startswith("wisp.")}
    try:
        mirror.install_as_wisp(force=True)
        from wisp.ops.mesh import compute_sdf, point_sample
        assert compute_sdf is mesh_ops.compute_sdf and point_sample is mesh_ops.point_sample
    finally:
        for k in [k for k in sys.modules if k == "wisp" or k.startswith("wisp.")]:
            del sys.modules[k]
        sys.modules.update(saved)
