"""closest_point and the textured branch of wisp.ops.mesh without a GPU: ``closest_point`` on host tensors against the numpy
restatement of the contract (tests/mesh_closest_ref.py) bit for bit, the restatement against exact fp64 geometry, the two C
entry points' validation, ``barycentric_coordinates`` / ``sample_tex`` against arrays the reference's own functions returned
(tests/golden/mesh_tex.npz), ``closest_tex``, ``load_obj_materials`` and ``NeuralSDFTex``.

Bounds (eps = fp32 epsilon; the meshes live in [-1, 1]^3, so eps of 1):
  restatement vs fp64     |hit - exact closest point on triangle tidx|, | |p - hit| - dist | and
                          d64(p, triangle tidx) - min over the candidate triangles of d64 are each <= 4 eps, the bound
                          test_mesh_cpu.py uses for distances at this scale; every point, no exclusions. Measured maxima
                          1.52, 1.34 and 0.06 eps. (tidx itself is NOT compared with an fp64 argmin: on closed meshes points
                          nearest to a shared edge tie, and the two pick different faces of the edge.)
  barycentric_coordinates <= 64 eps against the golden: weights in [0, 1], conditioning d00 * d11 / denom <= 4 at angles
                          >= 30 degrees, about ten roundings.
  sample_tex, closest_tex <= 16 eps: colours in [0, 1]; the reference's bilinear sample is within 2.3 eps of an fp64 one.
"""
import ctypes

import numpy as np
import pytest
import torch

import mesh_closest_ref as cref
import mesh_sdf_ref as ref
from conftest import ROOT
from mesh_sdf_ref import _POINTS as POINTS, _bits, _triangles
from shacira_amd import _lib
from shacira_amd.wisp.ops import mesh as mesh_ops

EPS = float(np.finfo(np.float32).eps)


_CASES = {}


def _case(name):
    """(points, triangles, {signed: restatement}), computed once."""
    if name not in _CASES:
        points = ref.lattice(9) if name == "lattice" else POINTS
        tri = _triangles("cube" if name == "lattice" else name)
        _CASES[name] = (points, tri, {s: cref.mesh_closest_ref(points, tri, signed=s) for s in (True, False)})
    return _CASES[name]


def _soup_mesh(tri):
    return tri.reshape(-1, 3), np.arange(tri.shape[0] * 3, dtype=np.int64).reshape(-1, 3)


def _closest(tri, points, **kw):
    V, F = _soup_mesh(tri)
    dist, hit, tidx = mesh_ops.closest_point(torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(points), **kw)
    n = points.shape[0]
    assert dist.dtype == torch.float32 and tuple(dist.shape) == (n, 1) and dist.device.type == "cpu"
    assert hit.dtype == torch.float32 and tuple(hit.shape) == (n, 3)
    assert tidx.dtype == torch.int64 and tuple(tidx.shape) == (n,)
    return dist.numpy()[:, 0], hit.numpy(), tidx.numpy()


MESHES = ["one", "cube", "soup", "ico2", "lattice", "cube x6"]


# ---- closest_point on host tensors = the restatement, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("mesh", MESHES)
def test_closest_point_equals_the_restatement_bitwise(mesh, signed):
    points, tri, want = _case(mesh)
    dist, hit, tidx = _closest(tri, points, signed=signed)
    wd, wh, wi = want[signed]
    assert np.array_equal(_bits(dist), _bits(wd))
    assert np.array_equal(_bits(hit), _bits(wh))
    assert np.array_equal(tidx, wi)
    assert (wi >= 0).all()
    if mesh == "cube x6":        # six copies of every triangle tie exactly: the lowest index wins
        assert tri.shape[0] == 72 and int(wi.max()) < 12


@pytest.mark.parametrize("mesh", MESHES)
def test_dist_has_the_bits_of_compute_sdf(mesh):
    points, tri, want = _case(mesh)
    V, F = _soup_mesh(tri)
    sdf = mesh_ops.compute_sdf(torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(points)).numpy()[:, 0]
    assert np.array_equal(_bits(_closest(tri, points)[0]), _bits(sdf))                  # signed is the default
    assert np.array_equal(_bits(_closest(tri, points, signed=False)[0]), _bits(np.abs(sdf)))
    assert np.array_equal(_bits(want[True][0]), _bits(ref.mesh_sdf_ref(points, tri)))
    assert np.array_equal(_bits(want[False][0]), _bits(ref.mesh_sdf_ref(points, tri, unsigned=True)))
    if mesh in ("cube", "ico2"):
        assert (sdf < 0).any() and (sdf > 0).any()


# ---- the restatement against exact geometry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["one", "cube", "soup", "ico2", "lattice"])
def test_restatement_against_fp64(mesh):
    points, tri, want = _case(mesh)
    dist, hit, tidx = want[False]
    won = tri[tidx].astype(np.float64)
    exact = cref.closest_on_triangle64(points, won[:, 0], won[:, 1], won[:, 2])
    p64 = points.astype(np.float64)
    e_hit = float(np.abs(hit - exact).max())
    e_len = float(np.abs(np.linalg.norm(p64 - hit, axis=1) - dist).max())
    least = cref.distance64(points, tri)[:, cref.candidates(tri)].min(axis=1)
    e_min = float((np.linalg.norm(p64 - exact, axis=1) - least).max())
    print(f"{mesh}: |hit - exact| = {e_hit / EPS:.2f} eps, ||p - hit| - dist| = {e_len / EPS:.2f} eps, "
          f"d64(tidx) - min d64 = {e_min / EPS:.2f} eps (bound 4 eps each)")
    assert e_hit <= 4 * EPS
    assert e_len <= 4 * EPS
    assert e_min <= 4 * EPS


# ---- no candidate, empty batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
def test_no_candidate_and_empty_batch(signed):
    points = POINTS[:65]
    degenerate = ref.soup(37, seed=3)[1:3]                       # two equal vertices; three equal vertices
    assert not cref.candidates(degenerate).any()
    for tri in (degenerate, np.zeros((0, 3, 3), dtype=np.float32)):
        for dist, hit, tidx in (_closest(tri, points, signed=signed), cref.mesh_closest_ref(points, tri, signed=signed)):
            assert np.isposinf(dist).all() and (tidx == -1).all() and np.array_equal(_bits(hit), _bits(points))
    dist, hit, tidx = _closest(_triangles("cube"), np.zeros((0, 3), dtype=np.float32), signed=signed)
    assert dist.shape == (0,) and hit.shape == (0, 3) and tidx.shape == (0,)


# ---- the C entry points ------------------------------------------------------------------------------------------------------
def test_mesh_closest_validation_codes():
    L = _lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first, or N == 0
    f, q = L.shacira_mesh_closest, L.shacira_mesh_closest_workspace_bytes
    big = 1 << 30
    S = _lib.MESH_CLOSEST_SIGNED
    text = open(f"{ROOT}/include/shacira_hip.h").read()
    assert f"#define SHACIRA_MESH_CLOSEST_SIGNED {S}\n" in text
    for flags in (0, S):
        assert f(-1, 4, one, one, flags, one, one, one, one, big, None) == _lib.EINVAL
        assert f(4, -1, one, one, flags, one, one, one, one, big, None) == _lib.EINVAL
        assert f(1 << 31, 4, one, one, flags, one, one, one, one, big, None) == _lib.EINVAL
        assert f(4, 1 << 31, one, one, flags, one, one, one, one, big, None) == _lib.EINVAL
        for null in (2, 3, 5, 6, 7):
            args = [4, 4, one, one, flags, one, one, one, one, big, None]
            args[null] = None
            assert f(*args) == _lib.EINVAL
        assert f(4, 4, one, one, flags, one, one, one, None, big, None) == _lib.EWORKSPACE
        assert f(4, 4, one, one, flags, one, one, one, one, q(4, 4, flags) - 1, None) == _lib.EWORKSPACE
        assert f(4, 0, one, None, flags, one, one, one, one, q(4, 0, flags) - 1, None) == _lib.EWORKSPACE
        assert f(0, 4, one, one, flags, one, one, one, None, 0, None) == 0     # N == 0: nothing to do, nothing launched
        assert f(0, 0, None, None, flags, None, None, None, None, 0, None) == 0
        record = 352
        assert q(0, 100, flags) == 0 and q(-1, 5, flags) == 0 and q(5, 1 << 31, flags) == 0
        assert q(100, 0, flags) == 1600
        assert q(1, 1, flags) == record + 16
        assert q(1000, 37, flags) == 37 * record + 16000
        P = _lib.MESH_SDF_PASS_TRIANGLES
        assert q(1000, P, flags) == q(1000, 10 * P, flags) == P * record + 16000
    for flags in (2, 3, 4, 1 << 30, -1):                                         # any bit but SIGNED
        assert f(4, 4, one, one, flags, one, one, one, one, big, None) == _lib.EINVAL
        assert f(0, 4, one, one, flags, one, one, one, one, big, None) == _lib.EINVAL
        assert q(4, 4, flags) == 0


def test_device_operands_are_required_by_hip_ops():
    from shacira_amd import hip_ops
    with pytest.raises(RuntimeError, match="HIP"):
        hip_ops.mesh_closest(torch.zeros(4, 3), torch.zeros(2, 3, 3))


# ---- barycentric_coordinates and sample_tex against the reference's results --------------------------------------------------
def _golden_materials(g, with_unused=True):
    mats = {0: {"diffuse_texname": torch.from_numpy(g["tex0"])},
            1: {"diffuse": torch.from_numpy(g["diffuse1"])},
            2: {"diffuse_texname": torch.from_numpy(g["tex2"])} if with_unused else None,
            3: {"diffuse": torch.from_numpy(g["diffuse3"]), "diffuse_texname": torch.from_numpy(g["tex3"])}}
    return mats


def test_barycentric_coordinates_against_the_reference(golden):
    golden = golden("mesh_tex.npz")
    P, A, B, C = (torch.from_numpy(golden[k]) for k in ("bary_p", "bary_a", "bary_b", "bary_c"))
    assert P.shape[0] == 257
    L = mesh_ops.barycentric_coordinates(P, A, B, C)
    assert L.dtype == torch.float32 and tuple(L.shape) == (257, 3)
    err = float(np.abs(L.numpy() - golden["bary_l"]).max())
    print(f"barycentric_coordinates: max |L - reference| = {err / EPS:.2f} eps (bound 64 eps)")
    assert err <= 64 * EPS
    assert float(L.min()) >= 0 and float(L.max()) <= 1
    # the clipping: a point outside its triangle keeps weights in [0, 1]
    out = mesh_ops.barycentric_coordinates(A + 2 * (A - B), A, B, C)
    assert float(out.min()) >= 0 and float(out.max()) <= 1


def test_sample_tex_against_the_reference(golden):
    golden = golden("mesh_tex.npz")
    uv, tm = torch.from_numpy(golden["tex_uv"]), torch.from_numpy(golden["tex_tm"])
    assert uv.shape[0] == 257 and float(uv.min()) < 0 and float(uv.max()) > 1          # reflection is exercised
    assert sorted(set(tm.tolist())) == [0, 1, 3]
    before = uv.clone()
    rgb = mesh_ops.sample_tex(uv, tm, _golden_materials(golden))
    assert torch.equal(uv, before)                                                      # Tp is not modified ...
    view = torch.cat([uv, uv], dim=1)[:, 1:3]
    kept = view.clone()
    mesh_ops.sample_tex(view, tm, _golden_materials(golden))
    assert torch.equal(view, kept)                                                      # ... nor is a view
    assert rgb.dtype == torch.float32 and tuple(rgb.shape) == (257, 3)
    err = float(np.abs(rgb.numpy() - golden["tex_rgb"]).max())
    print(f"sample_tex: max |rgb - reference| = {err / EPS:.2f} eps (bound 16 eps)")
    assert err <= 16 * EPS
    assert torch.equal(rgb[tm == 1], torch.from_numpy(golden["diffuse1"]).expand(int((tm == 1).sum()), 3))
    # the material no point uses is skipped: its entry is not even looked at
    again = mesh_ops.sample_tex(uv, tm, _golden_materials(golden, with_unused=False))
    assert torch.equal(again, rgb)
    with pytest.raises(ValueError, match="material"):
        mesh_ops.sample_tex(uv, torch.full_like(tm, -1), _golden_materials(golden))


# ---- closest_tex ---------------------------------------------------------------------------------------------------------------
def test_closest_tex_on_a_textured_cube():
    V, F, TV, TF, mats, colours, texture = cref.textured_cube()
    points, quad = cref.face_points()
    rgb, hit, dist = mesh_ops.closest_tex(*(torch.from_numpy(x) for x in (V, F, TV, TF)), mats, torch.from_numpy(points))
    assert rgb.dtype == torch.float32 and tuple(rgb.shape) == (240, 3)
    assert tuple(hit.shape) == (240, 3) and tuple(dist.shape) == (240, 1)
    cref.check_closest_tex(rgb.numpy(), hit.numpy(), dist.numpy(), points, quad, colours, texture)
    # without texture coordinates the uv is the first two barycentric weights: still every flat face's colour
    rgb2, _, _ = mesh_ops.closest_tex(torch.from_numpy(V), torch.from_numpy(F), torch.zeros((0, 2)), torch.from_numpy(TF),
                                      mats, torch.from_numpy(points))
    assert np.array_equal(rgb2.numpy()[quad != 1], colours[quad[quad != 1]])
    with pytest.raises(ValueError):
        mesh_ops.closest_tex(torch.from_numpy(V), torch.from_numpy(F[:0]), torch.from_numpy(TV), torch.from_numpy(TF[:0]),
                             mats, torch.from_numpy(points))


# ---- load_obj_materials --------------------------------------------------------------------------------------------------------
def test_load_obj_materials(tmp_path):
    from PIL import Image
    V, _ = ref.cube(0.5)
    pixels = np.random.default_rng(43).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    Image.fromarray(pixels).save(tmp_path / "wood.png")
    (tmp_path / "cube.mtl").write_text("# two materials\nnewmtl red\nKd 1.0 0.25 0.0\nKa 0 0 0\n\n"
                                       "newmtl wood\nmap_Kd wood.png\nnewmtl bare\n")
    lines = ["mtllib cube.mtl", "o cube"]
    lines += [f"v {x:.1f} {y:.1f} {z:.1f}" for x, y, z in V.tolist()]
    lines += ["vt 0.0 0.0", "vt 1.0 0.0", "vt 1.0 1.0 0.0", "vt 0.0 1.0", "vn 0.0 0.0 1.0"]
    lines += ["f 1/1/1 2/2/1 4/3/1 3/4/1",            # before any usemtl: material -1
              "usemtl red",
              "f 5//1 7//1 8//1 6//1",                 # no texture coordinates: -1
              "f 1/1 5/2 6/3 2/4",
              "usemtl wood",
              "f 3 4 8 7",
              "f -8/-4 -6/-3 -2/-2 -4/-1",             # = 1/1 3/2 7/3 5/4
              "usemtl unknown",
              "f -7/1/1 -3/2/1 -1/3/1"]                # a triangle, of a material no library defines: -1
    path = tmp_path / "cube.obj"
    path.write_text("\n".join(lines) + "\n")
    Vl, Fl, texv, texf, mats = mesh_ops.load_obj_materials(str(path))
    assert Vl.dtype == torch.float32 and Fl.dtype == torch.long
    assert texv.dtype == torch.float32 and texf.dtype == torch.long
    Vg, Fg = mesh_ops.load_obj(str(path))
    assert torch.equal(Vl, Vg) and torch.equal(Fl, Fg) and tuple(Fl.shape) == (11, 3)
    assert texv.tolist() == [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    quad = [[0, 1, 2], [0, 2, 3]]
    want = ([t + [-1] for t in quad] + [[-1, -1, -1, 0]] * 2 + [t + [0] for t in quad] + [[-1, -1, -1, 1]] * 2
            + [t + [1] for t in quad] + [[0, 1, 2, -1]])
    assert texf.tolist() == want
    assert sorted(mats) == [0, 1, 2]
    assert mats[0]["diffuse"].dtype == torch.float32 and mats[0]["diffuse"].tolist() == [1.0, 0.25, 0.0]
    assert "diffuse_texname" not in mats[0] and "diffuse_texname" not in mats[2]
    assert mats[1]["diffuse"].tolist() == [0.0, 0.0, 0.0] and mats[2]["diffuse"].tolist() == [0.0, 0.0, 0.0]
    image = mats[1]["diffuse_texname"]
    assert image.dtype == torch.float32 and tuple(image.shape) == (3, 5, 3)
    assert np.array_equal(image.numpy(), pixels.astype(np.float32) / np.float32(255.0))
    with pytest.raises(NotImplementedError, match="texture"):
        mesh_ops.load_obj(str(path), load_materials=True)
    # what was loaded feeds closest_tex: the faces of material 'red' answer with its colour
    inner = Fl[2:6]
    assert (texf[2:6, 3] == 0).all()
    centre = Vl[inner].mean(dim=1) * 1.5
    rgb, _, _ = mesh_ops.closest_tex(Vl, Fl, texv, texf, mats, centre)
    assert torch.equal(rgb, mats[0]["diffuse"].expand(4, 3))


# ---- NeuralSDFTex ---------------------------------------------------------------------------------------------------------------
class _GridShape:
    multiscale_type, feature_dim, num_lods = "cat", 2, 4


def test_neural_sdf_tex_channels_and_constructor():
    from shacira_amd.wisp.models import nefs
    assert "NeuralSDFTex" in nefs.__all__
    model = nefs.NeuralSDFTex(grid=_GridShape(), hidden_dim=16)
    assert model.get_supported_channels() == {"rgb", "sdf"}
    assert model.pos_embedder is None and model.decoder_input_dim() == 8             # no position input without an embedder
    assert model.decoder.lout.out_features == 4
    assert model._forward_functions["rgb"] == model._forward_functions["sdf"] == model.rgbsdf
    embedded = nefs.NeuralSDFTex(grid=_GridShape(), embedder_type="positional", pos_multires=4, hidden_dim=16)
    assert embedded.decoder_input_dim() == 8 + 3 + 3 * 4 * 2
    with pytest.raises(NotImplementedError):
        nefs.NeuralSDFTex(grid=_GridShape(), embedder_type="identity")
    with pytest.raises(NotImplementedError):
        nefs.NeuralSDFTex(grid=_GridShape(), activation_type="sin")
    with pytest.raises(Exception, match="not supported"):
        model.get_forward_function("density")
    with pytest.raises(Exception, match="not supported"):
        model(channels=["rgb", "normal"], coords=torch.zeros(2, 3))
    empty = model(coords=torch.zeros(0, 3))
    assert tuple(empty["rgb"].shape) == (0, 3) and tuple(empty["sdf"].shape) == (0, 1)
