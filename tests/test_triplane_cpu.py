"""TriplanarGrid without a GPU: the fp64 restatement (tests/triplane_ref.py) against torch's own CPU grid_sample and its
autograd, the module's construction and interface, its registration under ``wisp``, and the validation codes of the
shacira_triplane_* entry points (validation precedes any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplane_ref as tr
from shacira_amd import _lib
from shacira_amd.wisp.models.grids import TriplanarGrid  # noqa: F401  (the feature under test: absent, nothing runs)


def _coords(rng, n, R):
    """inside the cube, on texel lines of resolution R, exactly +-1, and far outside (several reflections)."""
    parts = [rng.uniform(-1, 1, (n, 3)),
             -1 + 2 * rng.integers(0, R + 1, (n // 2, 3)) / R,
             rng.choice([-1.0, 1.0], (n // 4, 3)),
             rng.uniform(-9.5, 9.5, (n // 2, 3)),
             np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 1.0], [3.0, -5.0, 7.0]])]
    c = np.concatenate(parts)
    mix = rng.integers(0, 4, c.shape)          # mix categories within one sample as well
    return np.where(mix == 0, rng.uniform(-1, 1, c.shape), c)


def _torch_triplane(coords, planes, summed):
    """the reference's composition, in fp64 on the host."""
    N = coords.shape[0]
    grid = coords.reshape(1, N, 1, 3)
    per_lod = []
    for lod in planes:
        cols = []
        for p, (a, b) in enumerate(tr.PLANE_AXES):
            s = F.grid_sample(lod[p], grid[..., [a, b]], mode="bilinear", align_corners=True, padding_mode="reflection")
            cols.append(s[0, :, :, 0].T)
        per_lod.append(torch.cat(cols, -1))
    return torch.stack(per_lod).sum(0) if summed else torch.cat(per_lod, -1)


@pytest.mark.parametrize("fdim", [1, 2, 4, 8])
@pytest.mark.parametrize("lods", [[0, 1, 2], [3, 4], [5, 6], [7], [8]])
@pytest.mark.parametrize("summed", [True, False])
def test_restatement_matches_torch_fp64(fdim, lods, summed):
    rng = np.random.default_rng(fdim * 100 + lods[0] * 7 + summed)
    coords = _coords(rng, 64, 2 ** lods[-1])
    planes = [[rng.standard_normal((fdim, 2 ** l + 1, 2 ** l + 1)) for _ in range(3)] for l in lods]
    tp = [[torch.tensor(p[None], requires_grad=True) for p in lod] for lod in planes]
    tc = torch.tensor(coords, requires_grad=True)
    out = _torch_triplane(tc, tp, summed)
    ref = tr.forward(coords, planes, summed)
    np.testing.assert_allclose(ref, out.detach().numpy(), rtol=1e-12, atol=1e-12)
    go = rng.standard_normal(out.shape)
    out.backward(torch.tensor(go))
    gplanes, gc, _ = tr.backward(coords, planes, go, summed)
    for l in range(len(lods)):
        for p in range(3):
            np.testing.assert_allclose(gplanes[l][p], tp[l][p].grad[0].numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(gc, tc.grad.numpy(), rtol=1e-9, atol=1e-9)


def test_fp32_index_math_restates_torch_fp32():
    """index_dtype=float32 gives torch's fp32 CPU op to fp32 rounding of the sums (the GPU tests' reference)."""
    rng = np.random.default_rng(3)
    coords = _coords(rng, 256, 64).astype(np.float32)
    planes = [[rng.standard_normal((4, 65, 65)).astype(np.float32) for _ in range(3)]]
    out = _torch_triplane(torch.tensor(coords), [[torch.tensor(p[None]) for p in planes[0]]], True).numpy()
    ref = tr.forward(coords, planes, True, index_dtype=np.float32)
    scale = tr.abs_forward(coords, planes, True, index_dtype=np.float32)
    assert np.all(np.abs(out - ref) <= 4 * np.finfo(np.float32).eps * scale + 1e-30)


def _draw(seed, fdim, lods, std, bias):
    torch.manual_seed(seed)
    out = {}
    for i, lod in enumerate(lods):
        for name in ("fmx", "fmy", "fmz"):
            out[f"features.{i}.{name}"] = torch.randn(1, fdim, 2 ** lod + 1, 2 ** lod + 1) * std + bias
    return out


def test_module_construction_state_dict_and_draw_order():
    from shacira_amd.wisp.models.grids import TriplanarGrid
    torch.manual_seed(11)
    g = TriplanarGrid(feature_dim=4, base_lod=5, num_lods=4, multiscale_type="sum", feature_std=0.01, feature_bias=0.2)
    expect = _draw(11, 4, [5, 6, 7, 8], 0.01, 0.2)
    sd = g.state_dict()
    assert list(sd.keys()) == list(expect.keys())
    for k, v in expect.items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k
    assert g.feature_dim == 12 and g.num_lods == 4 and g.max_lod == 8 and g.active_lods == [5, 6, 7, 8]
    assert g.num_feat == sum(((2 ** l + 1) ** 2) * 12 * 3 for l in range(5, 9))
    assert g.features[0].fsize == 32 and g.features[0].fdim == 4


def test_module_interface():
    from shacira_amd.wisp.accelstructs import AxisAlignedBBoxAS
    from shacira_amd.wisp.models.grids import TriplanarGrid
    g = TriplanarGrid(feature_dim=2, base_lod=1, num_lods=2, multiscale_type="cat")
    assert g.name() == "Triplanar Grid"
    props = g.public_properties()
    assert list(props) == ["Acceleration Structure", "Feature Dims", "Total LODs", "Active feature LODs", "Interpolation",
                           "Multiscale aggregation", "Pyramid Layer #1", "Pyramid Layer #2"]
    assert props["Feature Dims"] == 6 and props["Total LODs"] == 2 and props["Active feature LODs"] == ["1", "2"]
    assert props["Pyramid Layer #2"] is g.features[1] and g.features[1].public_properties() == {"Resolution": "3x4x4"}
    assert g.features[0].name() == "TriplanarFeatureVolume"
    assert isinstance(g.blas, AxisAlignedBBoxAS) and g.blas.name() == "AABB" and g.blas.max_level == 0
    assert g.supported_blas() == {AxisAlignedBBoxAS}
    g.freeze()
    assert not any(p.requires_grad for p in g.parameters())


def test_interpolation_type_error_and_host_tensors():
    from shacira_amd.wisp.models.grids import TriplanarGrid
    g = TriplanarGrid(feature_dim=2, base_lod=2, interpolation_type="cubic")
    with pytest.raises(ValueError, match="Interpolation mode 'cubic' is not supported"):
        g.interpolate(torch.zeros(4, 3), 0)
    g = TriplanarGrid(feature_dim=2, base_lod=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.interpolate(torch.zeros(4, 3), 0)


def test_reference_layout_state_dict_loads():
    from shacira_amd.wisp.models.grids import TriplanarGrid
    sd = _draw(5, 3, [2, 3], 0.1, 0.0)
    g = TriplanarGrid(feature_dim=3, base_lod=2, num_lods=2)
    g.load_state_dict(sd)
    assert torch.equal(g.features[1].fmz, sd["features.1.fmz"])


def test_install_as_wisp_exposes_the_grid_and_the_aabb():
    import sys

    from shacira_amd import wisp as sw
    saved = {k: v for k, v in sys.modules.items() if k == "wisp" or k.startswith("wisp.")}
    try:
        sw.install_as_wisp(force=True)
        import wisp.accelstructs
        import wisp.models.grids
        assert wisp.models.grids.TriplanarGrid is sw.models.grids.TriplanarGrid
        assert wisp.accelstructs.AxisAlignedBBoxAS().name() == "AABB"
        assert sys.modules["wisp.models.grids.triplanar_grid"].TriplanarFeatureVolume is not None
    finally:
        for k in [k for k in sys.modules if k == "wisp" or k.startswith("wisp.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_triplane_abi_validation_codes():
    L = _lib.lib()
    lods = (ctypes.c_int32 * 2)(5, 6)
    bad = (ctypes.c_int32 * 1)(11)
    one = ctypes.c_void_p(16)            # never dereferenced: validation fails first or N == 0
    ptrs = (ctypes.c_void_p * 6)(*([16] * 6))
    nulls = (ctypes.c_void_p * 6)(16, 16, 16, 0, 16, 16)
    fwd = L.shacira_triplane_forward
    assert fwd(0, 2, lods, 4, one, ptrs, 1, one, None, 0, None) == 0                          # N == 0
    assert fwd(-1, 2, lods, 4, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL               # negative N
    assert fwd(1 << 31, 2, lods, 4, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL          # N >= 2^31
    assert fwd(5, 0, lods, 4, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL                # no LOD
    assert fwd(5, 12, lods, 4, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL               # > SHACIRA_TRIPLANE_MAX_LODS
    assert fwd(5, 1, bad, 4, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL                 # LOD > SHACIRA_TRIPLANE_MAX_LOD
    assert fwd(5, 2, lods, 0, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL                # fdim 0
    assert fwd(5, 2, lods, 33, one, ptrs, 1, one, None, 0, None) == _lib.EINVAL               # fdim > 32
    assert fwd(5, 2, lods, 4, one, ptrs, 2, one, None, 0, None) == _lib.EINVAL                # multiscale flag
    assert fwd(5, 2, lods, 4, None, ptrs, 1, one, None, 0, None) == _lib.EINVAL               # null coords
    assert fwd(5, 2, lods, 4, one, nulls, 1, one, None, 0, None) == _lib.EINVAL               # a null plane
    assert fwd(5, 2, lods, 4, one, None, 1, one, None, 0, None) == _lib.EINVAL                # no plane array
    ws = L.shacira_triplane_forward_workspace_bytes(5, 2, lods, 4, 1)
    if ws:
        assert fwd(5, 2, lods, 4, one, ptrs, 1, one, None, 0, None) == _lib.EWORKSPACE
    bwd = L.shacira_triplane_backward
    need = L.shacira_triplane_backward_workspace_bytes(5, 2, lods, 4, 1, 1)
    assert need >= 5 * 4
    assert L.shacira_triplane_backward_workspace_bytes(5, 2, lods, 4, 1, 2) == 0    # coordinate gradient: a gather
    assert bwd(5, 2, lods, 4, one, None, one, 1, 0, ptrs, None, None, 0, None) == _lib.EINVAL     # no flag
    assert bwd(5, 2, lods, 4, one, None, one, 1, 4, ptrs, None, None, 0, None) == _lib.EINVAL     # unknown flag
    assert bwd(5, 2, lods, 4, one, None, one, 1, 1, nulls, None, None, 0, None) == _lib.EINVAL    # null gradient plane
    assert bwd(5, 2, lods, 4, one, None, one, 1, 2, None, one, None, 0, None) == _lib.EINVAL      # coords flag, no planes
    assert bwd(5, 2, lods, 4, one, ptrs, one, 1, 2, None, None, None, 0, None) == _lib.EINVAL     # no grad_coords
    assert bwd(5, 2, lods, 4, None, None, one, 1, 1, ptrs, None, None, 0, None) == _lib.EINVAL    # null coords
    assert bwd(5, 2, lods, 4, one, None, one, 1, 1, ptrs, None, None, 0, None) == _lib.EWORKSPACE
    assert bwd(5, 2, lods, 4, one, None, one, 1, 1, ptrs, None, one, need - 1, None) == _lib.EWORKSPACE
    assert L.shacira_set_option(b"triplane_layout", 2) == _lib.EINVAL
