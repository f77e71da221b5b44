"""The view-shading kernels of shacira_amd/csrc/shade.hip on the MI355X against the fp64 restatement of their contracts
(tests/shade_ref.py, written from include/shacira_hip.h) on the same fp32 inputs, then ``OfflineRenderer`` end to end on the
analytic sphere with the real ``PackedSDFTracer``.

Shapes: n = 1, below and above one workgroup (255, 257) and 1000 (four workgroups, the last one partial); textures 2 x 2 (the
smallest scipy accepts: every sample clamps x0 to mw - 2), 5 x 7 x 4 and 64 x 33 x 3; blur views 1 x 1, 3 x 5 (both below the
radius: the periodic reflection), 17 x 9 and 40 x 70 (more than one workgroup).

u = 2^-24 below is the unit roundoff of fp32: every operator's result is within a factor 1 +- u of the exact one."""
import os

import numpy as np
import pytest
import torch

import shade_ref as R
import sphere_trace_ref as sref

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
VARIATE_TOL = min(2 * 5.685e-7, 1e-5)        # the Box-Muller tolerance of tests/test_gpu_mesh_sample.py
SIZES = [1, 255, 257, 1000]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def unit_rows(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def rotation():
    a, b = 0.7, -0.4
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (rz @ rx).astype(F)


# The uv bound, from the operation count, for |n|, |d| <= 1 (unit rows; mm a rotation), absolute errors in units of u:
#   v = d mm^T       three products and two sums of terms that add up to <= 1: 3 per component (0 without mm)
#   s = n . v        3 of its own, sqrt(3) * 3 inherited: 8.2; p = 2 s is exact: 16.4, |p| <= 2
#   r_k = v_k - p n_k    3 + 16.4 inherited, 2 for the product (|p n_k| <= 2), 3 for the difference (|r_k| <= 3): 24.4;
#                    r_z - 1 adds 4 (|r_z| <= 4): 28.4
#   |r|              sqrt(25^2 + 25^2 + 29^2) = 45.7 inherited; three squares, two sums and the root are 2.5 relative on |r| <= 4.5:
#                    57 in all; m = 2 |r| <= 9 is an exact doubling: 114
#   q = r_x / m      |q| <= 1/2: 25 / m + 114 / (2 m) + 1/2 = 82 / m + 1/2
#   1 - (q + 0.5)    one each on values <= 1; the clamp moves nothing further: 82 / m + 2.5 <= (82 + 22.5) / m since m <= 9
# UV_C = 128 rounds 104.5 up.
UV_C = 128.0


def uv_bound(m):
    return UV_C * U / m


def sampler_bound(mh, mw):
    """x = u (mw - 1) carries (mw - 1) u, fx = x - x0 one more u: M u with M = max(mw, mh). Each weight is a product of two factors
    <= 1 that carry (M + 1) u each, plus its own rounding: (2 M + 3) u. A term w T, T <= 255, carries 255 (2 M + 4) u; four terms and
    three sums of partial sums <= 255 (1 + small): 255 (4 (2 M + 4) + 3) u; over 255 and one rounding of a value <= 1:
    (8 M + 20) u = (8 (M - 1) + 28) u."""
    return (8 * max(mh, mw) + 20) * U


def shade_rows(rng, n):
    """(normal, dirs, expect_exact bool [n]): random unit rows with the oracle's m >= 0.25, and the degenerate rows at the front
    when n allows."""
    normal, dirs = unit_rows(rng, n), unit_rows(rng, n)
    special = np.zeros(n, dtype=bool)
    rows = [
        ((0, 0, 0), (0.3, -0.4, 0.5)),              # normal = 0: r = v - (0, 0, 1)
        ((0, 0, 0), (0, 0, -1)),                    # m = 0: 0 / 0 -> NaN -> uv (0, 0)
        ((np.nan, 0, 1), (0, 0, -1)),               # NaN normal -> uv (0, 0)
        ((0, 0, 1), (1, 0, 0)),                     # v = (1, 0, 0), r = (1, 0, -1): u = 1 - (1 / (2 sqrt 2) + 0.5)
        ((1, 0, 0), (0, 0, -1)),                    # v = (0, 0, 1), dot 0, r = (0, 0, 0) -> m = 0 -> (0, 0)
        ((0, 0, 0), (4, 0, -1)),                    # r = (4, 0, 0), m = 8: u = 1 - (0.5 + 0.5) = 0 exactly, v = 0.5
        ((0, 0, 0), (-4, 0, -1)),                   # u = 1 - (-0.5 + 0.5) = 1 exactly
        ((0, 0, 0), (0, -4, -1)),                   # v = 1 exactly
    ]
    k = min(len(rows), n) if n >= len(rows) else 0
    for i in range(k):
        normal[i], dirs[i] = rows[i]
        special[i] = True
    return normal, dirs, special


def fix_small_m(normal, dirs, special, mm):
    """Rows whose oracle m is below 0.25 become the head-on row n = (0, 0, 1), d = mm^T (0, 0, -1) (m = 4 without mm)."""
    _, m = R.envmap(dirs, normal, mm)
    bad = ~special & ~(m >= 0.25)
    normal[bad] = (0, 0, 1)
    dirs[bad] = (0, 0, -1)
    if mm is not None:
        _, m2 = R.envmap(dirs, normal, mm)
        assert (m2[~special] >= 0.25).all()
    return normal, dirs


TEXTURES = {"2x2x3": (2, 2, 3), "5x7x4": (5, 7, 4), "64x33x3": (64, 33, 3)}


@pytest.mark.parametrize("use_mm", [False, True], ids=["nomm", "mm"])
@pytest.mark.parametrize("tex_name", list(TEXTURES))
@pytest.mark.parametrize("n", SIZES)
def test_matcap_uv_and_sampler_against_fp64(dev, n, tex_name, use_mm):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(n * 7 + len(tex_name) + use_mm)
    mh, mw, mc = TEXTURES[tex_name]
    tex = rng.integers(0, 256, size=(mh, mw, mc), dtype=np.uint8)
    mm = rotation() if use_mm else None
    normal, dirs, special = shade_rows(rng, n)
    if use_mm and special.any():          # a rotated direction is not exact: only the NaN row stays degenerate
        keep = (normal[2].copy(), dirs[2].copy())
        normal[:8], dirs[:8] = unit_rows(rng, 8), unit_rows(rng, 8)
        normal[2], dirs[2] = keep
        special[:] = False
        special[2] = True
    normal, dirs = fix_small_m(normal, dirs, special, mm)
    hit = rng.random(n) < 0.7
    hit[:8] = True
    garbage = ~hit
    normal[garbage] = rng.normal(size=(int(garbage.sum()), 3)).astype(F) * F(1e20)     # missed rows carry garbage normals
    normal[garbage & (np.arange(n) % 2 == 0)] = np.nan
    want = R.shade_view(R.MATCAP, normal, dirs, hit=hit, mm=mm, tex=tex)
    tn = T(normal, dev)
    rgb, uv, rgb8 = hip_ops.shade_view("matcap", normal=tn, dirs=T(dirs, dev), hit=T(hit, dev), matcap=T(tex, dev),
                                       mm=None if mm is None else torch.from_numpy(mm), with_uv=True, with_rgb8=True)
    uv, rgb, rgb8, got_normal = N(uv).astype(np.float64), N(rgb), N(rgb8), N(tn)
    # the coordinates: degenerate rows exactly, the others within UV_C u / m
    if special.any():
        print("degenerate rows, kernel uv:", uv[special].tolist())
        assert np.array_equal(uv[2], np.zeros(2))
    if special.sum() == 8:
        assert np.array_equal(uv[[1, 4]], np.zeros((2, 2)))
        assert uv[5, 0] == 0.0 and uv[6, 0] == 1.0 and uv[7, 1] == 1.0 and uv[5, 1] == 0.5
    live = hit & ~special & np.isfinite(want["m"])
    if live.any():
        err = np.abs(uv[live] - want["uv"][live]).max(axis=1) / uv_bound(want["m"][live])
        print(f"n {n} {tex_name} mm {use_mm}: largest uv error / bound {err.max():.3f}")
        assert err.max() <= 1.0
    rest = hit & special              # m is 0, NaN or >= 2 on these rows
    if rest.any():
        assert np.abs(uv[rest] - want["uv"][rest]).max() <= UV_C * U / 2
    assert ((uv >= 0) & (uv <= 1)).all()
    # step one: the fp64 sampler at the kernel's own coordinates
    at_own = R.sample_matcap(tex, uv)
    err = np.abs(rgb[hit].astype(np.float64) - at_own[hit]).max()
    print(f"largest sampler error {err:.3e} (bound {sampler_bound(mh, mw):.3e})")
    assert err <= sampler_bound(mh, mw)
    # segmentation: missed rows are 1 in both buffers whatever they held; hit rows keep their normal's bits
    assert (rgb[~hit] == 1.0).all() and (got_normal[~hit] == 1.0).all()
    assert np.array_equal(got_normal[hit].view(np.uint32), normal[hit].view(np.uint32))
    assert np.array_equal(rgb8, R.level8(rgb))


@pytest.mark.parametrize("hits", ["none", "all", "absent"])
@pytest.mark.parametrize("n", SIZES)
def test_matcap_with_every_pixel_hit_missed_or_no_mask(dev, n, hits):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(n + 31)
    tex = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    normal, dirs, special = shade_rows(rng, n)
    normal, dirs = fix_small_m(normal, dirs, special, None)
    hit = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "absent": None}[hits]
    tn = T(normal, dev)
    rgb, uv, rgb8 = hip_ops.shade_view("matcap", normal=tn, dirs=T(dirs, dev), hit=None if hit is None else T(hit, dev),
                                       matcap=T(tex, dev), with_uv=True, with_rgb8=True)
    rgb, uv = N(rgb), N(uv).astype(np.float64)
    if hits == "none":
        assert (rgb == 1.0).all() and (N(tn) == 1.0).all() and (N(rgb8) == 255).all()
    else:                                   # nothing is segmented: the normals keep their bits, NaN payloads aside
        assert np.array_equal(np.nan_to_num(N(tn), nan=7.0).view(np.uint32), np.nan_to_num(normal, nan=7.0).view(np.uint32))
        assert np.abs(rgb.astype(np.float64) - R.sample_matcap(tex, uv)).max() <= sampler_bound(5, 7)
        assert np.array_equal(N(rgb8), R.level8(rgb))
    want, m = R.envmap(dirs, normal)        # the coordinates do not depend on the mask
    live = ~special
    assert (np.abs(uv[live] - want[live]).max(axis=1) <= uv_bound(m[live])).all()


def smooth_texture(mh, mw):
    y, x = np.mgrid[0:mh, 0:mw]
    t = np.stack([2 * x + y, 250 - 3 * y, 40 + x + 2 * y], axis=-1)
    return t.astype(np.uint8)


@pytest.mark.parametrize("n", [257, 1000])
def test_matcap_end_to_end_on_a_smooth_texture(dev, n):
    """The colour against the oracle's OWN coordinates. A coordinate error e moves the sample point by e (M - 1) texels per axis,
    and the bilinear surface climbs at most `step` levels per texel along each axis: |dc| <= 2 e (M - 1) step / 255, on top of the
    sampler's own bound."""
    from shacira_amd import hip_ops
    rng = np.random.default_rng(n)
    mh, mw = 33, 64
    tex = smooth_texture(mh, mw)
    t = tex.astype(np.int64)
    step = max(np.abs(np.diff(t, axis=0)).max(), np.abs(np.diff(t, axis=1)).max())
    assert step <= 3
    normal, dirs, special = shade_rows(rng, n)
    special[:] = False
    normal[:8], dirs[:8] = unit_rows(rng, 8), unit_rows(rng, 8)
    normal, dirs = fix_small_m(normal, dirs, special, None)
    want = R.shade_view(R.MATCAP, normal, dirs, tex=tex)
    rgb, _, _ = hip_ops.shade_view("matcap", normal=T(normal, dev), dirs=T(dirs, dev), matcap=T(tex, dev))
    bound = sampler_bound(mh, mw) + 2 * uv_bound(want["m"]) * (max(mh, mw) - 1) * step / 255.0
    err = np.abs(N(rgb).astype(np.float64) - want["rgb"]).max(axis=1) / bound
    print(f"n {n}: largest end-to-end error / bound {err.max():.3f}")
    assert err.max() <= 1.0


@pytest.mark.parametrize("hits", ["none", "all", "mixed"])
@pytest.mark.parametrize("mode", ["rb", "normal"])
@pytest.mark.parametrize("n", SIZES)
def test_rb_and_normal_modes(dev, n, mode, hits):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(n)
    normal = unit_rows(rng, n)
    rgb_in = rng.random((n, 3)).astype(F) * F(1.5) - F(0.25)          # below 0 and above 1: the 8-bit form saturates
    if n > 2:
        normal[1] = np.nan
        rgb_in[2] = (np.nan, np.inf, -np.inf)
    hit = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "mixed": rng.random(n) < 0.5}[hits]
    want = R.shade_view(R.RB if mode == "rb" else R.NORMAL, normal, hit=hit, rgb=rgb_in)
    tn, trgb = T(normal, dev), T(rgb_in, dev)
    rgb, uv, rgb8 = hip_ops.shade_view(mode, normal=tn, hit=T(hit, dev), rgb=trgb if mode == "rb" else None, with_rgb8=True)
    assert uv is None and (mode != "rb" or rgb is trgb)
    got = N(rgb)
    # (x + 1) / 2 is two operators on a value the oracle forms exactly: 2 u relative; rb keeps the bits
    both_nan = np.isnan(got) & np.isnan(want["rgb"])
    with np.errstate(invalid="ignore"):
        ok = both_nan | (got == want["rgb"]) | (np.abs(got - want["rgb"]) <= 2 * U * np.abs(want["rgb"]))
    assert ok.all()
    if mode == "rb":
        assert np.array_equal(got[hit].view(np.uint32), rgb_in[hit].view(np.uint32))
    assert (N(tn)[~hit] == 1.0).all()
    assert np.array_equal(N(tn)[hit].view(np.uint32), normal[hit].view(np.uint32))
    assert np.array_equal(N(rgb8), R.level8(got))


@pytest.mark.parametrize("n", SIZES)
def test_uv_alone_is_spherical_envmap(dev, n):
    from shacira_amd.wisp.ops.geometric import spherical_envmap
    rng = np.random.default_rng(n + 5)
    normal, dirs, special = shade_rows(rng, n)
    normal, dirs = fix_small_m(normal, dirs, special, None)
    want, m = R.envmap(dirs, normal)
    keep = normal.copy()
    tn = T(normal, dev)
    uv = N(spherical_envmap(T(dirs, dev).reshape(n, 1, 3), tn.reshape(n, 1, 3))).astype(np.float64)
    assert uv.shape == (n, 2)
    live = ~special
    if live.any():
        assert (np.abs(uv[live] - want[live]).max(axis=1) <= uv_bound(m[live])).all()
    if special.any():                 # m is 0, NaN or >= 2 on these rows
        assert np.abs(uv[special] - want[special]).max() <= UV_C * U / 2
        assert np.array_equal(uv[[1, 2, 4]], np.zeros((3, 2)))
    assert np.array_equal(N(tn).view(np.uint32), keep.view(np.uint32))        # nothing is written back


# ---- shadow rays ----------------------------------------------------------------------------------------------------------------
LIGHT, MIN_Y = (1.5, 4.5, 1.5), -2.0


def shadow_inputs(rng, n):
    """Rays from around (0, 1, 3) looking down and up, a traced buffer with hits at depth 1..6 and misses at depth 0, and the rows
    that can go wrong at the front (exactly representable numbers: their plane_t has no rounding)."""
    o = (rng.normal(size=(n, 3)) * 0.5 + (0, 1, 3)).astype(F)
    d = unit_rows(rng, n)
    hit = rng.random(n) < 0.5
    depth = np.where(hit, rng.random(n) * 5 + 1, 0).astype(F)
    xyz = np.where(hit[:, None], o + d * depth[:, None], 0).astype(F)
    normal = np.where(hit[:, None], unit_rows(rng, n), 0).astype(F)
    rows = [
        # o, d, depth, hit
        ((0, 1, 0), (1, 0, 0), 4, 1),          # d.y = 0, o.y != min_y: plane_t = -inf... (3 / -0) -> no plane hit
        ((0, -2, 0), (1, 0, 0), 4, 1),         # d.y = 0, o.y = min_y: 0 / 0 = NaN -> no plane hit
        ((0, 1, 0), (0, 1, 0), 4, 1),          # the plane behind the origin: plane_t = -3
        ((0, 1022, 0), (0, -2, 0), 600, 1),    # plane_t = 512 >= 500
        ((0, 998, 0), (0, -2, 0), 600, 1),     # plane_t = 500 exactly: not < 500
        ((0, 2, 0), (0, -1, 0), 4, 1),         # plane_t = 4 == depth: strict <, the surface keeps the pixel
        ((0, 2, 0), (0, -1, 0), 4.5, 1),       # plane_t = 4 < depth: the plane takes the pixel over
        ((0, 2, 0), (0, -1, 0), 0, 0),         # a miss with depth 0: plane_t < 0 is false, no plane hit
        ((0, 0, 0), (0.5, -0.5, 0), 8, 1),     # plane_t = 4, xyz = (2, -2, 0)
    ]
    k = len(rows) if n >= len(rows) else 0
    for i in range(k):
        o[i], d[i], depth[i], hit[i] = rows[i][0], rows[i][1], rows[i][2], bool(rows[i][3])
        xyz[i] = (o[i].astype(np.float64) + d[i].astype(np.float64) * depth[i]).astype(F) if hit[i] else 0
        normal[i] = (0, 1, 0) if hit[i] else 0
    return o, d, depth, xyz, normal, hit, k


def shadow_bands(o, d, want, normal_norm):
    """The fp32 bounds on the two deciding quantities and on the float outputs, per row.
    plane_t = (o_y - min_y) / rate: a difference and a quotient of exact inputs, 2 u |plane_t|; the band is twice that. A taken-over
    pixel's xyz_k = o_k + d_k plane_t carries 4 u A, A = max_k(|o_k| + |d_k plane_t|); so_k one product (exact constant times
    normal, u) and a sum: + 2 u (|xyz_k| + 0.01); x_k = (light_k + 0.01 g_k) - so_k: 0.01 VARIATE_TOL from g and 3 u B more, with
    B = max(|light|, |so|) + 0.06: in all E = 4 u A + 0.01 VARIATE_TOL + 6 u B per component. A unit vector made from a vector
    within sqrt(3) E of x moves by at most 2 sqrt(3) E / |x|, the root and the quotients add 3 u; the dot product with the normal,
    three products and two sums: |n| (sqrt(3) (2 sqrt(3) E / |x| + 3 u) + 3 u) <= |n| (6 E / |x| + 16 u)."""
    t = np.where(np.isfinite(want["plane_t"]), np.abs(want["plane_t"]), 0.0)
    plane_band = 4 * U * t
    A = (np.abs(o.astype(np.float64)) + np.abs(d.astype(np.float64)) * t[:, None]).max(axis=1)
    A = np.where(want["plane_hit"], A, 0.0)
    B = np.maximum(np.abs(LIGHT).max(), np.abs(want["so"]).max(axis=1)) + 0.06
    E = 4 * U * A + 0.01 * VARIATE_TOL + 6 * U * B
    x = (np.asarray(LIGHT) + 0.01 * want["g"]) - want["so"]
    xn = np.linalg.norm(x, axis=1)
    sd_tol = 2 * np.sqrt(3) * E / xn + 3 * U
    light_band = normal_norm * (6 * E / xn + 16 * U)
    return plane_band, light_band, E, sd_tol


@pytest.mark.parametrize("n", SIZES)
def test_shadow_rays_against_fp64(dev, n):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(100 + n)
    o, d, depth, xyz, normal, hit, k = shadow_inputs(rng, n)
    want = R.shadow_rays(o, d, depth, xyz, normal, hit, LIGHT, MIN_Y, seed=11)
    plane_band, light_band, E, sd_tol = shadow_bands(o, d, want, np.linalg.norm(want["normal"], axis=1))
    # the rows built from exactly representable numbers: their difference and quotient have no rounding in fp32 either, so
    # they are decided exactly even where plane_t sits ON a threshold (500, the depth)
    exact = np.arange(n) < k
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = o[:, 1].astype(np.float64) - MIN_Y
        assert (diff[exact] == diff[exact].astype(F)).all()
        pt = want["plane_t"][exact]
        assert (np.isnan(pt) | (pt == pt.astype(F))).all()
    plane_sure = (want["plane_margin"] > plane_band) | exact
    light_sure = plane_sure & (np.abs(want["light_dot"]) > light_band)
    # a zero normal (a miss the plane did not take) has dot == 0 exactly on both sides: sure
    zero_normal = plane_sure & ~(want["normal"] != 0).any(axis=1)
    light_sure |= zero_normal
    share = 1.0 - min(plane_sure.mean(), light_sure.mean())
    print(f"n {n}: rows inside a band {share:.4f}")
    assert share <= 0.01
    assert plane_sure[:k].all() and light_sure[:k].all()                   # the exact rows are never in a band
    td, tx, tn, th = T(depth, dev), T(xyz, dev), T(normal, dev), T(hit, dev)
    so, sd, light_hit, plane_hit = hip_ops.shadow_rays(T(o, dev), T(d, dev), td, tx, tn, th, LIGHT, MIN_Y, seed=11)
    assert light_hit.dtype == torch.bool and plane_hit.dtype == torch.bool
    assert np.array_equal(N(plane_hit)[plane_sure], want["plane_hit"][plane_sure])
    assert np.array_equal(N(light_hit)[light_sure], want["light_hit"][light_sure])
    if k:
        assert N(plane_hit)[:k].tolist() == [False, False, False, False, False, False, True, False, True]
        assert np.array_equal(N(tx)[8], np.array([2, -2, 0], dtype=F)) and N(td)[8] == 4.0
    s = plane_sure
    assert np.array_equal(N(th)[s], want["hit"][s])
    assert not N(th)[N(plane_hit)].any()                                    # a pixel the plane took over is no longer hit
    assert (np.abs(N(td)[s] - want["depth"][s]) <= 2 * U * np.abs(want["depth"][s])).all()
    tol_xyz = (4 * U * np.where(want["plane_hit"], (np.abs(o) + np.abs(d) * np.abs(want["depth"])[:, None]).max(axis=1), 0))
    assert (np.abs(N(tx)[s] - want["xyz"][s]).max(axis=1) <= tol_xyz[s]).all()
    kept = s & ~want["plane_hit"]
    assert np.array_equal(N(tx)[kept].view(np.uint32), xyz[kept].view(np.uint32))       # untouched rows keep their bits
    assert np.array_equal(N(tn)[kept].view(np.uint32), normal[kept].view(np.uint32))
    assert np.array_equal(N(tn)[s & want["plane_hit"]], want["normal"][s & want["plane_hit"]].astype(F))
    so_tol = tol_xyz + 2 * U * (np.abs(want["so"]).max(axis=1) + 0.01)
    assert (np.abs(N(so)[s] - want["so"][s]).max(axis=1) <= so_tol[s]).all()
    err = np.abs(N(sd)[s] - want["sd"][s]).max(axis=1) / sd_tol[s]
    print(f"largest shadow direction error / bound {err.max():.3f}")
    assert err.max() <= 1.0


def test_shadow_jitter_is_the_philox_stream_of_the_seed(dev):
    """With the light and the shadow origin at 0 the direction is g / |g|: all the entry point shows of g. A unit vector made from
    a vector within sqrt(3) VARIATE_TOL of g moves by at most 2 sqrt(3) VARIATE_TOL / |g|; the product 0.01 g, the root and the
    quotients add 4 u."""
    from shacira_amd import hip_ops
    n = 1000
    z3, z1 = np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F)
    up = np.tile(np.array([0, 1, 0], dtype=F), (n, 1))

    def run(seed):
        out = hip_ops.shadow_rays(T(z3, dev), T(up, dev), T(z1, dev), T(z3, dev), T(z3, dev), T(np.zeros(n, bool), dev),
                                  (0.0, 0.0, 0.0), MIN_Y, seed=seed)
        assert not N(out[3]).any()
        return N(out[1])
    a, again, b = run(3), run(3), run(4)
    assert np.array_equal(a.view(np.uint32), again.view(np.uint32))
    assert (np.abs(a - b).max(axis=1) > 1e-3).mean() > 0.99
    for seed, got in ((3, a), (4, b), ((1 << 40) + 3, run((1 << 40) + 3))):
        g = R.shadow_gaussians(n, seed)
        gn = np.linalg.norm(g, axis=1)
        err = np.abs(got - g / gn[:, None]).max(axis=1) / (2 * np.sqrt(3) * VARIATE_TOL / gn + 4 * U)
        print(f"seed {seed}: largest jitter direction error / bound {err.max():.3f}")
        assert err.max() <= 1.0
    assert not np.array_equal(a, run((1 << 40) + 3))                       # the seed's high word is part of the key


# ---- shadow apply ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["lit", "occluded", "one", "random"])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 9), (40, 70)])
def test_shadow_apply_against_fp64(dev, H, W, C, pattern):
    from shacira_amd import hip_ops
    rng = np.random.default_rng(H * 100 + W)
    n = H * W
    occluded = {"lit": np.zeros(n, bool), "occluded": np.ones(n, bool), "one": np.arange(n) == n // 2,
                "random": rng.random(n) < 0.4}[pattern]
    light_hit = np.ones(n, bool) if pattern != "random" else rng.random(n) < 0.8
    rgb = (rng.random((n, C)) * 2 - 0.5).astype(F)
    want = R.shadow_apply(H, W, occluded, light_hit, rgb)
    trgb = T(rgb, dev)
    shadow = hip_ops.shadow_apply(H, W, T(occluded, dev), T(light_hit, dev), trgb)
    got = N(trgb)
    assert shadow.dtype == torch.bool and np.array_equal(N(shadow), want["shadow"])
    # 17 products and 16 sums per axis on values <= 1, the tap's and the map's own rounding, the final product
    tol = (2 * 17 + 6) * U * np.abs(rgb[:, :3].astype(np.float64))
    err = np.abs(got[:, :3] - want["rgb"][:, :3])
    print(f"{H}x{W} C{C} {pattern}: largest error / bound {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert (err <= tol).all()
    if C == 4:
        assert np.array_equal(got[:, 3].view(np.uint32), rgb[:, 3].view(np.uint32))
    if pattern == "lit":
        assert (np.abs(got[:, :3] - rgb[:, :3]) <= 40 * U * np.abs(rgb[:, :3])).all()


# ---- slice colours --------------------------------------------------------------------------------------------------------------
def ulp_neighbours(x, k=3):
    """float32 x and its k neighbours on each side."""
    out, lo, hi = [F(x)], F(x), F(x)
    for _ in range(k):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return out


def slice_thresholds():
    """Every value of dd at which a rule of the colour map switches, in float32: the surface band's two ends, the
    inside / outside switch, the clip ends, then each isoline's two ends and its centre."""
    dds = [F(0.5) - F(0.004), F(0.5) + F(0.004), F(0.5), F(0.0), F(1.0)]
    for i in range(50):
        c = F(0.02 * i)
        dds += [c - F(0.0015), c + F(0.0015), c]
    return dds


def d_around(dd_t):
    """The float32 d whose dd = (d + 1) / 2, before the clip, are the three closest values on each side of ``dd_t`` that any
    float32 d reaches, and ``dd_t`` itself where one does. dd moves only when d + 1 does, so d is stepped on the grid of d + 1
    (2^-24 wide below 1, 2^-23 up to 2, 2^-22 above), not by d's own ulp, which near d = 0 is far too fine to move dd at
    all. For dd_t in (0.25, 1] these are dd_t and its float32 neighbours; below 0.25 dd is a multiple of 2^-25 (2^-24 below
    0), coarser than its own ulp, so dd_t itself is mostly out of reach. Returns (d, dd), ascending, 6 or 7 long."""
    d0 = np.float64(F(np.float64(dd_t) * 2.0 - 1.0))        # onto d's grid first: a d0 half-way would round in pairs below
    cand = np.unique((d0 + np.arange(-16, 17) * 2.0 ** -24).astype(F))
    dd, first = np.unique((cand + F(1)) / F(2), return_index=True)
    at = int(np.searchsorted(dd, F(dd_t)))
    end = at + 3 + int(dd[at] == F(dd_t))
    assert at >= 3 and end <= dd.shape[0]
    return cand[first[at - 3:end]], dd[at - 3:end]


def slice_inputs(n):
    """d whose dd sits on every threshold and on its three nearest reachable values on either side, NaN, the infinities and
    -0, then a ramp over [-1.5, 1.5]. Fewer than all of them (n = 257): an even stride through the list, which still lands
    within 3 steps of every threshold but takes about one in four of the neighbours; n = 4096 holds them all."""
    d = [d_around(dd_t)[0] for dd_t in slice_thresholds()]
    d = np.concatenate(d + [np.array([np.nan, np.inf, -np.inf, -0.0], dtype=F)])
    if n == 1:
        return np.array([0.25], dtype=F)
    if n <= d.shape[0]:
        return d[np.round(np.linspace(0, d.shape[0] - 1, n)).astype(np.int64)]
    return np.concatenate([d, np.linspace(-1.5, 1.5, n - d.shape[0]).astype(F)])


def test_slice_inputs_straddle_every_threshold():
    """No GPU work: the inputs themselves. Around each threshold the dd are distinct and three lie strictly on each side;
    wherever dd's own float32 neighbours can be reached (dd > 0.25) they are exactly the threshold and those neighbours, and
    below that they are consecutive points of the grid that dd lives on."""
    for dd_t in slice_thresholds():
        d, dd = d_around(dd_t)
        assert d.dtype == F and dd.dtype == F
        got = (d + F(1)) / F(2)
        assert np.array_equal(got, dd) and np.unique(dd).shape[0] == dd.shape[0]
        assert (dd[:3] < F(dd_t)).all() and (dd[-3:] > F(dd_t)).all()
        assert dd.shape[0] == 6 or (dd.shape[0] == 7 and dd[3] == F(dd_t))
        if dd_t > 0.25:
            assert np.array_equal(dd, np.sort(np.array(ulp_neighbours(dd_t), dtype=F)))
        else:
            assert np.array_equal(np.diff(dd.astype(np.float64)), np.where(dd[:-1] < 0, 2.0 ** -24, 2.0 ** -25))
    every = slice_inputs(4096)
    for dd_t in slice_thresholds():
        assert np.isin(d_around(dd_t)[0], every).all()


def slice_class(vis):
    """The class a colour row shows: the four fixed colours are exact constants, anything else is the base ramp."""
    cls = np.full(vis.shape[0], R.SLICE_BASE)
    cls[np.isnan(vis).any(axis=1)] = R.SLICE_NAN
    cls[(vis == np.array([1.0, 0.38, 0.0], dtype=F)).all(axis=1)] = R.SLICE_INSIDE
    cls[(vis == F(0.8)).all(axis=1)] = R.SLICE_LINE
    cls[(vis == 0).all(axis=1)] = R.SLICE_ZERO
    return cls


@pytest.mark.parametrize("n", [1, 257, 4096])
def test_slice_colours_against_the_fp32_contract(dev, n):
    from shacira_amd import hip_ops
    d = slice_inputs(n)
    assert d.shape[0] == n
    want, cls = R.sdf_slice_colors(d)
    got = N(hip_ops.sdf_slice_colors(T(d, dev)))
    assert got.shape == (n, 3)
    if n == 4096:
        assert set(cls.tolist()) == {R.SLICE_BASE, R.SLICE_INSIDE, R.SLICE_LINE, R.SLICE_ZERO, R.SLICE_NAN}
    assert np.array_equal(slice_class(got), cls)
    ok = cls != R.SLICE_NAN
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)).max() if ok.any() else 0.0
    print(f"n {n}: largest colour difference {err:.3e}")
    assert err <= 2.0 ** -22
    # the reference's own accumulation: float64 vis from the float32 blue / yellow
    with np.errstate(invalid="ignore"):
        dd = np.clip((d + F(1)) / F(2), F(0), F(1))
        blue = np.clip((dd - F(0.5)) * F(2), F(0), F(1))
    base = np.zeros((n, 3))
    base[:, 2] = blue
    base += (F(1) - blue)[:, None] * np.array([0.4, 0.3, 0.0])
    base += 0.2
    sel = cls == R.SLICE_BASE
    if sel.any():
        assert np.abs(got[sel] - base[sel]).max() <= 2.0 ** -22


# ---- end to end: OfflineRenderer over the real PackedSDFTracer on the analytic sphere ---------------------------------------------
WIDTH, HEIGHT, MIN_DIS = 24, 16, 0.0003
EYE = [1.5, 1.2, 2.0]


class _Grid:
    """What the tracer asks of a grid: the occupancy structure's raytrace and the level list."""

    def __init__(self, blas, level):
        self.blas, self.active_lods, self.num_lods = blas, [level], 1

    def raytrace(self, rays, level=None, with_exit=False):
        return self.blas.raytrace(rays, level, with_exit=with_exit)


class SphereNef(torch.nn.Module):
    """sdf = |x| - 0.7 with the operator order of sphere_trace_ref.analytic_sdf, evaluated where the coordinates live."""

    def __init__(self, grid):
        super().__init__()
        self.grid = grid

    def sdf(self, coords, lod_idx=None):
        x = coords
        return dict(sdf=(torch.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) - sref.RADIUS)[:, None])

    def forward(self, channels=None, coords=None, lod_idx=None, pidx=None):
        return self.sdf(coords)[channels]

    def get_forward_function(self, channel):
        return lambda x: self.sdf(x)[channel]


@pytest.fixture(scope="module")
def scene(dev):
    """(pipeline, rays of the 24 x 16 view, the tracer's own buffers as numpy): traced once, shared, left unchanged."""
    from shacira_amd.wisp.accelstructs import OctreeAS
    from shacira_amd.wisp.core import Rays
    from shacira_amd.wisp.models.pipeline import Pipeline
    from shacira_amd.wisp.ops.geometric import look_at_rays
    from shacira_amd.wisp.tracers import PackedSDFTracer
    level = 4
    nef = SphereNef(_Grid(OctreeAS(level, sref.occupancy_grid(level, False).to(dev)), level))
    pipeline = Pipeline(nef, PackedSDFTracer(min_dis=MIN_DIS))
    o, d = look_at_rays(EYE, [0, 0, 0], HEIGHT, WIDTH, fov=40.0, device=dev)
    rays = Rays(o.contiguous(), d.contiguous(), dist_min=0, dist_max=10)
    rb = pipeline.tracer(nef, rays=rays)
    traced = {k: N(getattr(rb, k)) for k in ("hit", "normal", "rgb", "xyz", "depth")}
    assert 0.1 < traced["hit"].mean() < 0.9
    return pipeline, rays, traced


def _renderer(**kw):
    from shacira_amd.wisp.offline_renderer import OfflineRenderer
    return OfflineRenderer(render_res=[WIDTH, HEIGHT], **kw)


@pytest.mark.parametrize("mode", ["matcap", "normal", "rb"])
def test_renderer_modes_equal_the_oracle_on_the_tracers_buffers_batched_or_not(scene, dev, mode):
    from shacira_amd.wisp.ops.shaders import default_matcap
    pipeline, rays, traced = scene
    whole = _renderer(shading_mode=mode).render(pipeline, rays)
    batched = _renderer(shading_mode=mode, render_batch=100).render(pipeline, rays)      # 384 rays: 100, 100, 100, 84
    for name in ("rgb", "normal", "hit", "xyz", "depth", "alpha"):
        a, b = getattr(whole, name), getattr(batched, name)
        assert a.shape[0] == WIDTH * HEIGHT and torch.equal(a.reshape(b.shape), b), name
    tex = N(default_matcap())
    hit = traced["hit"]
    want = R.shade_view({"matcap": R.MATCAP, "normal": R.NORMAL, "rb": R.RB}[mode], traced["normal"], N(rays.dirs), hit=hit,
                        tex=tex, rgb=traced["rgb"])
    got, got_normal = N(whole.rgb).astype(np.float64), N(whole.normal)
    assert (got[~hit] == 1.0).all() and (got_normal[~hit] == 1.0).all()
    assert np.array_equal(got_normal[hit].view(np.uint32), traced["normal"][hit].view(np.uint32))
    if mode == "rb":
        assert np.array_equal(N(whole.rgb)[hit].view(np.uint32), traced["rgb"][hit].view(np.uint32))
    elif mode == "normal":
        assert (np.abs(got - want["rgb"]) <= 2 * U * np.abs(want["rgb"])).all()
    else:
        t = tex.astype(np.int64)
        step = max(np.abs(np.diff(t, axis=0)).max(), np.abs(np.diff(t, axis=1)).max())
        with np.errstate(divide="ignore"):
            bound = sampler_bound(*tex.shape[:2]) + 2 * uv_bound(want["m"]) * (max(tex.shape[:2]) - 1) * step / 255.0
        err = (np.abs(got - want["rgb"]).max(axis=1) / bound)[hit]
        print(f"matcap on the sphere: largest error / bound {err.max():.3f}, texture step {step}")
        assert err.max() <= 1.0
        assert np.ptp(got[hit]) > 0.2                       # the sphere is shaded, not flat


def test_renderer_shadows_equal_the_oracle_given_the_same_occlusion(scene, dev):
    from shacira_amd import hip_ops
    from shacira_amd.wisp.core import Rays
    pipeline, rays, traced = scene
    plain = _renderer(shading_mode="normal").render(pipeline, rays)
    shadowed = _renderer(shading_mode="normal", shadow=True, seed=7)
    shadowed.min_y = 0.1               # the plane cuts the sphere: seen from above, the surface below it is behind the plane
    rb = shadowed.render(pipeline, rays)
    # the same two kernels and the tracer by hand, from the unshadowed render
    depth, xyz, normal, hit = (getattr(plain, k).clone().contiguous() for k in ("depth", "xyz", "normal", "hit"))
    so, sd, light_hit, plane_hit = hip_ops.shadow_rays(rays.origins, rays.dirs, depth, xyz, normal, hit, min_y=0.1, seed=7)
    occluded = pipeline.tracer(pipeline.nef, rays=Rays(so, sd, dist_min=0, dist_max=rays.dist_max)).hit
    want = R.shadow_apply(HEIGHT, WIDTH, N(occluded), N(light_hit), N(plain.rgb))
    print(f"plane pixels {int(plane_hit.sum())}, occluded {int(occluded.sum())}, shadowed {int(want['shadow'].sum())}")
    assert plane_hit.any() and want["shadow"].any() and (~want["shadow"]).any()
    assert np.array_equal(N(rb.shadow), want["shadow"])
    assert not N(rb.shadow)[~N(light_hit)].any()
    assert not (N(rb.hit) & N(plane_hit)).any() and (N(plain.hit) & N(plane_hit)).any()
    assert torch.equal(rb.hit, hit) and torch.equal(rb.depth, depth) and torch.equal(rb.xyz, xyz) and torch.equal(rb.normal, normal)
    src = N(plain.rgb).astype(np.float64)
    assert (np.abs(N(rb.rgb) - want["rgb"]) <= (2 * 17 + 6) * U * np.abs(src)).all()
    assert (N(rb.rgb)[want["shadow"]] < N(plain.rgb)[want["shadow"]]).all()
    with pytest.raises(ValueError, match="height \\* width"):
        _renderer(shading_mode="normal", shadow=True).render(pipeline, rays[:100])


def test_render_sdf_writes_pngs_that_read_back(scene, dev, tmp_path):
    import PIL.Image
    from shacira_amd import harness
    from shacira_amd.wisp.tracers import PackedSDFTracer
    pipeline, rays, traced = scene
    out = harness.render_sdf(pipeline.nef, out_dir=str(tmp_path), res=(WIDTH, HEIGHT), views=[dict(f=EYE, t=[0, 0, 0], fov=40.0)],
                             tracer=PackedSDFTracer(min_dis=MIN_DIS))
    assert len(out) == 1 and tuple(out[0].rgb.shape) == (HEIGHT, WIDTH, 3) and out[0].rgb.is_cuda
    img = out[0].image().byte().cpu()
    for name in ("rgb", "normal", "depth"):
        back = np.array(PIL.Image.open(os.path.join(str(tmp_path), f"view0_{name}.png")))
        assert np.array_equal(back, N(getattr(img, name))), name
    assert np.array_equal(N(out[0].hit).reshape(-1), traced["hit"])
    assert img.rgb.float().std() > 10
