"""Mip levels on the MI355X: shacira_image_mip against exact integer sums, shacira_raygen_sums against the host's fp32 chain bit
for bit, NeRFSyntheticDataset(mip=...) against both and, within carried bounds, against the reference's float chain, and the
multiview harness at a mip level. References and bounds: tests/image_mip_ref.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import image_mip_ref as ref
from shacira_amd import _lib, harness, hip_ops, render
from shacira_amd.wisp.accelstructs import ASRaymarchResults
from shacira_amd.wisp.datasets import NeRFSyntheticDataset, SampleRays
from shacira_amd.wisp.tracers import PackedRFTracer

pytestmark = pytest.mark.gpu
K = _lib.RAYGEN_RECORD_FLOATS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def offset_tensor(array, pad, dev):
    """``array`` on the device at ``pad`` elements past an allocation's start: a slice of a flat buffer, contiguous."""
    flat = np.concatenate([np.zeros(pad, array.dtype), array.reshape(-1)])
    t = torch.from_numpy(flat).to(dev)[pad:].view(array.shape)
    assert t.is_contiguous() and t.data_ptr() % 256 == pad * array.dtype.itemsize
    return t


# ---- shacira_image_mip -------------------------------------------------------------------------------------------------------
MIP_CASES = [((1, 2, 2, 4), 1, "random"), ((2, 4, 6, 3), 1, "random"), ((1, 2, 514, 4), 1, "random"),
             ((1, 68, 76, 3), 2, "random"), ((3, 8, 24, 4), 3, "random"), ((1, 16, 48, 4), 4, "full"),
             ((1, 16, 48, 4), 4, "random"), ((1, 8, 8, 1), 2, "random"), ((1, 8, 8, 2), 2, "random"),
             ((2, 12, 20, 4), 2, "random"), ((1, 32, 2080, 4), 4, "random"), ((2, 16, 1040, 4), 3, "random")]


@pytest.mark.parametrize("shape,mip,fill", MIP_CASES)
def test_image_mip_equals_the_integer_sums(dev, shape, mip, fill):
    rng = np.random.default_rng(7)
    img = np.full(shape, 255, np.uint8) if fill == "full" else rng.integers(0, 256, shape, dtype=np.uint8)
    want = ref.block_sums(img, mip)
    if fill == "full":
        assert (want == 65280).all()
    # an aligned base (16-byte loads), a base 4 bytes in (dword loads) and a base 1 byte in (byte loads) where C = 4
    for pad in ((0, 4, 1) if shape[3] == 4 else (0, 1)):
        t = offset_tensor(img, pad, dev)
        got = hip_ops.image_mip(t, mip)
        assert got.dtype == torch.uint16 and got.is_cuda
        assert tuple(got.shape) == (shape[0], shape[1] >> mip, shape[2] >> mip, shape[3])
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (shape, mip, pad)
    one = hip_ops.image_mip(torch.from_numpy(img[0]).to(dev), mip)               # a single [H, W, C] image
    assert tuple(one.shape) == want.shape[1:] and np.array_equal(one.cpu().numpy().astype(np.int64), want[0])


def test_image_mip_writes_into_a_slice_and_checks_its_operands(dev):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (3, 8, 8, 4), dtype=np.uint8)
    out = torch.from_numpy(np.zeros((5, 4, 4, 4), np.uint16)).to(dev)
    hip_ops.image_mip(torch.from_numpy(img).to(dev), 1, out=out[1:4])
    got = out.cpu().numpy().astype(np.int64)
    assert np.array_equal(got[1:4], ref.block_sums(img, 1)) and not got[0].any() and not got[4].any()
    t = torch.from_numpy(img).to(dev)
    for bad in (0, 5):
        with pytest.raises(RuntimeError, match="mip"):
            hip_ops.image_mip(t, bad)
    with pytest.raises(RuntimeError, match="divisible"):
        hip_ops.image_mip(t[:, :6], 2)
    with pytest.raises(RuntimeError, match="uint8"):
        hip_ops.image_mip(t.float(), 1)
    with pytest.raises(RuntimeError):
        hip_ops.image_mip(torch.from_numpy(img), 1)                              # a host tensor


def test_image_mip_error_codes(dev):
    L = _lib.lib()
    src = torch.zeros(64, dtype=torch.uint8, device=dev)
    dst = torch.from_numpy(np.zeros(64, np.uint16)).to(dev)
    s, d = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr())
    call = L.shacira_image_mip
    assert call(s, 1, 4, 4, 4, 1, d, None) == 0
    torch.cuda.synchronize()
    for mip in (0, 5, -1):
        assert call(s, 1, 16, 16, 1, mip, d, None) == _lib.EINVAL               # mip outside 1..4
    for channels in (0, 5):
        assert call(s, 1, 4, 4, channels, 1, d, None) == _lib.EINVAL             # channels outside 1..4
    for v, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert call(s, v, h, w, 4, 1, d, None) == _lib.EINVAL                    # V, H or W <= 0: nothing is launched
    assert call(s, 1, 6, 8, 1, 2, d, None) == _lib.EINVAL                        # H not a multiple of 2^mip
    assert call(s, 1, 8, 6, 1, 2, d, None) == _lib.EINVAL                        # W not a multiple of 2^mip
    assert call(s, 1, 1 << 17, 1 << 16, 1, 1, d, None) == _lib.EINVAL            # (H >> 1) (W >> 1) = 2^31
    assert call(None, 1, 4, 4, 4, 1, d, None) == _lib.EINVAL                     # NULL pointers
    assert call(s, 1, 4, 4, 4, 1, None, None) == _lib.EINVAL
    torch.cuda.synchronize()
    assert not dst.cpu().numpy()[16:].any()                                      # only the one good call wrote


# ---- shacira_raygen_sums ------------------------------------------------------------------------------------------------------
def records(V, dev, seed=0):
    rng = np.random.default_rng(seed)
    rec = np.zeros((V, K), np.float32)
    for v in range(V):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        rec[v, 0:9] = q.reshape(9)
        rec[v, 9:12] = rng.normal(size=3)
        rec[v, 12:16] = 0.4, 0.3, 0.75, -0.5
    return torch.from_numpy(rec).to(dev)


@pytest.mark.parametrize("mip", [1, 2, 3, 4])
def test_raygen_on_sums_equals_the_host_chain(dev, mip):
    D = 255 * 4 ** mip
    n_s = len(ref.s_table(mip))
    H = W = n_s                                                   # one view: pixel (i, j) = (S_colour i, S_alpha j)
    rec = records(1, dev)
    o0, d0, none_rgb, none_mask = hip_ops.raygen(rec, W, H)       # the rays without images: what the sums must not change
    assert none_rgb is None and none_mask is None
    for channels in (4, 3):
        px = ref.s_pixels(mip, channels)
        sums = px.astype(np.uint16).reshape(1, H, W, channels)
        for bg in ("white", "black"):
            want_rgb, want_mask = ref.colors_chain(px, mip, bg == "black")
            for pad in (0, 1):                                    # 8-byte aligned: one load per ray; 2 bytes in: uint16 loads
                t = offset_tensor(sums, pad, dev)
                o, d, rgb, mask = hip_ops.raygen(rec, W, H, images=t, bg_color=bg, mip=mip)
                assert torch.equal(o, o0) and torch.equal(d, d0)
                assert torch.equal(rgb.cpu(), want_rgb), (mip, channels, bg, pad)
                assert mask.dtype == torch.bool and torch.equal(mask.cpu()[:, 0], want_mask)
        if channels == 4:
            assert np.array_equal(want_mask.numpy(), ref.mask_exact(px[:, 3], mip))
            at = lambda s: bool(want_mask[np.nonzero(px[:, 3] == s)[0][0]])
            assert not at(D // 2) and at(D // 2 + 1)
        else:
            assert bool(want_mask.all())


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_raygen_on_sums_indexed_whole_view_and_out_of_range(dev, n):
    mip, V, H, W = 2, 3, 5, 7
    rng = np.random.default_rng(n)
    sums = rng.integers(0, 255 * 16 + 1, (V, H, W, 4)).astype(np.uint16)
    rec = records(V, dev, seed=1)
    t = torch.from_numpy(sums).to(dev)
    flat = sums.reshape(V * H * W, 4).astype(np.int64)
    # the whole-view form: the first n rays of the V H W
    m = min(n, V * H * W)
    o, d, rgb, mask = hip_ops.raygen(rec, W, H, images=t, mip=mip, num_rays=m)
    o0, d0, _, _ = hip_ops.raygen(rec, W, H, num_rays=m)
    want_rgb, want_mask = ref.colors_chain(flat[:m], mip, False)
    assert torch.equal(o, o0) and torch.equal(d, d0) and torch.equal(rgb.cpu(), want_rgb)
    assert torch.equal(mask.cpu()[:, 0], want_mask)
    # the indexed form with bad indices among good ones
    vi = rng.integers(0, V, n).astype(np.int32)
    pi = rng.integers(0, H * W, n).astype(np.int32)
    bad = np.zeros(n, bool)
    if n > 2:
        vi[n // 2], pi[n - 2], bad[n // 2], bad[n - 2] = V, H * W, True, True
        vi[1], bad[1] = -1, True
        pi[n // 3 + 2], bad[n // 3 + 2] = -1, True
    tv, tp = torch.from_numpy(vi).to(dev), torch.from_numpy(pi).to(dev)
    for bg in ("white", "black"):
        o, d, rgb, mask = hip_ops.raygen(rec, W, H, tv, tp, images=t, bg_color=bg, mip=mip)
        o0, d0, _, _ = hip_ops.raygen(rec, W, H, tv, tp)
        assert torch.equal(o.isnan(), o0.isnan()) and torch.equal(o.nan_to_num(7.0), o0.nan_to_num(7.0))
        assert torch.equal(d.nan_to_num(7.0), d0.nan_to_num(7.0))
        good = ~bad
        want_rgb, want_mask = ref.colors_chain(flat[vi[good].astype(np.int64) * H * W + pi[good]], mip, bg == "black")
        rgb, mask, o = rgb.cpu().numpy(), mask.cpu().numpy()[:, 0], o.cpu().numpy()
        assert np.array_equal(rgb[good], want_rgb.numpy()) and np.array_equal(mask[good], want_mask.numpy())
        assert np.isnan(rgb[bad]).all() and np.isnan(o[bad]).all() and not mask[bad].any()
        assert not np.isnan(o[good]).any()


def test_raygen_refuses_sums_without_a_mip_and_bytes_with_one(dev):
    rec = records(1, dev)
    u16 = torch.from_numpy(np.zeros((1, 4, 4, 4), np.uint16)).to(dev)
    u8 = torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="uint8"):
        hip_ops.raygen(rec, 4, 4, images=u16)
    with pytest.raises(RuntimeError, match="uint8"):
        hip_ops.raygen(rec, 4, 4, images=u16, mip=0)
    with pytest.raises(RuntimeError, match="uint16"):
        hip_ops.raygen(rec, 4, 4, images=u8, mip=1)
    with pytest.raises(RuntimeError, match="mip"):
        hip_ops.raygen(rec, 4, 4, images=u16, mip=5)
    L = _lib.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    out = torch.zeros((16, 3), device=dev)
    m = torch.zeros(16, dtype=torch.uint8, device=dev)
    for mip in (0, 5):
        assert L.shacira_raygen_sums(p(rec), 1, 4, 4, None, None, None, 16, p(u16), 4, mip, 0, p(out), p(out), p(out), p(m),
                                     None) == _lib.EINVAL
    assert L.shacira_raygen_sums(p(rec), 1, 4, 4, None, None, None, 16, p(u16), 2, 1, 0, p(out), p(out), p(out), p(m),
                                 None) == _lib.EINVAL


# ---- NeRFSyntheticDataset(mip=...) --------------------------------------------------------------------------------------------
DS_V, DS_H, DS_W = 3, 8, 12
ALPHAS = np.array([0, 127, 128, 255], np.uint8)


def dataset_pixels():
    """3 RGBA views of 8 x 12 random bytes with alpha drawn from {0, 127, 128, 255}. A 4 x 4 block's alphas are drawn again
    until neither it nor any of its four 2 x 2 blocks has a mean of exactly 0.5 (a sum of 2 * 255 per four pixels), so that no
    pixel of the mip levels 1 and 2 sits on the mask's threshold: the test excuses ties and asserts there are none."""
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (DS_V, DS_H, DS_W, 4), dtype=np.uint8)
    for v in range(DS_V):
        for y in range(0, DS_H, 4):
            for x in range(0, DS_W, 4):
                while True:
                    a = ALPHAS[rng.integers(0, 4, (4, 4))].astype(np.int64)
                    quads = a.reshape(2, 2, 2, 2).sum(axis=(1, 3))
                    if (quads != 2 * 255).all() and a.sum() != 8 * 255:
                        break
                img[v, y:y + 4, x:x + 4, 3] = a
    return img


def write_views(root, img, meta):
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    rng = np.random.default_rng(4)
    frames = []
    for v in range(img.shape[0]):
        Image.fromarray(img[v], "RGBA").save(os.path.join(root, "train", f"r_{v}.png"))
        pose = np.eye(4)
        pose[:3, :3], _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pose[:3, 3] = rng.normal(size=3)
        frames.append(dict(file_path=f"./train/r_{v}", transform_matrix=pose.tolist()))
    with open(os.path.join(root, "transforms_train.json"), "w") as fh:
        json.dump(dict(frames=frames, **meta), fh)


@pytest.fixture(scope="module")
def views(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("mipviews"))
    img = dataset_pixels()
    write_views(root, img, dict(camera_angle_x=0.7, cx=7.5, cy=3.0))
    return root, img


@pytest.mark.parametrize("mip", [1, 2])
@pytest.mark.parametrize("bg", ["white", "black"])
def test_dataset_at_a_mip_level(dev, views, mip, bg):
    root, img = views
    f = 1 << mip
    h, w = DS_H // f, DS_W // f
    ds = NeRFSyntheticDataset(root, bg_color=bg, device=dev, mip=mip)
    sums = ref.block_sums(img, mip)
    assert ds.mip == mip and ds.images.dtype == torch.uint16 and ds.images.is_cuda and tuple(ds.images.shape) == (DS_V, h, w, 4)
    assert np.array_equal(ds.images.cpu().numpy().astype(np.int64), sums)
    assert len(ds) == DS_V and ds.img_shape == torch.Size((h, w, 3))
    assert ds.cameras.width == w and ds.cameras.height == h
    assert ds.cameras.focal_x[0].item() == pytest.approx((0.5 * w) / np.tan(0.5 * 0.7), rel=1e-15)
    assert ds.cameras.x0[0].item() == 7.5 / f - (w // 2) and ds.cameras.y0[0].item() == 3.0 / f - (h // 2)
    assert ds.records[0, 14].item() == np.float32(7.5 / f - (w // 2))
    assert ds.resident_bytes() == DS_V * h * w * 4 * 2 + DS_V * 80
    assert ds.reference_resident_bytes() == DS_V * h * w * 37
    # every view, bit for bit against the host chain; rays equal to the rays of the level's cameras without images
    flat = sums.reshape(DS_V, h * w, 4)
    for i in range(DS_V):
        item = ds[i]
        want_rgb, want_mask = ref.colors_chain(flat[i], mip, bg == "black")
        assert torch.equal(item["rgb"].cpu(), want_rgb) and torch.equal(item["masks"].cpu()[:, 0], want_mask)
        o0, d0, _, _ = hip_ops.raygen(ds.records[i:i + 1], w, h)
        assert torch.equal(item["rays"].origins, o0) and torch.equal(item["rays"].dirs, d0)
    whole = torch.stack([ds[i]["rgb"] for i in range(DS_V)])
    s = ds.sample(100, generator=torch.Generator(device=dev).manual_seed(1))
    assert s["rgb"].shape == (100, 3) and s["masks"].shape == (100, 1) and s["rays"].origins.shape == (100, 3)
    assert s["view_idx"].shape == s["pixel_idx"].shape == (100,) and int(s["pixel_idx"].max()) < h * w
    assert torch.equal(s["rgb"], whole[s["view_idx"].long(), s["pixel_idx"].long()])
    one = ds.sample(10, view=2)
    assert bool((one["view_idx"] == 2).all()) and torch.equal(one["rgb"], whole[2][one["pixel_idx"].long()])
    picked = SampleRays(16)(ds[0])
    assert picked["rgb"].shape == (16, 3) and picked["rays"].dirs.is_cuda
    # against the reference's float chain: colours within the two chains' carried bounds, masks equal away from a tie
    got = whole.cpu().numpy().astype(np.float64).reshape(-1, 3)
    their_rgb, their_mask = ref.reference_chain(img, mip, bg == "black")
    b = ref.chain_bounds(img, mip, bg == "black")
    tol = b["ours"] + b["theirs"]
    err = np.abs(got - their_rgb.numpy().astype(np.float64))
    print(f"mip {mip} {bg}: |ours - reference chain| max {err.max():.3e}, bound max {tol.max():.3e}, "
          f"largest ratio {(err / tol).max():.3f}")
    assert tol.max() < 64 * ref.U                                  # a loose derivation cannot hide an error
    assert (err <= tol).all()
    assert (np.abs(got - np.clip(b["rgb"], 0.0, 1.0)) <= b["ours"]).all()
    our_mask = torch.stack([ds[i]["masks"] for i in range(DS_V)]).cpu().numpy().reshape(-1)
    tie = np.abs(b["alpha"] - 0.5) <= b["alpha_theirs"]
    assert not tie.any() and (b["alpha"] > 0.5).any() and (b["alpha"] < 0.5).any()
    assert np.array_equal(our_mask[~tie], their_mask.numpy()[~tie])
    assert np.array_equal(our_mask, b["alpha"] > 0.5)


def test_dataset_mip_arguments(dev, views, tmp_path):
    root, img = views
    with pytest.raises(ValueError, match="5"):
        NeRFSyntheticDataset(root, device=dev, mip=5)
    with pytest.raises(ValueError, match="8 x 12"):
        NeRFSyntheticDataset(root, device=dev, mip=3)              # 12 is not divisible by 8
    small = str(tmp_path / "small")
    write_views(small, img[:, :4, :6], dict(camera_angle_x=0.7))
    with pytest.raises(ValueError, match="4 x 6"):
        NeRFSyntheticDataset(small, device=dev, mip=2)
    assert NeRFSyntheticDataset(small, device=dev, mip=1).images.shape == (DS_V, 2, 3, 4)
    a, b = NeRFSyntheticDataset(root, device=dev, mip=None), NeRFSyntheticDataset(root, device=dev, mip=0)
    assert a.mip == b.mip == 0 and a.images.dtype == torch.uint8 and torch.equal(a.images, b.images)
    assert torch.equal(a.images.cpu(), torch.from_numpy(img)) and torch.equal(a[1]["rgb"], b[1]["rgb"])
    assert a.cameras.x0[0].item() == 7.5 - DS_W // 2
    with pytest.raises(NotImplementedError):
        NeRFSyntheticDataset(root, mip=1)                          # a host dataset


def test_dataset_uploads_in_bounded_chunks(dev, views, monkeypatch):
    """With the bound below two views' bytes every view goes up alone; the sums are the same."""
    from shacira_amd.wisp.datasets import multiview_dataset
    root, img = views
    calls = []
    real = hip_ops.image_mip
    monkeypatch.setattr(multiview_dataset, "MIP_UPLOAD_BYTES", DS_H * DS_W * 4 + 1)
    monkeypatch.setattr(hip_ops, "image_mip", lambda images, mip, out=None: calls.append(images.shape[0]) or real(images, mip, out))
    ds = NeRFSyntheticDataset(root, device=dev, mip=1)
    assert calls == [1, 1, 1]
    assert np.array_equal(ds.images.cpu().numpy().astype(np.int64), ref.block_sums(img, 1))


# ---- the multiview harness at a mip level -------------------------------------------------------------------------------------
VIEWS, H, W = 6, 48, 32


@pytest.fixture(scope="module")
def analytic(dev, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("analytic_mip"))
    harness.write_analytic_dataset(root, VIEWS, H, W, seed=3, device=dev)
    ds = NeRFSyntheticDataset(root, split="train", bg_color="white", device=dev, mip=1)
    assert ds.img_shape == torch.Size((H // 2, W // 2, 3)) and ds.images.dtype == torch.uint16
    return ds


def test_evaluate_view_in_chunks_at_a_mip_level(analytic, dev):
    """tests/test_gpu_multiview.py's check on the mip level's 24 x 16 views: with the marcher's jitter fixed a ray's samples
    depend on the ray alone, and chunks of 50 rays give the unchunked image bit for bit."""
    ds = analytic
    h, w = H // 2, W // 2
    truth = harness._analytic_truth()
    blas = truth.grid.blas

    def fixed_raymarch(rays, level=None, num_samples=64, raymarch_type="ray"):
        lvl = blas._level(level)
        n = rays.origins.shape[0]
        ridx, samples, depth, deltas, boundary, offsets = render.raymarch_ray(
            rays.origins, rays.dirs, rays.dist_min, rays.dist_max, blas.occupancy_at(lvl, rays.origins.device), lvl,
            num_samples, jitter=torch.full((n, num_samples), 0.5, device=rays.origins.device))
        return ASRaymarchResults(ridx=ridx, samples=samples, depth_samples=depth, deltas=deltas, boundary=boundary,
                                 ray_offsets=offsets)

    truth.grid.raymarch = fixed_raymarch
    tracer = PackedRFTracer(raymarch_type="ray", num_steps=64, bg_color="white")
    whole = harness.evaluate_view(truth, tracer, ds, 2, chunk=h * w)
    parts = harness.evaluate_view(truth, tracer, ds, 2, chunk=50)
    assert whole["rgb"].shape == (h, w, 3) and torch.equal(whole["rgb"], parts["rgb"])
    assert whole["psnr"] == parts["psnr"] and whole["ssim"] == parts["ssim"]
    print(f"evaluate_view at mip 1: psnr {whole['psnr']:.2f} dB, ssim {whole['ssim']:.4f}")


def test_fit_multiview_reduces_the_loss_at_a_mip_level(analytic, dev):
    out = harness.fit_multiview(analytic, dev, steps=60, rays=512, num_steps=32, codebook_bitwidth=12, max_grid_res=64,
                                num_lods=8, prune_every=0, hidden_dim=32)
    losses = out["losses"]
    assert losses.shape == (60,) and torch.isfinite(losses).all()
    first, last = losses[:5].mean().item(), losses[-5:].mean().item()
    print(f"fit_multiview at mip 1: loss {first:.4f} -> {last:.4f}, {out['ms_per_step']:.2f} ms / step")
    assert last < first
