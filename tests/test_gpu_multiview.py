"""The multiview path end to end on the MI355X: harness.write_analytic_dataset renders a small NeRF-synthetic style dataset
through this package's rays, wisp.datasets.NeRFSyntheticDataset reads it back onto the device, harness.evaluate_view renders a
view in chunks and harness.fit_multiview trains on dataset.sample. Wiring checks, not quality bars."""
import numpy as np
import pytest
import torch
from PIL import Image

import raygen_ref
from shacira_amd import harness, render
from shacira_amd.wisp.accelstructs import ASRaymarchResults
from shacira_amd.wisp.datasets import NeRFSyntheticDataset, SampleRays
from shacira_amd.wisp.tracers import PackedRFTracer

pytestmark = pytest.mark.gpu
VIEWS, H, W = 6, 16, 24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dataset(dev, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("analytic"))
    files = harness.write_analytic_dataset(root, VIEWS, H, W, seed=3, device=dev)
    return NeRFSyntheticDataset(root, split="train", bg_color="white", device=dev), files


def test_dataset_views_equal_the_png_composite(dataset, dev):
    ds, files = dataset
    assert len(ds) == len(files) == VIEWS and ds.img_shape == torch.Size((H, W, 3))
    assert ds.images.shape == (VIEWS, H, W, 4) and ds.images.is_cuda and ds.records.is_cuda
    assert ds.resident_bytes() == VIEWS * H * W * 4 + VIEWS * 80 and ds.reference_resident_bytes() == VIEWS * H * W * 37
    seen_object = False
    for i, path in enumerate(files):
        png = np.array(Image.open(path))
        assert png.shape == (H, W, 4)
        rgb, mask = raygen_ref.colors_ref(png.reshape(-1, 4), False)
        item = ds[i]
        assert torch.equal(item["rgb"].cpu(), rgb) and torch.equal(item["masks"].cpu()[:, 0], mask)
        assert item["rays"].origins.shape == (H * W, 3) and item["rays"].dist_max == 6.0
        assert torch.allclose(item["rays"].origins.norm(dim=1), torch.full((H * W,), 3.0, device=dev), atol=1e-5)
        seen_object |= bool(mask.any()) and not bool(mask.all())
    assert seen_object                                   # the cameras look at the scene: object and background in view
    s = ds.sample(300, generator=torch.Generator(device=dev).manual_seed(1))
    whole = torch.stack([ds[i]["rgb"] for i in range(VIEWS)])
    assert s["view_idx"].is_cuda and torch.equal(s["rgb"], whole[s["view_idx"].long(), s["pixel_idx"].long()])
    picked = SampleRays(32)(ds[0])
    assert picked["rgb"].shape == (32, 3) and picked["rays"].dirs.is_cuda


def test_evaluate_view_in_chunks_equals_the_unchunked_render(dataset, dev):
    """The 'ray' marcher draws its stratified jitter from the global generator, one row per ray of the BATCH, so two chunkings
    see different jitter. Here the truth field's grid marches with the jitter fixed at the middle of every stratum (the marcher's
    own ``jitter=`` operand): then every ray's samples are a function of the ray alone, and 7 chunks of 50 rays + one of 34
    must give the unchunked image bit for bit."""
    ds, _ = dataset
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
    whole = harness.evaluate_view(truth, tracer, ds, 2, chunk=H * W)
    parts = harness.evaluate_view(truth, tracer, ds, 2, chunk=50)
    assert whole["rgb"].shape == (H, W, 3) and torch.equal(whole["rgb"], parts["rgb"])
    assert whole["psnr"] == parts["psnr"] and whole["ssim"] == parts["ssim"]
    # the dataset was rendered from this scene (256 jittered steps, 8-bit): the 64-step render is close to its target
    print(f"evaluate_view: psnr {whole['psnr']:.2f} dB, ssim {whole['ssim']:.4f}")
    assert whole["psnr"] > 20.0


def test_fit_multiview_reduces_the_loss(dataset, dev):
    ds, _ = dataset
    out = harness.fit_multiview(ds, dev, steps=60, rays=512, num_steps=32, codebook_bitwidth=12, max_grid_res=64, num_lods=8,
                                prune_every=0, hidden_dim=32)
    losses = out["losses"]
    assert losses.shape == (60,) and torch.isfinite(losses).all()
    first, last = losses[:5].mean().item(), losses[-5:].mean().item()
    print(f"fit_multiview: loss {first:.4f} -> {last:.4f}, {out['ms_per_step']:.2f} ms / step")
    assert last < first
