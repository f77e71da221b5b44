"""MultiImageDataset on the host (no GPU) against tests/golden/image_dataset.npz: what the reference's own MultiImageDataset
returned for two small PNGs in each of its five modes (tests/golden/make_image_dataset_golden.py). Bit for bit, with the
reference's ``shuffle_idx`` put in place of ours -- no RNG stream is relied on."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from shacira_amd.wisp.datasets import MultiImageDataset
from shacira_amd.wisp.ops.image import io

from image_dataset_cases import CASES, IMAGES, check_against_golden, write_images


@pytest.mark.parametrize("case", sorted(CASES))
def test_cpu_dataset_equals_the_references_batches(golden, tmp_path, case):
    gold = golden("image_dataset.npz")
    mode, num_samples = CASES[case]
    ds = MultiImageDataset(write_images(gold, tmp_path), 0, "train", None, num_samples, mode)
    assert [os.path.basename(p) for p in ds.image_list] == ["a.png", "b.png"] and ds.num_images == 2 and ds.image_idx == 0
    with pytest.raises(RuntimeError, match="load_next"):
        ds.batch(0)
    for k, name in enumerate(IMAGES):                        # load_next walks the directory
        ds.load_next()
        assert ds.image_idx == k + 1 and ds.image_path.endswith(f"{name}.png")
        assert torch.equal(ds.image, torch.from_numpy(gold[f"image.{name}"]))
        check_against_golden(gold, ds, case, name)
    with pytest.raises(IndexError):
        ds.load_next()
    split = ds.create_split("val")
    assert (split.sample_mode, split.num_samples, split.split, split.dataset_path) == ("eval", ds.num_samples, "val",
                                                                                       ds.dataset_path)
    assert isinstance(split, MultiImageDataset) and split.image_idx == 0


def test_short_last_batch_resample_and_resident_bytes(golden, tmp_path):
    gold = golden("image_dataset.npz")
    path = write_images(gold, tmp_path)
    ds = MultiImageDataset(path, 0, "train", num_samples=8, sample_mode="woreplace")
    ds.load_next()                                           # 7 x 5 = 35 pixels: four batches of 8 and one of 3
    assert len(ds) == 5 and [ds[i]["rgb"].shape[0] for i in range(5)] == [8, 8, 8, 8, 3]
    assert ds.shuffle_idx.dtype == torch.int32
    assert ds.resident_bytes() == 35 * 3 + 35 * 4 and ds.reference_resident_bytes() == 35 * 40
    before = ds.shuffle_idx.clone()
    torch.manual_seed(5)
    ds.resample()
    assert sorted(ds.shuffle_idx.tolist()) == list(range(35)) and not torch.equal(before, ds.shuffle_idx)
    for mode, per_pixel, own in (("sequential", 20, 3), ("eval", 12, 3), ("wreplace", 12, 3), ("full", 40, 3 + 4)):
        other = MultiImageDataset(path, 0, "train", num_samples=8, sample_mode=mode)
        other.load_next()
        kept = other.shuffle_idx
        other.resample()                                     # only 'woreplace' draws again
        assert other.shuffle_idx is kept
        assert other.reference_resident_bytes() == 35 * per_pixel and other.resident_bytes() == 35 * own, mode
    first = other.batch(0)                                   # 'full': the one batch is made once and kept
    assert other.batch(0)["coords"] is first["coords"] and other.resident_bytes() == 35 * (3 + 4 + 20)
    g = torch.Generator().manual_seed(11)
    s1 = ds.sample(64, generator=g)
    s2 = ds.sample(64, generator=torch.Generator().manual_seed(11))
    assert torch.equal(s1["pixel_idx"], s2["pixel_idx"]) and torch.equal(s1["rgb"], s2["rgb"])
    assert tuple(s1["coords"].shape) == (64, 2) and int(s1["pixel_idx"].max()) < 35
    with pytest.raises(ValueError):
        MultiImageDataset(path, 0, "train", sample_mode="random")
    assert MultiImageDataset.is_root_of_dataset(path, ["x.txt", "a.JPG"]) and not MultiImageDataset.is_root_of_dataset(path, ["a.txt"])


def test_image_io_round_trip(tmp_path):
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (6, 9, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    path = str(tmp_path / "x.png")
    io.write_png(path, img)
    assert torch.equal(io.load_rgb_u8(path), img)
    chw = io.load_rgb_tensor(path)
    assert chw.dtype == torch.float32 and tuple(chw.shape) == (3, 6, 9)
    assert torch.equal(io.chw_to_hwc(chw), img.float() / 255) and torch.equal(io.hwc_to_chw(io.chw_to_hwc(chw)), chw)
    arr = io.load_rgb(path)
    assert arr.dtype == np.float32 and arr.shape == (6, 9, 3) and np.array_equal(arr, (img.float() / 255).numpy())
    assert np.array_equal(io.load_rgb(path, normalize=False), img.numpy())
    assert io.glob_imgs(str(tmp_path)) == [path]
    Image.fromarray(img.numpy()[..., 0]).save(str(tmp_path / "grey.png"))      # any mode comes back as RGB bytes
    assert tuple(io.load_rgb_u8(str(tmp_path / "grey.png")).shape) == (6, 9, 3)


def test_wisp_aliases_reach_the_dataset_and_io():
    import sys
    from shacira_amd import wisp as mirror
    saved = {k: v for k, v in sys.modules.items() if k == "wisp" or k.startswith("wisp.")}
    try:
        mirror.install_as_wisp(force=True)
        from wisp.datasets import MultiImageDataset as D1
        from wisp.datasets.image_dataset import MultiImageDataset as D2
        from wisp.ops.image.io import load_rgb_tensor
        from wisp.ops.image import load_rgb
        assert D1 is MultiImageDataset and D2 is MultiImageDataset and load_rgb_tensor is io.load_rgb_tensor and load_rgb is io.load_rgb
    finally:
        for k in [k for k in sys.modules if k == "wisp" or k.startswith("wisp.")]:
            del sys.modules[k]
        sys.modules.update(saved)
