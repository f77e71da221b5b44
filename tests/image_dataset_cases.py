"""What tests/test_image_dataset_cpu.py and tests/test_gpu_image_dataset.py share: the cases of tests/golden/image_dataset.npz
(tests/golden/make_image_dataset_golden.py), the two PNGs written from the golden's bytes, and the comparison of one loaded image
of a MultiImageDataset -- on either device -- with what the reference returned for it, bit for bit."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

CASES = {"full": ("full", 8), "woreplace": ("woreplace", 8), "sequential": ("sequential", 8), "wreplace": ("wreplace", 8),
         "eval": ("eval", 8), "eval_whole": ("eval", -1), "wreplace_over": ("wreplace", 100),
         "sequential_exact_a": ("sequential", 35)}
IMAGES = ("a", "b")


def write_images(gold, path):
    for name in IMAGES:
        Image.fromarray(gold[f"image.{name}"]).save(os.path.join(path, f"{name}.png"))
    with open(os.path.join(path, "notes.txt"), "w") as fh:
        fh.write("x")
    return str(path)


def check_against_golden(gold, ds, case, name):
    """The loaded image ``name`` of ``ds`` against the golden's record of ``case``: every batch, both forms."""
    mode, _ = CASES[case]
    key = f"{case}.{name}"
    length, static, num_samples = (int(v) for v in gold[f"{key}.meta"])
    H, W = gold[f"image.{name}"].shape[:2]
    assert ds.image_size == (H, W) and len(ds) == length and ds.static_coords == bool(static) and ds.num_samples == num_samples
    if f"{key}.shuffle_idx" in gold:
        assert ds.shuffle_idx is not None and sorted(ds.shuffle_idx.tolist()) == list(range(H * W))
        ds.shuffle_idx = torch.from_numpy(gold[f"{key}.shuffle_idx"])
    else:
        assert ds.shuffle_idx is None
    coords, rgb = gold[f"{key}.coords"], gold[f"{key}.rgb"]
    per = coords.shape[0] if length == 1 else num_samples
    for i in range(length):
        want_c, want_rgb = coords[i * per:(i + 1) * per], rgb[i * per:(i + 1) * per]
        item = ds[i]
        assert set(item) == {"coords", "rgb"} and item["coords"].device.type == ds.device.type
        assert item["rgb"].dtype == torch.float32 and tuple(item["rgb"].shape) == want_rgb.shape
        native = ds.batch(i)
        assert native["coords"].dtype == torch.float32 and tuple(native["coords"].shape) == (want_c.shape[0], 2)
        if coords.dtype == np.int64:                         # 'eval' / 'wreplace': indices [n, 1] and their coordinates
            want_t = gold[f"{key}.tcoords"][i * per:(i + 1) * per]
            assert item["coords"].dtype == torch.int64 and tuple(item["coords"].shape) == want_c.shape
            idx = torch.from_numpy(want_c).to(ds.device)
            if mode == "eval":
                assert np.array_equal(item["coords"].cpu().numpy(), want_c)
                assert np.array_equal(item["rgb"].cpu().numpy(), want_rgb)
                assert np.array_equal(native["coords"].cpu().numpy(), want_t)
                assert np.array_equal(native["rgb"].cpu().numpy(), want_rgb)
                assert native["pixel_idx"] is None and native["start"] == i * per
            else:                                            # our draws are our own: hold the gather to the reference's draws
                assert int(item["coords"].min()) >= 0 and int(item["coords"].max()) < H * W
                got_c, got_rgb = ds.pixels_of(idx)
                assert np.array_equal(got_rgb.cpu().numpy(), want_rgb) and np.array_equal(got_c.cpu().numpy(), want_t)
                own_c, own_rgb = ds.pixels_of(native["pixel_idx"])
                assert torch.equal(own_c, native["coords"]) and torch.equal(own_rgb, native["rgb"])
            got_t = ds.transform_coords(idx, ds.device)
            assert got_t.dtype == torch.float32 and np.array_equal(got_t.cpu().numpy(), want_t)
        else:
            assert np.array_equal(item["coords"].cpu().numpy(), want_c) and np.array_equal(item["rgb"].cpu().numpy(), want_rgb)
            assert np.array_equal(native["coords"].cpu().numpy(), want_c) and np.array_equal(native["rgb"].cpu().numpy(), want_rgb)
            assert ds.transform_coords(item["coords"], ds.device) is item["coords"]
            if native["pixel_idx"] is not None:
                assert np.array_equal(native["pixel_idx"].cpu().numpy(), gold[f"{key}.shuffle_idx"][i * per:(i + 1) * per])
            else:
                assert mode == "sequential" and native["start"] == i * per
    with pytest.raises(IndexError):
        ds.batch(length)
    if coords.dtype != np.int64:
        assert np.array_equal(ds.coordinates.cpu().numpy(), coords) and np.array_equal(ds.pixels.cpu().numpy(), rgb)
    else:
        assert ds.coordinates is None and ds.pixels is None
