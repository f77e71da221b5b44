#!/usr/bin/env python3
"""Generate tests/golden/image_dataset.npz by RUNNING the reference's MultiImageDataset on the CPU (dev container only).

Run:  python tests/golden/make_image_dataset_golden.py        (needs /root/reference)

The reference's wisp/datasets/formats/multi_image_dataset.py is executed from its file, and so is its
wisp/ops/raygen/raygen.py for ``generate_2d_grid`` (by the loader of make_raygen_golden.py). What it imports besides is
shimmed: ``BaseImageDataset`` by a stand-in that keeps the four constructor arguments and routes ``load()`` to
``load_singleprocess()``, ``ImageBatch`` by a dict, ``wisp.ops.mesh`` by an empty module, and ``wisp.ops.image`` -- whose io.py
imports torchvision, which is not installed -- by a stand-in for ``load_rgb_tensor``: PIL's RGB bytes, permuted to CHW, as fp32,
divided by 255, which is what torchvision's ``ToTensor`` does to an 8-bit image. So the sampling, slicing, shuffling and
index-to-coordinate arithmetic recorded here is the reference's own executed text; the decode-and-divide underneath is the
stand-in. Recorded per (case, image): the image's bytes, ``shuffle_idx``, (``len``, ``static_coords``, ``num_samples``) and all
batches' ``coords`` / ``rgb`` one after the other (with ``transform_coords`` of the coords where they are indices). The permutation is stored, not an RNG seed. Nothing of the
reference is copied: outputs are plain arrays."""
import importlib.util
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch
from PIL import Image

from make_raygen_golden import _reference_module as _reference_raygen

IMAGES = {"a": (7, 5), "b": (4, 6)}          # name: (H, W); the files sort in this order
CASES = {      # name: (sample_mode, num_samples)
    "full": ("full", 8),                     # the mode forces num_samples = -1
    "woreplace": ("woreplace", 8),
    "sequential": ("sequential", 8),
    "wreplace": ("wreplace", 8),
    "eval": ("eval", 8),
    "eval_whole": ("eval", -1),              # one batch of the whole image: the reference shuffles it
    "wreplace_over": ("wreplace", 100),      # more samples than pixels: the whole image again
    "sequential_exact_a": ("sequential", 35),  # exactly image a's pixels: one full batch, static by the >= rule
}


def make_image(name):
    H, W = IMAGES[name]
    g = torch.Generator().manual_seed(H * 100 + W)
    return torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8).numpy()


def _reference_class():
    raygen = _reference_raygen()             # installs shims for `wisp` and `wisp.core`

    class BaseImageDataset(torch.utils.data.Dataset):
        def __init__(self, dataset_path=None, dataset_num_workers=-1, transform=None, split=None):
            self.dataset_path, self.dataset_num_workers = dataset_path, dataset_num_workers
            self.transform, self.split = transform, split

        def load(self):
            return self.load_singleprocess()

    def load_rgb_tensor(path, normalize=True):          # the stand-in for torchvision's ToTensor
        data = torch.from_numpy(np.array(Image.open(path).convert("RGB"), dtype=np.uint8))
        return data.permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def module(name, **members):
        mod = types.ModuleType(name)
        mod.__dict__.update(members)
        sys.modules[name] = mod
        return mod

    module("wisp.datasets").__path__ = []
    module("wisp.datasets.base_datasets", BaseImageDataset=BaseImageDataset)
    module("wisp.datasets.batch", ImageBatch=dict)
    module("wisp.ops").__path__ = []
    module("wisp.ops.mesh")
    module("wisp.ops.image", load_rgb=None, load_rgb_tensor=load_rgb_tensor)
    module("wisp.ops.raygen", generate_2d_grid=raygen.generate_2d_grid)
    spec = importlib.util.spec_from_file_location("reference_multi_image_dataset",
                                                  f"{REF}/wisp/datasets/formats/multi_image_dataset.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MultiImageDataset


def main():
    cls = _reference_class()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in IMAGES:
            out[f"image.{name}"] = make_image(name)
            Image.fromarray(out[f"image.{name}"]).save(os.path.join(tmp, f"{name}.png"))
        with open(os.path.join(tmp, "notes.txt"), "w") as fh:      # not an image: must not be listed
            fh.write("x")
        torch.manual_seed(20240)
        for case, (mode, num_samples) in CASES.items():
            ds = cls(tmp, 0, "train", None, num_samples, mode)
            assert [os.path.basename(p) for p in ds.image_list] == ["a.png", "b.png"] and ds.num_images == 2
            for name in IMAGES:
                ds.load_next()
                key = f"{case}.{name}"
                assert tuple(ds.image_size) == IMAGES[name]
                out[f"{key}.meta"] = np.array([len(ds), int(ds.static_coords), ds.num_samples], np.int64)
                if "coords" in ds.data and mode != "sequential":
                    out[f"{key}.shuffle_idx"] = ds.shuffle_idx.numpy().astype(np.int64)
                batches = [ds[i] for i in range(len(ds))]
                sizes = [b["coords"].shape[0] for b in batches]
                # the batches one after the other; all but the last have sizes[0] rows
                assert all(s == sizes[0] for s in sizes[:-1]) and sizes[-1] <= sizes[0]
                out[f"{key}.coords"] = torch.cat([b["coords"] for b in batches]).numpy()
                out[f"{key}.rgb"] = torch.cat([b["rgb"] for b in batches]).numpy()
                tcoords = torch.cat([ds.transform_coords(b["coords"], "cpu") for b in batches]).numpy()
                assert out[f"{key}.rgb"].dtype == np.float32 and tcoords.dtype == np.float32
                if out[f"{key}.coords"].dtype == np.int64:          # the on-the-fly modes: indices, and their coordinates
                    out[f"{key}.tcoords"] = tcoords
                else:                                              # the pregenerated modes pass their coordinates through
                    assert np.array_equal(tcoords, out[f"{key}.coords"])
            assert ds.image_idx == 2
            split = ds.create_split("val")
            assert split.sample_mode == "eval" and split.num_samples == ds.num_samples and split.split == "val"
    path = os.path.join(HERE, "image_dataset.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
