"""``MultiImageDataset``: a folder of images fitted one at a time (wisp/datasets/formats/multi_image_dataset.py), kept the way
this device wants it.

The reference loads the current image as fp32 colours and, in its pregenerated modes ('full', 'woreplace', 'sequential'), the
coordinate lattice and shuffled copies of both: 40 bytes per pixel on the host (12 colours, 8 coordinates, 20 shuffled), sliced
per batch and copied over. In its on-the-fly modes ('wreplace', 'eval') it keeps the fp32 colours (12 bytes) and gathers on the
host. Here the uint8 image lives on the dataset's device -- 3 bytes per pixel -- next to ``shuffle_idx`` in the shuffled modes,
and every batch's coordinates and colours are made from pixel indices by one kernel (``hip_ops.pixel_batch``); the loss reads the
same bytes (``hip_ops.pixel_loss``), so no fp32 target exists at any time. On a CPU device the same arithmetic runs in torch ops,
bit for bit.

One deliberate difference. The reference turns sampled indices into coordinates in ``transform_coords`` (:232-242) by dividing
the int64 index by an fp32 tensor, i.e. after rounding the index to 24 bits. That equals exact integer arithmetic for every pixel
of every image of up to 2^24 pixels (checked on the CPU for all pixels of sizes up to 4096 x 4095 and 3000 x 5592, and in
tests/test_pixels_cpu.py for the small ones), and here the rule IS the exact one: ``y = p // W, x = p - y * W``. Above 2^24
pixels the reference's rule returns a coordinate that is not the sampled pixel's -- for 88 % of 2^20 uniformly drawn indices of
its own gigapixel configuration, 20000 x 23466 (the same check, comparing the reference's three lines against the integer rule
on the CPU) -- so that its (coords, rgb) pairs do not belong together. That is not reproduced."""
import os
from math import prod

import torch

from ..ops.image.io import load_rgb_u8

_SUPPORTED_FORMATS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp", ".JPG", ".JPEG")
_MODES = ("full", "woreplace", "sequential", "wreplace", "eval")

REFERENCE_BYTES_PER_PIXEL = {"shuffled": 40, "sequential": 20, "on_the_fly": 12}


def pixel_coords_torch(pixel_idx, height, width):
    """fp32 [n, 2] lattice coordinates (row first) of integer pixel indices [n], in torch ops: the arithmetic of
    ``shacira_pixel_batch``, one rounding per operator."""
    p = pixel_idx.reshape(-1).to(torch.int64)
    y = torch.div(p, width, rounding_mode="floor")
    x = p - y * width
    cy = (y.to(torch.float32) / float(height) - 0.5) * 2.0
    cx = (x.to(torch.float32) / float(width) - 0.5) * 2.0
    return torch.stack([cy, cx], dim=-1)


class MultiImageDataset(torch.utils.data.Dataset):
    """Images of a directory, one resident at a time; ``load_next()`` brings in the next one.

    Args (the reference's, plus ``device``):
        dataset_path (str): directory of images.
        dataset_num_workers (int): kept for compatibility; loading is single-process.
        split (str): 'train' or 'val'; kept, not used internally.
        transform (Callable): kept, not applied (the reference does not apply it to coordinate batches either).
        num_samples (int): pixels per batch; -1 for the whole image.
        sample_mode (str): 'full' (the whole image, shuffled), 'woreplace' (shuffled, ``num_samples`` at a time), 'sequential'
            (image order, ``num_samples`` at a time), 'wreplace' (``num_samples`` uniform draws per batch), 'eval' (image order,
            batches carry indices).
        device: where the image and the batches live (default: the host).

    ``__getitem__`` has the reference's fields; ``batch`` / ``sample`` are the native form: always coordinates, colours and the
    pixel indices that ``hip_ops.pixel_loss`` takes."""

    def __init__(self, dataset_path, dataset_num_workers=-1, split="train", transform=None, num_samples=-1, sample_mode="full",
                 device=None):
        if sample_mode not in _MODES:
            raise ValueError(f"sample_mode must be one of {_MODES}, got {sample_mode!r}")
        self.dataset_path, self.dataset_num_workers, self.split, self.transform = dataset_path, dataset_num_workers, split, transform
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.image_list = []
        for imagename in sorted(os.listdir(self.dataset_path)):
            if any(imagename.endswith(ext) for ext in _SUPPORTED_FORMATS):
                self.image_list.append(os.path.join(self.dataset_path, imagename))
        self.num_images = len(self.image_list)
        self.sample_mode = sample_mode
        if self.sample_mode == "full":
            num_samples = -1
        self.num_samples = num_samples
        self.image_idx = 0
        self.image = None
        self._shuffle_idx = None
        self._cache = None

    @classmethod
    def is_root_of_dataset(cls, root, files_list):
        """True if ``files_list`` names at least one image of a supported format."""
        return any(any(filename.endswith(ext) for ext in _SUPPORTED_FORMATS) for filename in files_list)

    def create_split(self, split):
        """A dataset over the same directory and batch size for another split, in 'eval' mode."""
        return MultiImageDataset(dataset_path=self.dataset_path, dataset_num_workers=self.dataset_num_workers, split=split,
                                 transform=self.transform, num_samples=self.num_samples, sample_mode="eval", device=self.device)

    # ---- the resident image ----------------------------------------------------------------------------------------------
    def load_next(self):
        """Load the next image of the directory (IndexError past the last) and, in the shuffled modes, draw ``shuffle_idx``."""
        self.image_path = self.image_list[self.image_idx]
        self.set_image(load_rgb_u8(self.image_path))
        self.image_idx += 1

    def set_image(self, image):
        """Make ``image`` (uint8 [H, W, 3]) the resident image: what ``load_next`` does with the decoded file."""
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"MultiImageDataset expects a uint8 [H, W, 3] image, got {image.dtype} {tuple(image.shape)}")
        self._cache = None
        self._shuffle_idx = None
        self.image = image.to(self.device).contiguous()
        self.image_size = (int(image.shape[0]), int(image.shape[1]))
        # the trainer need not iterate a loader when every batch is the same pixels (the reference's rule, with its >=)
        self.static_coords = (self.num_samples == -1) or (self.num_samples >= prod(self.image_size))
        if self._shuffled():
            self.resample(force=True)

    def _whole(self):          # one batch of all pixels (the reference's rule, with its >)
        return self.num_samples == -1 or self.num_samples > prod(self.image_size)

    def _pregenerated(self):   # the modes in which the reference builds its coordinate grid
        return self.sample_mode not in ("eval", "wreplace") or self._whole()

    def _shuffled(self):
        return self._pregenerated() and self.sample_mode != "sequential"

    def _index_dtype(self):
        return torch.int32 if prod(self.image_size) <= 2 ** 31 - 1 else torch.int64

    @property
    def shuffle_idx(self):
        """The permutation of the pixels in the shuffled modes (int32 below 2^31 pixels, else int64), None otherwise."""
        return self._shuffle_idx

    @shuffle_idx.setter
    def shuffle_idx(self, value):
        value = torch.as_tensor(value)
        if value.dim() != 1 or value.shape[0] != prod(self.image_size) or value.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"shuffle_idx must be an integer permutation of {prod(self.image_size)} pixels")
        self._shuffle_idx = value.to(device=self.device, dtype=self._index_dtype()).contiguous()
        self._cache = None

    def resample(self, force=False):
        """Draw a new ``shuffle_idx`` in 'woreplace' mode; nothing in the other modes."""
        if self.sample_mode == "woreplace" or force:
            self._shuffle_idx = torch.randperm(prod(self.image_size), dtype=self._index_dtype(), device=self.device)
            self._cache = None

    def __len__(self):
        """Batches of the CURRENT image (not the number of images)."""
        if self._whole():
            return 1
        hw = prod(self.image_size)
        return hw // self.num_samples + (1 if hw % self.num_samples > 0 else 0)

    # ---- batches ---------------------------------------------------------------------------------------------------------
    def pixels_of(self, pixel_idx=None, start=0, n=None, want_coords=True, want_rgb=True):
        """(coords, rgb) of pixels by index or by range: the fused kernel on the device, the same arithmetic in torch ops on
        the host."""
        H, W = self.image_size
        if self.device.type == "cuda":
            from ... import hip_ops
            return hip_ops.pixel_batch(self.image, pixel_idx, start, n, want_coords, want_rgb)
        if pixel_idx is None:
            pixel_idx = torch.arange(start, H * W if n is None else start + n, dtype=torch.int64)
        p = pixel_idx.reshape(-1).to(torch.int64)
        coords = pixel_coords_torch(p, H, W) if want_coords else None
        rgb = self.image.reshape(-1, 3)[p].to(torch.float32) / 255.0 if want_rgb else None
        return coords, rgb

    def _range_of(self, i):
        hw = prod(self.image_size)
        if self._whole():
            if i != 0:
                raise IndexError(i)
            return 0, hw
        if not 0 <= i < len(self):
            raise IndexError(i)
        start = i * self.num_samples
        return start, min(start + self.num_samples, hw)

    def batch(self, i):
        """Batch ``i`` of the current image in every mode: dict(coords fp32 [n, 2], rgb fp32 [n, 3], pixel_idx, start).
        ``pixel_idx`` is the int32 / int64 [n] tensor of the batch's pixels, or None where the batch is the run of pixels
        ``start .. start + n`` of the image ('sequential' and 'eval'); both forms are what ``hip_ops.pixel_loss`` takes. In
        'wreplace' mode the batch is ``sample(num_samples)``. The one batch of a 'full' dataset is made once and kept."""
        if self.image is None:
            raise RuntimeError("MultiImageDataset: no image is loaded; call load_next() first")
        if self.sample_mode == "wreplace" and not self._whole():
            if not 0 <= i < len(self):
                raise IndexError(i)
            return self.sample(self.num_samples)
        start, end = self._range_of(i)
        if self._cache is not None and self._cache[0] == (start, end):
            return dict(self._cache[1])
        if self._shuffled():
            pixel_idx = self._shuffle_idx[start:end]
            coords, rgb = self.pixels_of(pixel_idx)
            out = dict(coords=coords, rgb=rgb, pixel_idx=pixel_idx, start=0)
        else:
            coords, rgb = self.pixels_of(None, start, end - start)
            out = dict(coords=coords, rgb=rgb, pixel_idx=None, start=start)
        if self.sample_mode == "full":
            self._cache = ((start, end), out)
            return dict(out)
        return out

    def sample(self, n, generator=None):
        """``n`` uniform draws with replacement from the current image: ``batch``'s dict. Indices and outputs are tensors on the
        dataset's device and nothing is read back."""
        if self.image is None:
            raise RuntimeError("MultiImageDataset: no image is loaded; call load_next() first")
        pixel_idx = torch.randint(0, prod(self.image_size), (n,), device=self.device, dtype=self._index_dtype(),
                                  generator=generator)
        coords, rgb = self.pixels_of(pixel_idx)
        return dict(coords=coords, rgb=rgb, pixel_idx=pixel_idx, start=0)

    def __getitem__(self, idx):
        """The reference's batch: dict(coords, rgb). In 'full', 'woreplace' and 'sequential' mode (and whenever one batch is the
        whole image) ``coords`` is fp32 [n, 2]; in 'eval' and 'wreplace' mode it is the int64 [n, 1] pixel indices, which
        ``transform_coords`` turns into coordinates."""
        if self._pregenerated():
            b = self.batch(0 if self._whole() else idx)
            return dict(coords=b["coords"], rgb=b["rgb"])
        if self.sample_mode == "eval":
            start, end = self._range_of(idx)
            index = torch.arange(start, end, dtype=torch.int64, device=self.device).reshape(-1, 1)
            _, rgb = self.pixels_of(None, start, end - start, want_coords=False)
        else:
            index = torch.randint(0, prod(self.image_size), (self.num_samples, 1), device=self.device)
            _, rgb = self.pixels_of(index, want_coords=False)
        return dict(coords=index, rgb=rgb)

    def transform_coords(self, coord_idx, device=None):
        """Batches of the pregenerated modes pass through; the [n, 1] indices of 'eval' and 'wreplace' batches become fp32
        [n, 2] coordinates in [-1, 1) by the exact integer rule (see the module's docstring)."""
        if self._pregenerated():
            return coord_idx
        coords = self.pixels_of(coord_idx.to(self.device), want_rgb=False)[0]      # made where the image lives
        return coords if device is None else coords.to(device)

    @property
    def coordinates(self):
        """The coordinates of the current image's pixels in batch order in the pregenerated modes (made now, not kept), None in
        the on-the-fly modes."""
        if self.image is None or not self._pregenerated():
            return None
        return self.pixels_of(self._shuffle_idx if self._shuffled() else None, want_rgb=False)[0]

    @property
    def pixels(self):
        """The colours that go with ``coordinates``."""
        if self.image is None or not self._pregenerated():
            return None
        return self.pixels_of(self._shuffle_idx if self._shuffled() else None, want_coords=False)[1]

    # ---- what is resident -------------------------------------------------------------------------------------------------
    def resident_bytes(self):
        """Bytes kept for the current image: its uint8 pixels, ``shuffle_idx`` in the shuffled modes, and the one kept batch of
        a 'full' dataset once it has been made."""
        size = lambda t: t.numel() * t.element_size()
        total = size(self.image) if self.image is not None else 0
        if self._shuffle_idx is not None:
            total += size(self._shuffle_idx)
        if self._cache is not None:
            total += size(self._cache[1]["coords"]) + size(self._cache[1]["rgb"])
        return total

    def reference_resident_bytes(self):
        """What the reference's layout keeps for the same image (its int64 ``shuffle_idx`` not counted): fp32 colours and
        coordinates and shuffled copies of both in the shuffled modes, no copies in 'sequential', colours alone on the fly."""
        kind = "shuffled" if self._shuffled() else "sequential" if self._pregenerated() else "on_the_fly"
        return prod(self.image_size) * REFERENCE_BYTES_PER_PIXEL[kind]
