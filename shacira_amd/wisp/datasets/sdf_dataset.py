"""Signed-distance datasets of the reference (``wisp/datasets/formats/mesh_sdf_dataset.py`` and ``octree_sdf_dataset.py``):
points sampled on, near and around one mesh with their distances to it, resampled during training.

The reference samples with a chain of host-side torch calls on the global generator, copies to the GPU for the distance and
back ("can take up to a minute"). Here the working set never leaves the device: the points come from the fused sampler of
mesh_sample.hip (``hip_ops.mesh_sample``), each a pure function of (seed, sample index, technique), the distances from
mesh_sdf.hip. A dataset built twice with the same ``seed`` holds the same bytes, resample after resample."""
import os

import torch

from .batch import SDFBatch

_SUPPORTED_FORMATS = ["obj"]
_DEFAULT_MODES = ("rand", "rand", "near", "near", "trace")


def _mesh_ops():
    from ..ops import mesh
    return mesh


class SDFDataset(torch.utils.data.Dataset):
    """What the signed-distance datasets share: a working set ``data`` of ``coords`` [N, 3], ``sdf`` [N, 1] and optional
    ``rgb`` / ``normals``, read in batches as ``SDFBatch`` and replaced by ``resample()``."""

    def __init__(self, dataset_path=None, split="train", transform=None):
        self.dataset_path, self.split, self.transform = dataset_path, split, transform
        self.data = None

    @property
    def coordinates(self) -> torch.Tensor:
        """The coordinates of the current working set, [N, 3]."""
        return self.data["coords"]

    def resample(self) -> None:
        """Replace the working set by a new one (in place)."""

    def __len__(self):
        return self.data["coords"].shape[0]

    def __getitem__(self, idx) -> SDFBatch:
        out = SDFBatch(coords=self.data["coords"][idx], sdf=self.data["sdf"][idx],
                       rgb=self.data["rgb"][idx] if "rgb" in self.data else None,
                       normals=self.data["normals"][idx] if "normals" in self.data else None)
        if self.transform is not None:
            out = self.transform(out)
        return out


def _resample_key(seed, count):
    """The 64-bit Philox key of working set ``count``: ``seed``'s low word, ``count`` as the high word."""
    return ((int(count) & 0xFFFFFFFF) << 32) | (int(seed) & 0xFFFFFFFF)


class MeshSampledSDFDataset(SDFDataset):
    """Samples over one mesh (.obj): ``num_samples`` points per entry of ``sample_mode`` ('trace' on the surface, 'near'
    within Gaussian noise of it, 'rand' uniform in the cube; default rand, rand, near, near, trace) and their signed
    distances. ``get_normals``: all samples lie on the surface and carry their face normals. ``sample_tex``: the colour of
    the nearest surface point comes along (``closest_tex``). ``mode_norm``: 'sphere', 'aabb', 'planar' or 'none'
    (``wisp.ops.mesh.normalize``). Beyond the reference: ``seed`` and ``device``; working set k is a function of (seed, k)."""

    def __init__(self, dataset_path, split, transform=None, sample_mode=None, num_samples=100000, get_normals=False,
                 sample_tex=False, mode_norm="sphere", seed=0, device="cuda"):
        super().__init__(dataset_path=dataset_path, split=split, transform=transform)
        self.sample_mode = list(sample_mode) if sample_mode is not None else list(_DEFAULT_MODES)
        self.num_samples, self.get_normals, self.sample_tex, self.mode_norm = num_samples, get_normals, sample_tex, mode_norm
        self.seed, self.device = int(seed), torch.device(device)
        self.verts = self.faces = self.texv = self.texf = self.mats = None
        self.resample_count = 0
        self.validate(dataset_path)
        self.load()

    def validate(self, dataset_path) -> None:
        if not os.path.exists(dataset_path):
            raise FileNotFoundError(f"MeshSampledSDFDataset requires a mesh path, the dataset_path does not exist: "
                                    f"{dataset_path}")
        if not any(dataset_path.endswith(ext) for ext in _SUPPORTED_FORMATS):
            raise FileNotFoundError(f"MeshSampledSDFDataset does not support the mesh format of {dataset_path}. "
                                    f"Please use any of the supported formats: {_SUPPORTED_FORMATS}")

    @classmethod
    def is_root_of_dataset(cls, root, files_list=None) -> bool:
        return any(root.endswith(ext) for ext in _SUPPORTED_FORMATS)

    def load(self) -> None:
        from ... import hip_ops
        mesh = _mesh_ops()
        if self.sample_tex:
            verts, faces, self.texv, self.texf, self.mats = mesh.load_obj_materials(self.dataset_path)
        else:
            verts, faces = mesh.load_obj(self.dataset_path)
        verts, faces = mesh.normalize(verts, faces, self.mode_norm)
        self.verts, self.faces = verts.to(self.device), faces.to(self.device)
        hip_ops._need_gpu(self.verts)
        self.face_cdf = hip_ops.mesh_face_cdf(self.verts[self.faces])       # once per mesh
        self.resample()

    def resample(self) -> None:
        """A new working set: the samples of key (seed, number of resamples so far) and their distances. Everything stays on
        the device."""
        mesh = _mesh_ops()
        key = _resample_key(self.seed, self.resample_count)
        self.resample_count += 1
        rgb = nrm = None
        if self.get_normals:
            pts, nrm = mesh.sample_surface(self.verts, self.faces, self.num_samples * len(self.sample_mode),
                                           distrib=self.face_cdf, seed=key)
        else:
            pts = mesh.point_sample(self.verts, self.faces, self.sample_mode, self.num_samples, seed=key,
                                    distrib=self.face_cdf)
        if self.sample_tex:
            rgb, _, d = mesh.closest_tex(self.verts, self.faces, self.texv, self.texf, self.mats, pts)
        else:
            d = mesh.compute_sdf(self.verts, self.faces, pts)
        self.data = dict(coords=pts, sdf=d)
        if rgb is not None:
            self.data["rgb"] = rgb
        if nrm is not None:
            self.data["normals"] = nrm


def pack_occupancy(grid: torch.Tensor) -> torch.Tensor:
    """int32 words of a bool [G, G, G] grid indexed [x][y][z]: bit ``key & 31`` of word ``key >> 5``, key = (x * G + y) * G + z
    (the layout of ``OctreeAS.packed_occupancy``)."""
    bits = grid.reshape(-1).to(torch.int64)
    pad = (-bits.shape[0]) % 32
    if pad:
        bits = torch.cat([bits, bits.new_zeros(pad)])
    words = (bits.view(-1, 32) << torch.arange(32, device=bits.device)).sum(dim=1)
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)


class OctreeSampledSDFDataset(SDFDataset):
    """Samples limited to the occupied cells of an octree built from a mesh (``OctreeAS.from_triangles``, which keeps the mesh
    in ``extent``). A pool is made once -- per entry of ``sample_mode`` ``cells * samples_per_voxel`` samples ('rand': that
    many per occupied cell; 'near': noise of 1 / 2^level; 'trace'), those outside the occupied cells dropped inside the
    sampling kernel -- with distances for all of it; ``resample()`` draws ``num_samples`` of the pool. The pool holds every
    'rand' segment first, then the others as listed, the reference's order. Where the reference sizes the surface segments
    by the first 'rand' segment, ``cells * samples_per_voxel`` is used directly, so a ``sample_mode`` without 'rand' works.

    A reproduced quirk: ``resample()`` permutes ``pool_size - 1`` indices, as the reference does, so the last row of the
    pool is never drawn. Beyond the reference: ``seed``; the pool and working set k are functions of (seed, k)."""

    def __init__(self, occupancy_struct, split, transform=None, sample_mode=None, num_samples=100000, sample_tex=False,
                 samples_per_voxel=32, seed=0):
        super().__init__(split=split, transform=transform)
        self.blas = occupancy_struct
        self.sample_mode = list(sample_mode) if sample_mode is not None else list(_DEFAULT_MODES)
        self.num_samples, self.sample_tex, self.samples_per_voxel = num_samples, sample_tex, samples_per_voxel
        self.seed = int(seed)
        self.resample_count = 0
        self.validate()
        self.data_pool = None
        self.segment_counts = []
        self.load()

    @staticmethod
    def supports_blas(blas) -> bool:
        """The structure must be an octree that kept the mesh it was built from."""
        from ..accelstructs import OctreeAS
        return isinstance(blas, OctreeAS) and "vertices" in blas.extent and "faces" in blas.extent

    def validate(self) -> None:
        if not self.supports_blas(self.blas):
            raise RuntimeError("The Octree acceleration structure was not initialized from a mesh. To use "
                               "an OctreeAS with this dataset, make sure to construct it with a mesh.")

    @classmethod
    def is_root_of_dataset(cls, root, files_list=None) -> bool:
        return False          # made from a structure in memory, never from a path

    def _sample_from_grid(self, blas, samples_per_voxel=32):
        from ... import hip_ops
        mesh = _mesh_ops()
        vertices, faces, level = blas.extent["vertices"], blas.extent["faces"], blas.max_level
        hip_ops._need_gpu(vertices)
        dev = vertices.device
        faces = faces.to(dev)
        for mode in self.sample_mode:
            if mode not in ("rand", "near", "trace"):
                raise Exception(f"Sampling mode {mode} not implemented")
        if self.sample_tex and not all(k in blas.extent for k in ("texv", "texf", "mats")):
            raise RuntimeError("OctreeSampledSDFDataset(sample_tex=True) needs the texture coordinates, texture faces and "
                               "materials of the mesh in blas.extent['texv'], ['texf'] and ['mats'] "
                               "(wisp.ops.mesh.load_obj_materials)")
        corners = blas.points.to(dev)
        words = blas.packed_occupancy(level)
        words = pack_occupancy(blas.occupancy_at(level, dev)) if words is None else words.to(dev)
        triangles = vertices[faces.long()]
        cdf = hip_ops.mesh_face_cdf(triangles) if any(m != "rand" for m in self.sample_mode) else None
        n = corners.shape[0] * int(samples_per_voxel)
        key = _resample_key(self.seed, 0)
        order = [k for k, m in enumerate(self.sample_mode) if m == "rand"] + \
                [k for k, m in enumerate(self.sample_mode) if m != "rand"]
        pts, self.segment_counts = [], []
        for k in order:
            mode = self.sample_mode[k]
            common = dict(seed=key, segment=k, occupancy=words, occupancy_level=level)
            if mode == "rand":
                out = hip_ops.mesh_sample("cells", corners=corners, samples_per_cell=samples_per_voxel, cell_level=level,
                                          **common)
            else:
                out = hip_ops.mesh_sample("near" if mode == "near" else "surface", n, triangles=triangles, cdf=cdf,
                                          sigma=1.0 / (2 ** level), **common)
            pts.append(out.points)
            self.segment_counts.append(int(out.block_counts.sum().item()))
        pts = torch.cat(pts, dim=0) if pts else torch.empty((0, 3), dtype=torch.float32, device=dev)
        rgb = None
        if self.sample_tex:
            rgb, _, d = mesh.closest_tex(vertices, faces, blas.extent["texv"], blas.extent["texf"], blas.extent["mats"], pts)
        else:
            d = mesh.compute_sdf(vertices, faces, pts)
        data = dict(coords=pts, sdf=d)
        if rgb is not None:
            data["rgb"] = rgb
        return data

    def load(self) -> None:
        self.data_pool = self._sample_from_grid(self.blas, self.samples_per_voxel)
        self.resample()

    @property
    def pool_size(self) -> int:
        """Samples in the pool, before ``resample()`` draws from it."""
        return self.data_pool["coords"].shape[0]

    def resample(self) -> None:
        """A new working set: the first ``num_samples`` of a seeded permutation of the pool's rows but the last (the
        reference's ``randperm(pool_size - 1)``), on the device."""
        if self.pool_size < 1:
            raise RuntimeError("OctreeSampledSDFDataset: no sample fell into an occupied cell, the pool is empty")
        dev = self.data_pool["coords"].device
        gen = torch.Generator(device=dev).manual_seed(_resample_key(self.seed, self.resample_count) & ((1 << 63) - 1))
        self.resample_count += 1
        idx = torch.randperm(self.pool_size - 1, device=dev, generator=gen)
        if self.num_samples is not None and self.num_samples < self.pool_size:
            idx = idx[:self.num_samples]
        self.data = {k: v[idx] for k, v in self.data_pool.items() if v is not None}
