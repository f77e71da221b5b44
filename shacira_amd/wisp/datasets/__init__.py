"""Datasets: images and cameras kept on the device as bytes; rays, coordinates and colours made on demand by fused kernels;
signed-distance working sets sampled from a mesh on the device."""
from .multiview_dataset import NeRFSyntheticDataset  # noqa: F401
from .rtmv_dataset import RTMVDataset  # noqa: F401
from .image_dataset import MultiImageDataset  # noqa: F401
from .ray_sampler import SampleRays  # noqa: F401
from .batch import Batch, SDFBatch  # noqa: F401
from .sdf_dataset import MeshSampledSDFDataset, OctreeSampledSDFDataset, SDFDataset  # noqa: F401
