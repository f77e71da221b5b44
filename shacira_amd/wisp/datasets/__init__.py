"""Datasets: multiview images and cameras kept on the device, rays made on demand by the fused ray kernel."""
from .multiview_dataset import NeRFSyntheticDataset  # noqa: F401
from .ray_sampler import SampleRays  # noqa: F401
