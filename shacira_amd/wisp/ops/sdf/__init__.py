"""Signed-distance metrics of the reference's ``wisp.ops.sdf``."""
from .metrics import compute_sdf_iou, compute_sparse_sdf_iou  # noqa: F401
