"""The reference's ``wisp.ops.spc`` as far as it makes sense on ``OctreeAS``'s dense bit grid: ``mesh_to_octree`` on the HIP
rasteriser of ``mesh_voxelize.hip`` (contract: include/shacira_hip.h, shacira_mesh_voxelize), ``pointcloud_to_octree``,
``dilate_points`` and the samplers ``sample_spc``, ``sample_from_depth_intervals`` and ``expand_pack_boundary``; and
``StructuredPointCloud``, a coloured SPC of one level in the layout the kernels of spc.hip build and trace.

Stated deviations: the conversions return an ``OctreeAS``, not kaolin's byte octree (nothing in this package reads one), and
``mesh_to_octree`` rasterises exactly instead of sampling. Not mirrored: ``create_dense_octree`` (``OctreeAS.make_dense``),
``make_trilinear_spc`` (``wisp.ops.octree.build_octree_index``), ``octree_to_spc`` and the kaolin-format conversions."""
from .conversions import mesh_to_octree, pointcloud_to_octree
from .processing import dilate_points
from .sampling import expand_pack_boundary, sample_from_depth_intervals, sample_spc

__all__ = ["dilate_points", "expand_pack_boundary", "mesh_to_octree", "pointcloud_to_octree", "sample_from_depth_intervals",
           "sample_spc"]
from .structured import StructuredPointCloud  # noqa: E402

__all__.append("StructuredPointCloud")
