"""Mesh operators of the reference's ``wisp.ops.mesh``: OBJ loading (geometry, and with ``load_obj_materials`` texture
coordinates and diffuse materials), normalisation, surface / near-surface / uniform point sampling, ``compute_sdf`` and
``closest_point`` on the fused HIP kernels of ``mesh_sdf.hip`` (contracts: include/shacira_hip.h, shacira_mesh_sdf and
shacira_mesh_closest), and on top of ``closest_point`` the textured branch: ``barycentric_coordinates``, ``sample_tex``,
``closest_tex``.

Not mirrored: ``trimmesh`` and texture maps other than the diffuse one.
``load_obj(load_materials=True)`` still raises: ``load_obj_materials`` is the entry point for textured meshes."""
from .load_obj import load_obj, load_obj_materials
from .normalize import normalize
from .sampling import (area_weighted_distribution, per_face_normals, point_sample, random_face, sample_near_surface,
                       sample_surface, sample_uniform)
from .compute_sdf import compute_sdf, mesh_sdf_torch
from .closest_point import closest_point, mesh_closest_torch
from .barycentric_coordinates import barycentric_coordinates
from .sample_tex import sample_tex
from .closest_tex import closest_tex

__all__ = ["area_weighted_distribution", "barycentric_coordinates", "closest_point", "closest_tex", "compute_sdf",
           "load_obj", "load_obj_materials", "mesh_closest_torch", "mesh_sdf_torch", "normalize", "per_face_normals",
           "point_sample", "random_face", "sample_near_surface", "sample_surface", "sample_tex", "sample_uniform"]
