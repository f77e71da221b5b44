"""Mesh operators of the reference's ``wisp.ops.mesh``: OBJ loading, normalisation, surface / near-surface / uniform point
sampling, and ``compute_sdf`` on the fused HIP kernel of ``mesh_sdf.hip`` (contract: include/shacira_hip.h, shacira_mesh_sdf).

Not mirrored: textures and materials (``sample_tex``, ``closest_tex``, ``barycentric_coordinates``,
``load_obj(load_materials=True)``), ``closest_point`` (the reference's is an ``assert False``) and ``trimmesh``."""
from .load_obj import load_obj
from .normalize import normalize
from .sampling import (area_weighted_distribution, per_face_normals, point_sample, random_face, sample_near_surface,
                       sample_surface, sample_uniform)
from .compute_sdf import compute_sdf, mesh_sdf_torch

__all__ = ["area_weighted_distribution", "compute_sdf", "load_obj", "mesh_sdf_torch", "normalize", "per_face_normals",
           "point_sample", "random_face", "sample_near_surface", "sample_surface", "sample_uniform"]
