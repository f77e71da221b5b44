"""Ray generation: the reference's functions and the batched ``generate_rays`` over the fused HIP kernel."""
from .raygen import (camera_records, composite_colors, composite_rays, generate_2d_grid, generate_centered_pixel_coords,  # noqa: F401
                     generate_ortho_rays, generate_pinhole_rays, generate_rays, image_mip_torch)
