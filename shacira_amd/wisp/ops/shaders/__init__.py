"""View shaders (reference wisp/ops/shaders): matcap shading and the point-light shadow, on the kernels of shade.hip."""
from .matcap import matcap_shader, matcap_sampler, default_matcap, sample_matcap_torch  # noqa: F401
from .shadow_rays import pointlight_shadow_shader, gaussian_blur_torch  # noqa: F401
