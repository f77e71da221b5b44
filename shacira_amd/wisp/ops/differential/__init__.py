from .gradients import autodiff_gradient, finitediff_gradient, tetrahedron_gradient

__all__ = ["autodiff_gradient", "finitediff_gradient", "tetrahedron_gradient"]
