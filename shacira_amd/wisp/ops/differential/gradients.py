"""Gradients of a scalar field ``f``: x [..., 3] -> [..., 1] (reference wisp/ops/differential/gradients.py), in torch: the
field's own lookups are the HIP kernels."""
import torch


def autodiff_gradient(x, f):
    """d f / d x by autograd (the graph is kept, so the result can be differentiated again)."""
    with torch.enable_grad():
        x = x.requires_grad_(True)
        y = f(x)
        return torch.autograd.grad(y, x, grad_outputs=torch.ones_like(y), create_graph=True)[0]


def finitediff_gradient(x, f, eps=0.005):
    """Central differences along the three axes: (f(x + eps e_k) - f(x - eps e_k)) / (2 eps); six evaluations."""
    steps = torch.eye(3, dtype=x.dtype, device=x.device) * eps
    return torch.cat([f(x + steps[k]) - f(x - steps[k]) for k in range(3)], dim=-1) / (2.0 * eps)


def tetrahedron_gradient(x, f, eps=0.005):
    """Four evaluations at the corners k_j of a tetrahedron: sum_j k_j f(x + eps k_j) / (4 eps)."""
    corners = torch.tensor([[1.0, -1.0, -1.0], [-1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, 1.0, 1.0]], dtype=x.dtype,
                           device=x.device)
    total = 0.0
    for k in corners:
        total = total + k * f((x + eps * k).detach())
    return total / (4.0 * eps)
