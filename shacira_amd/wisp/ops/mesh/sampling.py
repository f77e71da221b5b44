"""Point sampling on and around a triangle mesh: the samplers of the reference's ``wisp.ops.mesh``. Random numbers are drawn
on the device of ``V`` (the reference draws on the host and copies)."""
import torch


def per_face_normals(V: torch.Tensor, F: torch.Tensor):
    """Unnormalised face normals [F, 3]: cross(a - b, b - c), twice the face area long."""
    tri = V[F]
    return torch.cross(tri[:, 0] - tri[:, 1], tri[:, 1] - tri[:, 2], dim=-1)


def area_weighted_distribution(V: torch.Tensor, F: torch.Tensor, normals: torch.Tensor = None):
    """``torch.distributions.Categorical`` over the faces, proportional to their areas."""
    if normals is None:
        normals = per_face_normals(V, F)
    areas = torch.linalg.norm(normals, dim=1) * 0.5
    return torch.distributions.Categorical(areas / (areas.sum() + 1e-10))


def random_face(V: torch.Tensor, F: torch.Tensor, num_samples: int, distrib=None):
    """``num_samples`` faces drawn from ``distrib`` (area weighted by default): (vertex indices [n, 3], normals [n, 3])."""
    if distrib is None:
        distrib = area_weighted_distribution(V, F)
    idx = distrib.sample([num_samples])
    return F[idx], per_face_normals(V, F)[idx]


def sample_surface(V: torch.Tensor, F: torch.Tensor, num_samples: int, distrib=None):
    """Uniform samples on the surface: (points [n, 3], the normals of their faces [n, 3])."""
    fidx, normals = random_face(V, F, num_samples, distrib)
    tri = V[fidx]
    # sqrt of the first variate makes the barycentric point uniform over the triangle
    u = torch.sqrt(torch.rand(num_samples, 1, device=V.device, dtype=V.dtype))
    v = torch.rand(num_samples, 1, device=V.device, dtype=V.dtype)
    return (1 - u) * tri[:, 0] + (u * (1 - v)) * tri[:, 1] + (u * v) * tri[:, 2], normals


def sample_near_surface(V: torch.Tensor, F: torch.Tensor, num_samples: int, variance: float = 0.01, distrib=None):
    """Surface samples displaced by Gaussian noise; ``variance`` is the noise's standard deviation (the reference's name)."""
    samples = sample_surface(V, F, num_samples, distrib)[0]
    return samples + torch.randn_like(samples) * variance


def sample_uniform(num_samples: int):
    """Uniform samples in [-1, 1]^3, [n, 3] on the host."""
    return torch.rand(num_samples, 3) * 2.0 - 1.0


def point_sample(V: torch.Tensor, F: torch.Tensor, techniques: list, num_samples: int):
    """``num_samples`` points per entry of ``techniques`` ('trace': on the surface, 'near': near it, 'rand': uniform in the
    cube), concatenated in that order: [len(techniques) * num_samples, 3]."""
    distrib = area_weighted_distribution(V, F) if ("trace" in techniques or "near" in techniques) else None
    samples = []
    for technique in techniques:
        if technique == "trace":
            samples.append(sample_surface(V, F, num_samples, distrib)[0])
        elif technique == "near":
            samples.append(sample_near_surface(V, F, num_samples, distrib=distrib))
        elif technique == "rand":
            samples.append(sample_uniform(num_samples).to(device=V.device, dtype=V.dtype))
        else:
            raise ValueError(f"point_sample: unknown technique {technique!r} (expected 'trace', 'near' or 'rand')")
    return torch.cat(samples, dim=0)
