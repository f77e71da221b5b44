"""Point sampling on and around a triangle mesh: the samplers of the reference's ``wisp.ops.mesh``. Random numbers are drawn
on the device of ``V`` (the reference draws on the host and copies).

Every sampler takes ``seed=None``. None is the torch-op chain on torch's global generator. An int seed takes the fused kernel of
mesh_sample.hip (``hip_ops.mesh_sample``; contract: include/shacira_hip.h, shacira_mesh_sample): one launch, every sample a
pure function of (seed, sample index, segment), so a sample set can be restated and reproduced. The seeded path needs ``V`` on
the GPU; ``distrib`` is then not used (faces are chosen from the integer area CDF) unless it is the int32 CDF tensor of
``hip_ops.mesh_face_cdf``, which saves building it again."""
import torch


def _seeded(mode, V, F, num_samples, seed, segment=0, distrib=None, **kwargs):
    from .... import hip_ops
    hip_ops._need_gpu(V)
    cdf = distrib if isinstance(distrib, torch.Tensor) else None
    return hip_ops.mesh_sample(mode, num_samples, seed=seed, segment=segment, triangles=V[F.to(V.device).long()], cdf=cdf,
                               **kwargs)


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


def sample_surface(V: torch.Tensor, F: torch.Tensor, num_samples: int, distrib=None, seed=None, segment=0):
    """Uniform samples on the surface: (points [n, 3], the normals of their faces [n, 3])."""
    if seed is not None:
        out = _seeded("surface", V, F, num_samples, seed, segment, distrib, want_normals=True)
        return out.points.to(V.dtype), out.normals.to(V.dtype)
    fidx, normals = random_face(V, F, num_samples, distrib)
    tri = V[fidx]
    # sqrt of the first variate makes the barycentric point uniform over the triangle
    u = torch.sqrt(torch.rand(num_samples, 1, device=V.device, dtype=V.dtype))
    v = torch.rand(num_samples, 1, device=V.device, dtype=V.dtype)
    return (1 - u) * tri[:, 0] + (u * (1 - v)) * tri[:, 1] + (u * v) * tri[:, 2], normals


def sample_near_surface(V: torch.Tensor, F: torch.Tensor, num_samples: int, variance: float = 0.01, distrib=None, seed=None,
                        segment=0):
    """Surface samples displaced by Gaussian noise; ``variance`` is the noise's standard deviation (the reference's name)."""
    if seed is not None:
        return _seeded("near", V, F, num_samples, seed, segment, distrib, sigma=variance).points.to(V.dtype)
    samples = sample_surface(V, F, num_samples, distrib)[0]
    return samples + torch.randn_like(samples) * variance


def sample_uniform(num_samples: int, seed=None, device=None, segment=0):
    """Uniform samples in [-1, 1]^3, [n, 3]: on the host, or on ``device``. With a ``seed`` from the kernel, on the GPU."""
    if seed is not None:
        from .... import hip_ops
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            hip_ops._need_gpu(torch.empty(0))
        return hip_ops.mesh_sample("cube", num_samples, seed=seed, segment=segment, device=dev).points
    if device is not None:
        return torch.rand(num_samples, 3, device=device) * 2.0 - 1.0
    return torch.rand(num_samples, 3) * 2.0 - 1.0


def point_sample(V: torch.Tensor, F: torch.Tensor, techniques: list, num_samples: int, seed=None, distrib=None):
    """``num_samples`` points per entry of ``techniques`` ('trace': on the surface, 'near': near it, 'rand': uniform in the
    cube), concatenated in that order: [len(techniques) * num_samples, 3]. With a ``seed``: one kernel launch per technique,
    its segment the technique's position in the list, 'near' with the reference's default ``variance = 0.01``; ``distrib``
    may bring the mesh's ``hip_ops.mesh_face_cdf``."""
    if seed is not None:
        from .... import hip_ops
        hip_ops._need_gpu(V)
        modes = {"trace": "surface", "near": "near", "rand": "cube"}
        for technique in techniques:
            if technique not in modes:
                raise ValueError(f"point_sample: unknown technique {technique!r} (expected 'trace', 'near' or 'rand')")
        triangles = V[F.to(V.device).long()]
        if distrib is None and ("trace" in techniques or "near" in techniques):
            distrib = hip_ops.mesh_face_cdf(triangles)
        samples = [hip_ops.mesh_sample(modes[t], num_samples, seed=seed, segment=k, triangles=triangles, cdf=distrib,
                                       sigma=0.01, device=V.device).points for k, t in enumerate(techniques)]
        return torch.cat(samples, dim=0).to(V.dtype)
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
