"""``sample_tex`` of the reference (wisp/ops/mesh/sample_tex.py): diffuse colour of per-point (uv, material) pairs."""
import torch
import torch.nn.functional as F


def sample_tex(Tp: torch.Tensor, TM: torch.Tensor, materials):
    """RGB [N, 3] fp32 at the texture coordinates ``Tp`` [N, 2] of the materials ``TM`` [N] (integers; negative: none, black).

    ``materials[i]`` is a dict with an optional ``'diffuse'`` colour [3] and an optional ``'diffuse_texname'`` image
    [H, W, C >= 3] in [0, 1], which takes precedence: sampled bilinearly at ``uv * 2 - 1`` with v flipped, reflection
    padding, ``align_corners=True``. A material no point uses is skipped (its image is not touched). ``Tp`` is not
    modified (the reference flips it in place when it is a view)."""
    if TM.numel() == 0:
        return torch.zeros((0, 3), dtype=torch.float32, device=Tp.device)
    if int(TM.max()) < 0:
        raise ValueError("sample_tex: no materials detected; check the material definition of the mesh")
    rgb = torch.zeros((Tp.shape[0], 3), dtype=torch.float32, device=Tp.device)
    grid = Tp.to(torch.float32) * 2.0 - 1.0
    grid = torch.stack([grid[..., 0], -grid[..., 1]], dim=-1)
    for i in range(int(TM.max()) + 1):
        mask = TM == i
        if not bool(mask.any()):
            continue
        material = materials[i]
        if "diffuse_texname" not in material:
            if "diffuse" in material:
                rgb[mask] = material["diffuse"].to(device=Tp.device, dtype=torch.float32)
            continue
        image = material["diffuse_texname"][..., :3].permute(2, 0, 1)[None].to(device=Tp.device, dtype=torch.float32)
        sampled = F.grid_sample(image, grid[mask].reshape(1, -1, 1, 2), mode="bilinear", padding_mode="reflection",
                                align_corners=True)
        rgb[mask] = sampled[0, :, :, 0].permute(1, 0)
    return rgb
