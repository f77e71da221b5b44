#!/usr/bin/env python3
"""Generate tests/golden/mesh_tex.npz by EXECUTING the reference's wisp/ops/mesh/barycentric_coordinates.py and sample_tex.py,
loaded by file path (they import only torch and numpy). Nothing of the reference is copied: the file holds the inputs drawn
here and the arrays the reference's functions returned for them.

Run:  python tests/golden/make_mesh_tex_golden.py <root of a checkout of the reference>

sample_tex     257 uvs uniform in [-0.5, 1.5]^2 (outside [0, 1]: reflection padding), four materials: 0 an 8x5x3 texture,
               1 a diffuse colour only, 2 a textured material no point uses, 3 a 4x4x4 texture (alpha is dropped).
barycentric    points on faces of the cube and of the level-2 icosphere (tests/mesh_sdf_ref.py; every angle >= 30 degrees):
               fp64 barycentric blends of the fp32 vertices, rounded to fp32.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mesh_sdf_ref as ref   # noqa: E402


def load(root, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "wisp", "ops", "mesh", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return getattr(module, name)


def face_points(rng, V, F, count):
    faces = rng.integers(0, F.shape[0], count)
    w = rng.dirichlet((1.0, 1.0, 1.0), count)
    T = V[F[faces]]
    P = (T.astype(np.float64) * w[:, :, None]).sum(axis=1).astype(np.float32)
    return P, T[:, 0], T[:, 1], T[:, 2]


def main(root):
    sample_tex = load(root, "sample_tex")
    barycentric_coordinates = load(root, "barycentric_coordinates")
    rng = np.random.default_rng(31)
    out = {}

    uv = rng.uniform(-0.5, 1.5, (257, 2)).astype(np.float32)
    tm = rng.choice(np.asarray([0, 1, 3]), 257).astype(np.int64)
    tex0 = rng.uniform(0, 1, (8, 5, 3)).astype(np.float32)
    tex2 = rng.uniform(0, 1, (3, 3, 3)).astype(np.float32)
    tex3 = rng.uniform(0, 1, (4, 4, 4)).astype(np.float32)
    diffuse1 = np.asarray([0.25, 0.5, 0.75], dtype=np.float32)
    diffuse3 = np.asarray([1.0, 0.0, 0.0], dtype=np.float32)      # ignored: the texture takes precedence
    materials = {0: {"diffuse_texname": torch.from_numpy(tex0)},
                 1: {"diffuse": torch.from_numpy(diffuse1)},
                 2: {"diffuse_texname": torch.from_numpy(tex2)},
                 3: {"diffuse": torch.from_numpy(diffuse3), "diffuse_texname": torch.from_numpy(tex3)}}
    rgb = sample_tex(torch.from_numpy(uv.copy()), torch.from_numpy(tm), materials)
    out.update(tex_uv=uv, tex_tm=tm, tex0=tex0, tex2=tex2, tex3=tex3, diffuse1=diffuse1, diffuse3=diffuse3,
               tex_rgb=rgb.numpy().astype(np.float32))

    parts = [face_points(rng, *ref.cube(0.5), 128), face_points(rng, *ref.icosphere(2, 0.7), 129)]
    P, A, B, C = (np.concatenate([p[k] for p in parts]) for k in range(4))
    L = barycentric_coordinates(*(torch.from_numpy(x) for x in (P, A, B, C)))
    out.update(bary_p=P, bary_a=A, bary_b=B, bary_c=C, bary_l=L.numpy().astype(np.float32))

    path = os.path.join(HERE, "mesh_tex.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
