"""Wavefront OBJ: a plain-text parser (the reference goes through tinyobjloader, which is not a dependency here).
``load_obj`` reads the geometry (``v`` and ``f`` records); ``load_obj_materials`` also reads texture coordinates, per-face
materials and the diffuse part of the material libraries."""
import os

import torch


def _vertex_index(token, count):
    """The vertex part of an ``f`` token (``i``, ``i/j``, ``i/j/k``, ``i//k``), 0-based; negative indices count back from
    the ``count`` vertices read so far."""
    i = int(token.split("/", 1)[0])
    if i == 0:
        raise ValueError("OBJ vertex indices start at 1")
    return i - 1 if i > 0 else count + i


def load_obj(fname: str, load_materials: bool = False):
    """Vertices (FloatTensor [V, 3]) and triangles (LongTensor [F, 3]) of a Wavefront .obj file. Polygons are
    fan-triangulated (v0, v_k, v_k+1); everything but ``v`` and ``f`` records is ignored, and so are the vertex colours some
    exporters append to ``v``."""
    if load_materials:
        raise NotImplementedError("load_obj(load_materials=True): load_obj returns geometry only; texture coordinates, "
                                  "material libraries and diffuse texture maps come from load_obj_materials(fname)")
    vertices, faces = [], []
    with open(fname) as fh:
        for line in fh:
            fields = line.split("#", 1)[0].split()
            if not fields:
                continue
            if fields[0] == "v":
                if len(fields) < 4:
                    raise ValueError(f"{fname}: vertex record with fewer than three coordinates: {line.strip()!r}")
                vertices.append([float(x) for x in fields[1:4]])
            elif fields[0] == "f":
                corner = [_vertex_index(tok, len(vertices)) for tok in fields[1:]]
                if len(corner) < 3:
                    raise ValueError(f"{fname}: face with fewer than three vertices: {line.strip()!r}")
                for k in range(1, len(corner) - 1):
                    faces.append([corner[0], corner[k], corner[k + 1]])
    V = torch.tensor(vertices, dtype=torch.float32).reshape(-1, 3)
    F = torch.tensor(faces, dtype=torch.long).reshape(-1, 3)
    if F.numel() and (int(F.min()) < 0 or int(F.max()) >= V.shape[0]):
        raise ValueError(f"{fname}: face index outside the {V.shape[0]} vertices")
    return V, F


def _texcoord_index(token, count):
    """The texture-coordinate part of an ``f`` token, 0-based, -1 when the token has none."""
    parts = token.split("/")
    if len(parts) < 2 or parts[1] == "":
        return -1
    j = int(parts[1])
    if j == 0:
        raise ValueError("OBJ texture-coordinate indices start at 1")
    return j - 1 if j > 0 else count + j


def _load_image(path):
    """float [H, W, C] in [0, 1] (C = 3, or 4 with alpha)."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as img:
        if img.mode not in ("RGB", "RGBA"):
            img = img.convert("RGB")
        return torch.from_numpy(np.array(img, dtype=np.float32)) / 255.0


def _load_mtl(path, parent, names, mats):
    """Appends the materials of one ``.mtl`` file: ``newmtl``, ``Kd`` and ``map_Kd`` (its options are not interpreted: the
    last field is the file, relative to ``parent``)."""
    current = None
    with open(path) as fh:
        for line in fh:
            fields = line.split("#", 1)[0].split()
            if not fields:
                continue
            if fields[0] == "newmtl":
                current = {"diffuse": torch.zeros(3, dtype=torch.float32)}
                names.setdefault(" ".join(fields[1:]), len(mats))
                mats[len(mats)] = current
            elif current is None:
                continue
            elif fields[0] == "Kd":
                if len(fields) < 4:
                    raise ValueError(f"{path}: Kd record with fewer than three components: {line.strip()!r}")
                current["diffuse"] = torch.tensor([float(x) for x in fields[1:4]], dtype=torch.float32)
            elif fields[0] == "map_Kd" and len(fields) > 1:
                current["diffuse_texname"] = _load_image(os.path.join(parent, fields[-1]))


def load_obj_materials(fname: str):
    """``(V [#V, 3] float, F [#F, 3] long, texv [#VT, 2] float, texf [#F, 4] long, mats)`` of a Wavefront .obj file with its
    material libraries: what the reference's ``load_obj(fname, load_materials=True)`` returns.

    ``texf`` holds per triangle three indices into ``texv`` (-1: the corner has no texture coordinate) and the material id
    (-1: no ``usemtl`` in force, or an unknown name). ``mats[i]`` is a dict with ``'diffuse'`` ([3], the ``Kd`` colour, zeros
    by default) and, for a ``map_Kd``, ``'diffuse_texname'``: the image as float [H, W, C] / 255, its path relative to the
    OBJ. Materials are numbered in the order of their ``newmtl`` records over the ``mtllib`` files. Polygons are
    fan-triangulated exactly as ``load_obj`` does, so ``V`` and ``F`` equal its result. Other texture maps are not read."""
    parent = os.path.dirname(fname)
    vertices, texcoords, faces, texfaces, face_material = [], [], [], [], []
    names, mats, material = {}, {}, None
    with open(fname) as fh:
        for line in fh:
            fields = line.split("#", 1)[0].split()
            if not fields:
                continue
            if fields[0] == "v":
                if len(fields) < 4:
                    raise ValueError(f"{fname}: vertex record with fewer than three coordinates: {line.strip()!r}")
                vertices.append([float(x) for x in fields[1:4]])
            elif fields[0] == "vt":
                if len(fields) < 3:
                    raise ValueError(f"{fname}: texture-coordinate record with fewer than two coordinates: {line.strip()!r}")
                texcoords.append([float(x) for x in fields[1:3]])
            elif fields[0] == "mtllib":
                for lib in fields[1:]:      # a library that does not exist defines nothing, as for tinyobjloader
                    if os.path.exists(os.path.join(parent, lib)):
                        _load_mtl(os.path.join(parent, lib), parent, names, mats)
            elif fields[0] == "usemtl":
                material = " ".join(fields[1:])
            elif fields[0] == "f":
                corner = [_vertex_index(tok, len(vertices)) for tok in fields[1:]]
                tex = [_texcoord_index(tok, len(texcoords)) for tok in fields[1:]]
                if len(corner) < 3:
                    raise ValueError(f"{fname}: face with fewer than three vertices: {line.strip()!r}")
                for k in range(1, len(corner) - 1):
                    faces.append([corner[0], corner[k], corner[k + 1]])
                    texfaces.append([tex[0], tex[k], tex[k + 1]])
                    face_material.append(material)
    V = torch.tensor(vertices, dtype=torch.float32).reshape(-1, 3)
    F = torch.tensor(faces, dtype=torch.long).reshape(-1, 3)
    if F.numel() and (int(F.min()) < 0 or int(F.max()) >= V.shape[0]):
        raise ValueError(f"{fname}: face index outside the {V.shape[0]} vertices")
    texv = torch.tensor(texcoords, dtype=torch.float32).reshape(-1, 2)
    texf = torch.tensor([t + [names.get(m, -1)] for t, m in zip(texfaces, face_material)], dtype=torch.long).reshape(-1, 4)
    if texf.numel() and (int(texf[:, :3].min()) < -1 or int(texf[:, :3].max()) >= texv.shape[0]):
        raise ValueError(f"{fname}: texture-coordinate index outside the {texv.shape[0]} records")
    return V, F, texv, texf, mats
