"""Wavefront OBJ geometry: a plain-text parser of the ``v`` and ``f`` records (the reference goes through tinyobjloader,
which is not a dependency here)."""
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
        raise NotImplementedError("load_obj(load_materials=True): texture coordinates, material libraries and texture maps "
                                  "are outside this package (textures are not mirrored); only geometry is loaded")
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
