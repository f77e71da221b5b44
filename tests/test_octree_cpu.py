"""OctreeGrid / CodebookOctreeGrid without a GPU: the coarser levels of ``OctreeAS``, the corner index, the fp64 restatement
(tests/octree_ref.py) against a direct lattice evaluation and against finite differences, ``octree_torch`` on the host, the
modules' construction and interface, the codebook's per-corner decode against a per-sample restatement of the reference,
and the validation codes of the shacira_octree_* entry points (validation precedes any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import octree_ref as oref
from shacira_amd import _lib
from shacira_amd.wisp.accelstructs import OctreeAS
from shacira_amd.wisp.models.grids import CodebookOctreeGrid, OctreeGrid
from shacira_amd.wisp.ops import octree as octree_ops


# ---- occupancies -----------------------------------------------------------------------------------------------------------
shell_cells, random_cells = oref.shell_cells, oref.random_cells


def morton(cells, level):
    m = np.zeros(cells.shape[0], dtype=np.int64)
    for b in range(level):
        m |= (((cells[:, 0] >> b) & 1) << (3 * b + 2)) | (((cells[:, 1] >> b) & 1) << (3 * b + 1)) \
            | (((cells[:, 2] >> b) & 1) << (3 * b))
    return m


OCCUPANCIES = [("shell", 6), ("random", 5)]


def make_as(kind, level):
    cells = shell_cells(level) if kind == "shell" else random_cells(level)
    return OctreeAS.from_quantized_points(torch.from_numpy(cells), level), cells


def np_level_cells(cells, max_level, level):
    """Morton-sorted unique cells of a coarser level."""
    c = np.unique(cells >> (max_level - level), axis=0)
    return c[np.argsort(morton(c, level))]


def np_query(cells, max_level, level, coords):
    G = 1 << level
    occ = np.zeros((G, G, G), dtype=bool)
    c = cells >> (max_level - level)
    occ[c[:, 0], c[:, 1], c[:, 2]] = True
    inside, cell, _ = oref.locate(coords, level)
    hit = inside & occ[cell[:, 0], cell[:, 1], cell[:, 2]]
    return np.where(hit, morton(cell, level), -1)


# ---- the pyramid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,max_level", OCCUPANCIES)
def test_pyramid_levels_and_queries(kind, max_level):
    blas, cells = make_as(kind, max_level)
    assert blas.points.dtype == torch.int16 and blas.pyramid.shape == (2, 1)       # unchanged
    assert torch.equal(blas.level_points(max_level), blas.points)
    rng = np.random.default_rng(1)
    coords = rng.uniform(-1.2, 1.2, (4000, 3)).astype(np.float32)
    coords[:6] = [[1.0, 0, 0], [0, np.nan, 0], [np.inf, 0, 0], [0, 0, -np.inf], [-1.0, -1.0, -1.0], [0.999, 1.0, 0.2]]
    # samples inside occupied cells as well, so that the hits are many
    pick = cells[rng.integers(0, cells.shape[0], 2000)]
    coords[2000:] = ((pick + rng.uniform(0.01, 0.99, pick.shape)) * (2.0 / (1 << max_level)) - 1.0).astype(np.float32)
    tc = torch.from_numpy(coords)
    for level in range(max_level + 1):
        pts = blas.level_points(level)
        assert pts.dtype == torch.int16
        assert np.array_equal(pts.numpy().astype(np.int64), np_level_cells(cells, max_level, level))
        want = np_query(cells, max_level, level, coords)
        got = blas.query(tc, level).pidx.numpy()
        assert np.array_equal(got, want)
        assert (got[:4] == -1).all()                       # x = 1.0, NaN, +-inf
        assert (got >= 0).sum() > 500
    assert np.array_equal(blas.query(tc).pidx.numpy(), np_query(cells, max_level, max_level, coords))
    par = blas.query(tc, max_level, with_parents=True).pidx.numpy()
    assert par.shape == (coords.shape[0], max_level + 1)
    for level in range(max_level + 1):
        assert np.array_equal(par[:, level], np_query(cells, max_level, level, coords))
    with pytest.raises(ValueError):
        blas.query(tc, max_level + 1)


def test_coarse_levels_are_cached_and_dropped_with_the_occupancy():
    blas, _ = make_as("random", 5)
    a = blas.occupancy_at(3)
    assert blas.occupancy_at(3) is a
    blas.occupancy_grid = blas.occupancy_grid.clone()
    blas.occupancy_grid[:] = False
    assert blas.occupancy_at(3) is not a and not blas.occupancy_at(3).any()
    b = blas.occupancy_at(3)
    blas.occupancy_grid[:] = True                      # written in place: stale until the owner says so
    assert blas.occupancy_at(3) is b
    blas.occupancy_changed()
    assert blas.occupancy_at(3).all()


def test_from_pointcloud_quantises_like_query():
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(rng.uniform(-1, 1, (500, 3)).astype(np.float32))
    pts[0] = torch.tensor([1.0, -1.0, 1.0])
    blas = OctreeAS.from_pointcloud(pts, 4)
    inside = (pts < 1.0).all(-1)
    assert (blas.query(pts[inside], 4).pidx >= 0).all()
    want = np.unique(np.clip(np.floor(16 * (pts.numpy() + 1.0) / 2.0), 0, 15).astype(np.int64), axis=0)
    assert blas.points.shape[0] == want.shape[0]
    for fn in (OctreeAS.from_mesh, OctreeAS.from_spc, OctreeGrid.from_mesh, CodebookOctreeGrid.from_spc):
        with pytest.raises(NotImplementedError):
            fn("mesh.obj", 4)


# ---- the corner index ------------------------------------------------------------------------------------------------------
def np_corner_keys(cells, level):
    S = (1 << level) + 1
    q = (cells[:, None, :] + oref.CORNERS[None]).reshape(-1, 3)
    return np.unique((q[:, 0] * S + q[:, 1]) * S + q[:, 2])


@pytest.mark.parametrize("kind,max_level", OCCUPANCIES + [("dense", 4)])
def test_corner_index(kind, max_level):
    if kind == "dense":
        blas = OctreeAS.make_dense(max_level)
        cells = blas.points.numpy().astype(np.int64)
    else:
        blas, cells = make_as(kind, max_level)
    levels = list(range(max(0, max_level - 3), max_level + 1))
    index = octree_ops.build_octree_index(blas, levels)
    for level in levels:
        li = index[level]
        S = (1 << level) + 1
        lp = blas.level_points(level).numpy().astype(np.int64)
        pd = li.points_dual.numpy().astype(np.int64)
        tr = li.trinkets.numpy()
        assert li.points_dual.dtype == torch.int16 and li.trinkets.dtype == torch.int32 and tr.shape == (lp.shape[0], 8)
        for k in range(8):
            assert np.array_equal(pd[tr[:, k]], lp + oref.CORNERS[k])
        keys = (pd[:, 0] * S + pd[:, 1]) * S + pd[:, 2]
        assert np.all(np.diff(keys) > 0)                                  # unique, and the documented order
        assert np.array_equal(keys, np_corner_keys(np_level_cells(cells, max_level, level), level))
        assert li.rows == keys.shape[0]
        if kind == "dense":
            assert li.rows == S ** 3
        # what the kernels read: bits and counts agree with the rows
        ci = li.corner_index.numpy().astype(np.int64) & 0xFFFFFFFF
        word, bit = keys >> 5, keys & 31
        assert np.all((ci[word, 0] >> bit) & 1)
        below = np.array([bin(int(ci[w, 0]) & ((1 << int(b)) - 1)).count("1") for w, b in zip(word, bit)])
        assert np.array_equal(ci[word, 1] + below, np.arange(keys.shape[0]))
        assert sum(bin(int(v)).count("1") for v in ci[:, 0]) == keys.shape[0]
        occ = li.occupancy.numpy().astype(np.int64) & 0xFFFFFFFF
        G = 1 << level
        ck = (lp[:, 0] * G + lp[:, 1]) * G + lp[:, 2]
        assert np.all((occ[ck >> 5] >> (ck & 31)) & 1) and sum(bin(int(v)).count("1") for v in occ) == lp.shape[0]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def _np_index(index, levels):
    return ([index[l].level_points.numpy() for l in levels], [index[l].trinkets.numpy() for l in levels])


def test_restatement_on_a_dense_grid_is_lattice_trilinear():
    rng = np.random.default_rng(4)
    level, Fd = 3, 3
    S = (1 << level) + 1
    blas = OctreeAS.make_dense(level)
    index = octree_ops.build_octree_index(blas, [level])
    lattice = rng.standard_normal((S, S, S, Fd))
    table = np.concatenate([lattice.reshape(-1, Fd), np.full((1, Fd), 99.0)])    # linear key order + the padding row
    coords = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    lp, tr = _np_index(index, [level])
    got = oref.forward(coords, [level], lp, tr, [table], True)
    p = (coords.astype(np.float32) + np.float32(1)) * np.float32(4)
    c = np.floor(p).astype(np.int64)
    t = (p - np.floor(p)).astype(np.float64)
    want = np.zeros((500, Fd))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (t[:, 0] if dx else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dz else 1 - t[:, 2])
                want += w[:, None] * lattice[c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz]
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("summed", [True, False])
def test_restatement_backward_is_the_derivative_of_its_forward(summed):
    rng = np.random.default_rng(5)
    blas, cells = make_as("random", 5)
    levels = [3, 5]
    index = octree_ops.build_octree_index(blas, levels)
    lp, tr = _np_index(index, levels)
    tables = [rng.standard_normal((index[l].rows + 1, 2)) for l in levels]
    pick = cells[rng.integers(0, cells.shape[0], 40)]
    coords = (pick + rng.uniform(0.1, 0.9, pick.shape)) * (2.0 / 32) - 1.0       # away from the faces of level 5
    coords = np.concatenate([coords, rng.uniform(-1.2, 1.2, (20, 3))])
    coords = coords[np.all(np.abs((coords + 1) * 16 - np.round((coords + 1) * 16)) > 1e-3, axis=-1)]
    f = lambda c, tb: oref.forward(c, levels, lp, tr, tb, summed, index_dtype=np.float64)   # noqa: E731
    go = rng.standard_normal(f(coords, tables).shape)
    gt, gc, gs = oref.backward(coords, levels, lp, tr, tables, go, summed, index_dtype=np.float64)
    h = 1e-6
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = ((f(coords + e, tables) - f(coords - e, tables)) * go).sum(-1) / (2 * h)
        np.testing.assert_allclose(gc[:, a], fd, rtol=1e-6, atol=1e-6)
        assert np.all(np.abs(gc[:, a]) <= gs[:, a] + 1e-12)
    for l in range(len(levels)):
        assert np.all(gt[l][-1] == 0)
        for row in rng.integers(0, tables[l].shape[0] - 1, 25):
            for j in range(2):
                tp = [t.copy() for t in tables]
                tm = [t.copy() for t in tables]
                tp[l][row, j] += h
                tm[l][row, j] -= h
                fd = ((f(coords, tp) - f(coords, tm)) * go).sum() / (2 * h)
                assert abs(gt[l][row, j] - fd) <= 1e-6 * max(1.0, abs(fd))


@pytest.mark.parametrize("summed", [True, False])
def test_octree_torch_on_the_host_agrees_with_the_restatement(summed):
    rng = np.random.default_rng(6)
    blas, cells = make_as("shell", 6)
    levels = [3, 4, 5, 6]
    index = octree_ops.build_octree_index(blas, levels)
    lp, tr = _np_index(index, levels)
    tables = [torch.from_numpy(rng.standard_normal((index[l].rows + 1, 5))).requires_grad_(True) for l in levels]
    coords = rng.uniform(-1.2, 1.2, (3000, 3)).astype(np.float32)
    pick = cells[rng.integers(0, cells.shape[0], 1500)]
    coords[1500:] = ((pick + rng.uniform(0, 1, pick.shape)) * (2.0 / 64) - 1.0).astype(np.float32)
    coords[:3] = [[np.nan, 0, 0], [np.inf, 0, 0], [1.0, 1.0, 1.0]]
    tc = torch.from_numpy(coords).requires_grad_(True)
    out = octree_ops.octree_torch(tc, levels, tables, index, summed)
    nt = [t.detach().numpy() for t in tables]
    ref = oref.forward(coords, levels, lp, tr, nt, summed)
    assert out.dtype == torch.float64 and out.shape == ref.shape
    np.testing.assert_allclose(out.detach().numpy(), ref, rtol=1e-12, atol=1e-12)
    assert (np.abs(ref).sum(-1) > 0).sum() > 1000
    go = rng.standard_normal(ref.shape)
    grads = torch.autograd.grad(out, [tc, *tables], torch.from_numpy(go))
    gt, gc, _ = oref.backward(coords, levels, lp, tr, nt, go, summed)
    np.testing.assert_allclose(grads[0].numpy(), gc, rtol=1e-4, atol=1e-4)       # the coordinates are fp32
    for a, b in zip(grads[1:], gt):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-11, atol=1e-11)


# ---- the modules -----------------------------------------------------------------------------------------------------------
def test_octree_grid_attributes_initialisation_and_interface():
    torch.manual_seed(0)
    g = OctreeGrid.make_dense(feature_dim=5, base_lod=3, num_lods=3, multiscale_type="sum", feature_std=0.1,
                              feature_bias=0.5)
    assert (g.feature_dim, g.base_lod, g.num_lods, g.active_lods, g.max_lod) == (5, 3, 3, [3, 4, 5], 5)
    assert (g.interpolation_type, g.multiscale_type, g.feature_std, g.feature_bias) == ("linear", "sum", 0.1, 0.5)
    assert [n for n, _ in g.named_parameters()] == ["features.0", "features.1", "features.2"]
    assert [tuple(p.shape) for p in g.features] == [((2 ** l + 1) ** 3 + 1, 5) for l in (3, 4, 5)]
    assert int(g.num_feat) == sum((2 ** l + 1) ** 3 + 1 for l in (3, 4, 5))
    assert set(g.points_dual) == set(g.trinkets) == {3, 4, 5} and g.trinkets[5].shape == (32 ** 3, 8)
    big = g.features[2].detach()
    assert abs(float(big.mean()) - 0.5) < 3e-3 and abs(float(big.std()) - 0.1) < 3e-3
    # the reference's draws, in level order
    torch.manual_seed(0)
    for p in g.features:
        fts = torch.zeros(p.shape) + 0.5
        fts += torch.randn_like(fts) * 0.1
        assert torch.equal(p.detach(), fts)
    assert g.supported_blas() == {OctreeAS} and g.name() == "Octree Grid"
    assert g.public_properties()["Active feature LODs"] == ["3", "4", "5"]
    assert OctreeGrid.max_octree_lod(3, 3) == 5
    g.freeze()
    assert not any(p.requires_grad for p in g.parameters())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.interpolate(torch.zeros(4, 3), 2)
    with pytest.raises(NotImplementedError):
        OctreeGrid.make_dense(2, 2, 1, interpolation_type="closest")
    cat = OctreeGrid.make_dense(2, 2, 2)
    assert cat.multiscale_type == "cat"


def test_sparse_constructors_and_wisp_aliases():
    cells = torch.from_numpy(shell_cells(5))
    g = OctreeGrid.from_quantized_points(cells, feature_dim=2, base_lod=3, num_lods=3)
    assert g.blas.max_level == 5 and g.features[2].shape[0] == g.points_dual[5].shape[0] + 1
    pts = (cells.float() + 0.5) / 16 - 1
    g2 = CodebookOctreeGrid.from_pointcloud(pts, feature_dim=2, base_lod=3, num_lods=3, codebook_bitwidth=3)
    assert torch.equal(g2.blas.points, g.blas.points)
    import sys

    from shacira_amd import wisp as sw
    saved = {k: v for k, v in sys.modules.items() if k == "wisp" or k.startswith("wisp.")}
    try:
        sw.install_as_wisp(force=True)
        import wisp.models.grids as wg
        import wisp.ops.octree as wo
        from wisp.models.grids.codebook_grid import CodebookOctreeGrid as C2
        from wisp.models.grids.octree_grid import OctreeGrid as O2
        assert wg.OctreeGrid is OctreeGrid is O2 and wg.CodebookOctreeGrid is CodebookOctreeGrid is C2
        assert wo.octree_interpolate is octree_ops.octree_interpolate
    finally:
        for k in [k for k in sys.modules if k == "wisp" or k.startswith("wisp.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_replacing_the_occupancy_rebuilds_the_index_and_keeps_surviving_rows():
    torch.manual_seed(1)
    cells = torch.from_numpy(shell_cells(5))
    g = OctreeGrid.from_quantized_points(cells, feature_dim=3, base_lod=4, num_lods=2, feature_std=1.0)
    before = {l: (g.points_dual[l].clone(), g.features[i].detach().clone()) for i, l in enumerate(g.active_lods)}
    g.blas = OctreeAS.from_quantized_points(cells[::2], 5)
    g.refresh_index()
    for i, l in enumerate(g.active_lods):
        pd = g.points_dual[l]
        assert g.features[i].shape[0] == pd.shape[0] + 1 < before[l][1].shape[0]
        old = {tuple(p.tolist()): r for r, p in enumerate(before[l][0])}
        for r in range(0, pd.shape[0], 37):
            assert torch.equal(g.features[i][r], before[l][1][old[tuple(pd[r].tolist())]])


# ---- the codebook grid -----------------------------------------------------------------------------------------------------
def _reference_codebook_lookup(grid, coords, lod_idx, training):
    """codebook_grid.py:285-293 restated per (sample, corner), then 'trilinear_old': keys from the logits of the eight corner
    rows of every sample, features = dictionary * keys, blend with the coefficients."""
    outs = []
    for i in range(lod_idx + 1):
        li = grid.index[grid.active_lods[i]]
        level = li.level
        inside, cell, t = oref.locate(coords.numpy(), level)
        rank = oref.cell_rank(li.level_points.numpy(), level, cell, inside)
        valid = torch.from_numpy(rank >= 0)
        idx = li.trinkets[torch.from_numpy(rank[rank >= 0])].long()                 # [n, 8]
        logits = grid.features[i][idx]                                            # [n, 8, D]
        if training:
            y_soft = F.softmax(logits, dim=-1)
            index = y_soft.max(-1, keepdim=True)[1]
            y_hard = torch.zeros_like(logits).scatter_(-1, index, 1.0)
            keys = y_hard - y_soft.detach() + y_soft
            corner = (grid.dictionary[i][None, None] * keys[..., None]).sum(-2)  # [n, 8, F]
        else:
            corner = grid.dictionary[i][torch.max(logits, dim=-1)[1]]
        coeffs = torch.from_numpy(oref.weights(t[rank >= 0])).to(corner.dtype)
        fs = torch.zeros(coords.shape[0], grid.feature_dim, dtype=corner.dtype)
        fs[valid] = (corner * coeffs[..., None]).sum(-2)
        outs.append(fs)
    return torch.stack(outs).sum(0) if grid.multiscale_type == "sum" else torch.cat(outs, -1)


@pytest.mark.parametrize("ms", ["sum", "cat"])
def test_codebook_decode_per_corner_equals_the_per_sample_reference(ms):
    torch.manual_seed(2)
    cells = torch.from_numpy(random_cells(5, 0.05, seed=3))
    g = CodebookOctreeGrid.from_quantized_points(cells, feature_dim=4, base_lod=3, num_lods=3, multiscale_type=ms,
                                                 feature_std=0.5, codebook_bitwidth=4)
    assert [n for n, _ in g.named_parameters()] == [f"{p}.{i}" for p in ("dictionary", "features") for i in range(3)]
    assert all(tuple(d.shape) == (16, 4) for d in g.dictionary)
    assert [tuple(f.shape) for f in g.features] == [(g.points_dual[l].shape[0] + 1, 16) for l in (3, 4, 5)]
    assert g.bitwidth == 4 and g.name() == "Codebook Grid" and g.public_properties()["Bitwidth"] == 4
    rng = np.random.default_rng(7)
    pick = cells.numpy()[rng.integers(0, cells.shape[0], 400)]
    coords = torch.from_numpy(np.concatenate([(pick + rng.uniform(0, 1, pick.shape)) / 16 - 1,
                                              rng.uniform(-1.1, 1.1, (200, 3))]).astype(np.float32))
    params = [*g.dictionary, *g.features]
    for training in (True, False):
        g.train(training)
        got = octree_ops.octree_torch(coords, g.active_lods, g._tables(3), g.index, ms == "sum")
        want = _reference_codebook_lookup(g, coords, 2, training)
        assert got.shape == want.shape and float(want.abs().max()) > 0.1
        assert float((got - want).abs().max()) <= 1e-6
        if training:
            go = torch.randn_like(want)
            ga = torch.autograd.grad(got, params, go)
            gb = torch.autograd.grad(want, params, go)
            for a, b in zip(ga, gb):
                assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_codebook_size_is_the_entropy_of_the_indices():
    torch.manual_seed(3)
    g = CodebookOctreeGrid.make_dense(feature_dim=3, base_lod=2, num_lods=2, feature_std=1.0, codebook_bitwidth=3)
    bits = sum(d.numel() * 32 for d in g.dictionary)
    for f in g.features:
        idx = f.detach().numpy().argmax(-1)
        counts = np.bincount(idx)
        counts = counts[counts > 0]
        p = counts / counts.sum()
        bits += float((-np.log2(p) * counts).sum())
    zero, got = g.size()
    assert zero == 0.0 and abs(got - bits) <= 1e-4 * bits
    with pytest.raises(NotImplementedError):
        g.size(use_torchac=True)
    with pytest.raises(NotImplementedError):
        g.bake()


# ---- the C entry points reject bad calls before any HIP call ---------------------------------------------------------------
def test_entry_points_validate():
    L = _lib.lib()
    lv = (ctypes.c_int32 * 2)(3, 5)
    rows = (ctypes.c_int64 * 2)(10, 10)
    one = (ctypes.c_void_p * 2)(256, 256)
    fwd = lambda n, nl, F, ms, lv=lv, tabs=one, rows=rows: L.shacira_octree_forward(   # noqa: E731
        n, nl, lv, F, 256, tabs, rows, one, one, ms, 256, None, 0, None)
    assert fwd(16, 0, 4, 1) == _lib.EINVAL and fwd(16, 12, 4, 1) == _lib.EINVAL
    assert fwd(16, 2, 0, 1) == _lib.EINVAL and fwd(16, 2, 33, 1) == _lib.EINVAL
    assert fwd(16, 2, 4, 2) == _lib.EINVAL and fwd(-1, 2, 4, 1) == _lib.EINVAL
    assert fwd(16, 2, 4, 1, lv=(ctypes.c_int32 * 2)(3, 11)) == _lib.EINVAL
    assert fwd(16, 2, 4, 1, tabs=(ctypes.c_void_p * 2)(256, None)) == _lib.EINVAL
    assert fwd(16, 2, 4, 1, rows=(ctypes.c_int64 * 2)(10, 33 ** 3 + 1)) == _lib.EINVAL
    assert fwd(0, 2, 4, 1) == 0
    bwd = lambda n, flags, ws=0: L.shacira_octree_backward(   # noqa: E731
        n, 2, lv, 4, 256, one, rows, one, one, 256, 1, flags, one, 256, None, ws, None)
    assert bwd(16, 0) == _lib.EINVAL and bwd(16, 4) == _lib.EINVAL
    assert bwd(16, _lib.OCTREE_GRAD_FEATURES) == _lib.EWORKSPACE
    assert L.shacira_octree_backward_workspace_bytes(16, 2, lv, 4, 1, _lib.OCTREE_GRAD_FEATURES) > 0
    assert L.shacira_octree_backward_workspace_bytes(16, 2, lv, 4, 1, _lib.OCTREE_GRAD_COORDS) == 0
    assert L.shacira_octree_forward_workspace_bytes(16, 2, lv, 4, 1) == 0
