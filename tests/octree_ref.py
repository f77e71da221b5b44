"""The yardstick of the octree lookup: a numpy restatement in fp64 of the contract above ``shacira_octree_forward`` in
include/shacira_hip.h, written from that text and not from the product code.

Per level l with G = 2^l:  p = (x + 1) * G / 2,  cell = floor(p),  t = p - cell.  The level contributes zeros where a
component of cell is outside [0, G), a coordinate is not finite, or the cell is unoccupied; otherwise
sum_k w_k * table[trinkets[rank(cell), k]] with w_k the product of t or 1 - t per axis, corner k = (k >> 2 & 1, k >> 1 & 1,
k & 1). 'cat' concatenates the levels in the order given, 'sum' adds them.

p, cell and t are computed in ``index_dtype`` (fp32 by default, exactly as the contract states them: only the addition
rounds), so a sample near a cell face lands in the same cell as in the kernel and no sample needs excluding from a
comparison. Everything after that is fp64. ``index_dtype=np.float64`` makes the restatement differentiable by finite
differences.

Inputs are the inspectable tensors of the index as numpy arrays: ``level_points[l]`` int [cells, 3] (any order),
``trinkets[l]`` int [cells, 8] (row c belongs to ``level_points[l][c]``) and ``tables[l]`` [C + 1, F].
"""
import numpy as np

CORNERS = np.array([[k >> 2 & 1, k >> 1 & 1, k & 1] for k in range(8)], dtype=np.int64)


def _all_cells(level):
    G = 1 << level
    return np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 3)


def shell_cells(level, radius=0.7):
    """A test occupancy, a thin spherical shell: the cells of ``level`` whose centre lies within one cell of the sphere."""
    cells = _all_cells(level)
    centre = (cells + 0.5) * (2.0 / (1 << level)) - 1.0
    return cells[np.abs(np.linalg.norm(centre, axis=-1) - radius) < 2.0 / (1 << level)]


def random_cells(level, fraction=0.03, seed=0):
    """A test occupancy: ``fraction`` of the cells of ``level``, drawn without replacement."""
    G = 1 << level
    keys = np.random.default_rng(seed).choice(G ** 3, int(fraction * G ** 3), replace=False)
    return np.stack([keys // (G * G), (keys // G) % G, keys % G], -1)


def locate(coords, level, index_dtype=np.float32):
    """-> (inside bool [N], cell int64 [N, 3] (0 where not inside), t fp64 [N, 3] (0 where not inside))."""
    G = 1 << level
    x = np.asarray(coords).astype(index_dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x + index_dtype(1)) * index_dtype(G / 2)
        fl = np.floor(p)
        inside = np.all(np.isfinite(x), axis=-1) & np.all((fl >= 0) & (fl < G), axis=-1)
        cell = np.where(inside[:, None], fl, 0).astype(np.int64)
        t = np.where(inside[:, None], p - fl, 0).astype(np.float64)
    return inside, cell, t


class SortedCells:
    """``level_points`` of one level with its keys sorted once: pass it wherever a ``level_points[l]`` goes when the same
    index serves many calls (``cell_rank`` sorts a plain array on every call)."""

    def __init__(self, level_points, level):
        G = 1 << level
        pts = np.asarray(level_points).astype(np.int64)
        keys = (pts[:, 0] * G + pts[:, 1]) * G + pts[:, 2]
        self.level = level
        self.order = np.argsort(keys, kind="stable")
        self.keys = keys[self.order]


def cell_rank(level_points, level, cell, inside):
    """Row of ``level_points`` (an array or a ``SortedCells``) that equals each cell, -1 where there is none (unoccupied) or
    the sample is not inside."""
    G = 1 << level
    rank = np.full(cell.shape[0], -1, dtype=np.int64)
    sc = level_points if isinstance(level_points, SortedCells) else SortedCells(level_points, level)
    assert sc.level == level
    if sc.keys.shape[0] == 0:
        return rank
    ck = (cell[:, 0] * G + cell[:, 1]) * G + cell[:, 2]
    pos = np.clip(np.searchsorted(sc.keys, ck), 0, sc.keys.shape[0] - 1)
    found = inside & (sc.keys[pos] == ck)
    rank[found] = sc.order[pos[found]]
    return rank


def weights(t, weight_dtype=np.float64):
    """fp64 [N, 8]: w_k. ``weight_dtype=np.float32`` rounds 1 - t and the product (x, then y, then z) to fp32: the weights
    of a kernel that evaluates the contract's product in fp32, exactly (``t`` is an fp32 value already)."""
    dt = weight_dtype
    t = np.asarray(t).astype(dt)
    w = np.ones((t.shape[0], 8), dtype=dt)
    for k in range(8):
        for a in range(3):
            w[:, k] *= t[:, a] if CORNERS[k, a] else dt(1) - t[:, a]
    return w.astype(np.float64)


def _dweights(t):
    """fp64 [N, 8, 3]: d w_k / d t_a."""
    d = np.ones((t.shape[0], 8, 3), dtype=np.float64)
    for k in range(8):
        for a in range(3):
            for b in range(3):
                if a == b:
                    d[:, k, a] *= 1.0 if CORNERS[k, b] else -1.0
                else:
                    d[:, k, a] *= t[:, b] if CORNERS[k, b] else 1.0 - t[:, b]
    return d


def _per_level(coords, levels, level_points, trinkets, tables, index_dtype, absolute):
    out = []
    for l, level in enumerate(levels):
        table = np.asarray(tables[l], dtype=np.float64)
        inside, cell, t = locate(coords, level, index_dtype)
        rank = cell_rank(level_points[l], level, cell, inside)
        hit = rank >= 0
        val = np.zeros((coords.shape[0], table.shape[1]), dtype=np.float64)
        if hit.any():
            rows = np.asarray(trinkets[l]).astype(np.int64)[rank[hit]]          # [n, 8]
            w = weights(t[hit])
            v = table[rows]                                                      # [n, 8, F]
            val[hit] = (np.abs(w)[..., None] * np.abs(v)).sum(1) if absolute else (w[..., None] * v).sum(1)
        out.append(val)
    return out


def forward(coords, levels, level_points, trinkets, tables, multiscale_sum, index_dtype=np.float32):
    per = _per_level(coords, levels, level_points, trinkets, tables, index_dtype, False)
    return sum(per) if multiscale_sum else np.concatenate(per, axis=-1)


def abs_forward(coords, levels, level_points, trinkets, tables, multiscale_sum, index_dtype=np.float32):
    """sum |w| |v| in the output's layout: the scale of the forward's rounding error."""
    per = _per_level(coords, levels, level_points, trinkets, tables, index_dtype, True)
    return sum(per) if multiscale_sum else np.concatenate(per, axis=-1)


def hit_any(coords, levels, level_points, index_dtype=np.float32):
    """bool [N]: the sample lies in an occupied cell of at least one level."""
    any_hit = np.zeros(coords.shape[0], dtype=bool)
    for l, level in enumerate(levels):
        inside, cell, _ = locate(coords, level, index_dtype)
        any_hit |= cell_rank(level_points[l], level, cell, inside) >= 0
    return any_hit


def backward(coords, levels, level_points, trinkets, tables, grad_out, multiscale_sum, index_dtype=np.float32,
             weight_dtype=np.float64):
    """-> (table gradients, one fp64 [C + 1, F] per level; coordinate gradient fp64 [N, 3]; its absolute-sum scale [N, 3]).
    ``weight_dtype``: the precision of the table gradient's weights (``weights``); the sums are fp64 either way."""
    N = coords.shape[0]
    grad_out = np.asarray(grad_out, dtype=np.float64)
    grad_tables = []
    grad_coords = np.zeros((N, 3), dtype=np.float64)
    gscale = np.zeros((N, 3), dtype=np.float64)
    for l, level in enumerate(levels):
        table = np.asarray(tables[l], dtype=np.float64)
        F = table.shape[1]
        g = grad_out if multiscale_sum else grad_out[:, l * F:(l + 1) * F]
        G = 1 << level
        inside, cell, t = locate(coords, level, index_dtype)
        rank = cell_rank(level_points[l], level, cell, inside)
        hit = rank >= 0
        gt = np.zeros_like(table)
        if hit.any():
            rows = np.asarray(trinkets[l]).astype(np.int64)[rank[hit]]
            w = weights(t[hit], weight_dtype)
            contrib = w[..., None] * g[hit][:, None, :]                           # [n, 8, F]
            for j in range(F):
                gt[:, j] = np.bincount(rows.reshape(-1), weights=contrib[..., j].reshape(-1), minlength=gt.shape[0])
            dots = (table[rows] * g[hit][:, None, :]).sum(-1)                    # [n, 8]
            adots = (np.abs(table[rows]) * np.abs(g[hit])[:, None, :]).sum(-1)
            dw = _dweights(t[hit])                                               # [n, 8, 3]
            grad_coords[hit] += (G / 2) * (dw * dots[..., None]).sum(1)
            gscale[hit] += (G / 2) * (np.abs(dw) * adots[..., None]).sum(1)
        grad_tables.append(gt)
    return grad_tables, grad_coords, gscale


def backward_scale(coords, levels, level_points, trinkets, table_rows, grad_out, multiscale_sum, index_dtype=np.float32,
                   weight_dtype=np.float32):
    """The scale of the table gradient's rounding error, next to ``backward``: per level (count int64 [C + 1], abs_sum
    float64 [C + 1, F]). ``count`` = the corner contributions a row receives (eight per sample in an occupied cell,
    zero-weight ones included); ``abs_sum`` A = sum |w_k * g| over them, with the weights of ``weights(t, weight_dtype)``.
    ``table_rows[l]`` = C_l + 1."""
    grad_out = np.abs(np.asarray(grad_out, dtype=np.float64))
    out = []
    for l, level in enumerate(levels):
        rows_total = int(table_rows[l])
        F = grad_out.shape[1] if multiscale_sum else grad_out.shape[1] // len(levels)
        g = grad_out if multiscale_sum else grad_out[:, l * F:(l + 1) * F]
        inside, cell, t = locate(coords, level, index_dtype)
        rank = cell_rank(level_points[l], level, cell, inside)
        hit = rank >= 0
        count = np.zeros(rows_total, dtype=np.int64)
        asum = np.zeros((rows_total, F))
        if hit.any():
            rows = np.asarray(trinkets[l]).astype(np.int64)[rank[hit]]
            contrib = np.abs(weights(t[hit], weight_dtype))[..., None] * g[hit][:, None, :]
            count = np.bincount(rows.reshape(-1), minlength=rows_total)
            for j in range(F):
                asum[:, j] = np.bincount(rows.reshape(-1), weights=contrib[..., j].reshape(-1), minlength=rows_total)
        out.append((count, asum))
    return out
