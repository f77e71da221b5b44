"""fp64 numpy restatement of the backward of the hash-grid coordinate gradient (include/shacira_hip.h, comment above
shacira_hashgrid_coords_backward2): results (1), (2), (3) for v = dL/dgrad_coords. Test helper, not a test.

As in coord_grad_ref: the fractions are the forward's own fp32 values, the corner rows come from
``oracle.hashgrid_torch.corner_rows_and_weights``, everything after that is fp64.
"""
import numpy as np
import torch

from coord_grad_ref import fractions
from oracle.hashgrid_torch import corner_rows_and_weights


def coord_grad2(coords, table, first_idx, resolutions, bitwidth, grad_output, v):
    """-> dict with
      ``ggo`` [N, L*F], ``ggo_bound``        (1) and its bound A (sum of the absolute values of the expanded terms)
      ``rows`` [R] int64, ``vals`` [R, F]    (2): the table rows some sample touches (ascending) and their sums
      ``gc`` [N, d], ``gc_bound``            (3) and its bound A
    ``table`` [T, F], ``grad_output`` [N, L*F] of any float dtype (widened to fp64), ``v`` [N, d]."""
    coords = np.asarray(coords, dtype=np.float32)
    table = np.asarray(table).astype(np.float64)
    go = np.asarray(grad_output).astype(np.float64)
    v = np.asarray(v).astype(np.float64)
    N, dim = coords.shape
    T, F = table.shape
    L = len(resolutions)
    cs = 2 ** int(bitwidth)
    NC = 1 << dim
    bit = np.array([[(k >> (dim - 1 - a)) & 1 for a in range(dim)] for k in range(NC)])     # [NC, d]
    sigma = 2.0 * bit - 1.0
    ggo, ggo_bound = np.zeros((N, L * F)), np.zeros((N, L * F))
    gc, gc_bound = np.zeros((N, dim)), np.zeros((N, dim))
    all_rows, all_vals = [], []
    for l, res in enumerate(resolutions):
        rows, _ = corner_rows_and_weights(torch.from_numpy(coords), int(res), cs)
        rows = rows.numpy() + int(first_idx[l])
        ok = (rows >= 0) & (rows < T)
        vals = table[np.clip(rows, 0, max(T - 1, 0))] * ok[..., None] if T else np.zeros((N, NC, F))   # [N, NC, F]
        g = go[:, l * F:(l + 1) * F]                                                                # [N, F]
        frac, ifrac, slope = fractions(coords, res)
        f64, g64 = frac.astype(np.float64), ifrac.astype(np.float64)
        w = np.where(bit[None] == 1, f64[:, None, :], g64[:, None, :])                              # [N, NC, d]
        c = v * slope                                                                               # [N, d]

        def prod_except(skip):
            out = np.ones((N, NC))
            for ax in range(dim):
                if ax not in skip:
                    out = out * w[:, :, ax]
            return out

        dirw, dirw_abs = np.zeros((N, NC)), np.zeros((N, NC))
        for a in range(dim):
            wa = prod_except((a,))
            dirw += c[:, a, None] * sigma[None, :, a] * wa
            dirw_abs += np.abs(c[:, a, None]) * wa
        ggo[:, l * F:(l + 1) * F] = (dirw[:, :, None] * vals).sum(1)
        ggo_bound[:, l * F:(l + 1) * F] = (dirw_abs[:, :, None] * np.abs(vals)).sum(1)
        contrib = dirw[:, :, None] * g[:, None, :]                                                  # [N, NC, F]
        all_rows.append(rows[ok])
        all_vals.append(contrib[ok])
        gt = (vals * g[:, None, :]).sum(2)                                                          # [N, NC]
        gt_abs = (np.abs(vals) * np.abs(g[:, None, :])).sum(2)
        for b in range(dim):
            for a in range(dim):
                if a == b:
                    continue
                wab = prod_except((a, b))
                gc[:, b] += c[:, a] * slope[:, b] * (sigma[None, :, a] * sigma[None, :, b] * wab * gt).sum(1)
                gc_bound[:, b] += np.abs(c[:, a]) * slope[:, b] * (wab * gt_abs).sum(1)
    rows = np.concatenate(all_rows) if all_rows else np.zeros(0, dtype=np.int64)
    contrib = np.concatenate(all_vals) if all_vals else np.zeros((0, F))
    uniq, inv = np.unique(rows, return_inverse=True)
    sums = np.zeros((uniq.shape[0], F))
    np.add.at(sums, inv.reshape(-1), contrib)
    return {"ggo": ggo, "ggo_bound": ggo_bound, "rows": uniq.astype(np.int64), "vals": sums, "gc": gc, "gc_bound": gc_bound}


def dense_table_grad(result, table_rows):
    """(2) as a dense fp64 [T, F] array (small tables only)."""
    out = np.zeros((table_rows, result["vals"].shape[1]))
    out[result["rows"]] = result["vals"]
    return out
