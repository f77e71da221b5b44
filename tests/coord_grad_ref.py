"""fp64 numpy restatement of the coordinate gradient of the hash-grid operator (include/shacira_hip.h, comment above
shacira_hashgrid_coords_backward). Test helper, not a test.

The fractions are the forward's own fp32 values (the transform of ``oracle.hashgrid_torch.corner_rows_and_weights``,
mirrored here because that function returns products, not fractions); the corner rows come from that function itself.
Everything after that is fp64.
"""
import numpy as np
import torch

from oracle.hashgrid_torch import corner_rows_and_weights


def fractions(coords, res):
    """coords fp32 [N, d] -> (frac fp32, 1 - frac fp32, slope fp64) [N, d] of one level, exactly as the kernels make them."""
    coords = np.asarray(coords, dtype=np.float32)
    hi = np.float32(float(res) - 1.0 - 1e-5)
    u = (float(res) * (coords.astype(np.float64) * 0.5 + 0.5)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(u), hi, np.minimum(u, hi))       # CUDA fminf: NaN operand -> the other operand
        x = np.maximum(x, np.float32(0.0))
        slope = np.where((u >= 0) & (u <= hi), 0.5 * float(res), 0.0)   # both ends inclusive; NaN compares false
    frac = (x - np.floor(x)).astype(np.float32)
    ifrac = (1.0 - frac.astype(np.float64)).astype(np.float32)
    return frac, ifrac, slope


def coord_grad(coords, table, first_idx, resolutions, bitwidth, grad_output):
    """-> (grad [N, d] fp64, bound A [N, d] fp64).

    ``table`` [T, F] and ``grad_output`` [N, L*F] of any float dtype (widened to fp64). ``A`` sums the absolute values of
    the expanded terms s * g * W * t over both corners of every pair, the scale of the rounding error of an fp32
    evaluation of the same sum."""
    coords = np.asarray(coords, dtype=np.float32)
    table = np.asarray(table).astype(np.float64)
    go = np.asarray(grad_output).astype(np.float64)
    N, dim = coords.shape
    T, F = table.shape
    cs = 2 ** int(bitwidth)
    NC = 1 << dim
    grad = np.zeros((N, dim))
    bound = np.zeros((N, dim))
    for l, res in enumerate(resolutions):
        rows, _ = corner_rows_and_weights(torch.from_numpy(coords), int(res), cs)
        rows = rows.numpy() + int(first_idx[l])
        ok = (rows >= 0) & (rows < T)
        vals = table[np.clip(rows, 0, max(T - 1, 0))] * ok[..., None] if T else np.zeros((N, NC, F))   # [N, NC, F]
        g = go[:, l * F:(l + 1) * F]                                                                # [N, F]
        frac, ifrac, slope = fractions(coords, res)
        f64, g64 = frac.astype(np.float64), ifrac.astype(np.float64)
        for a in range(dim):
            bit = 1 << (dim - 1 - a)
            s = np.zeros(N)
            b = np.zeros(N)
            for k0 in range(NC):
                if k0 & bit:
                    continue
                w = np.ones(N)
                for c in range(dim):
                    if c != a:
                        w = w * (f64[:, c] if k0 & (1 << (dim - 1 - c)) else g64[:, c])
                d = vals[:, k0 | bit, :] - vals[:, k0, :]                                          # [N, F]
                s += w * (d * g).sum(1)
                b += np.abs(w) * ((np.abs(vals[:, k0 | bit, :]) + np.abs(vals[:, k0, :])) * np.abs(g)).sum(1)
            grad[:, a] += slope[:, a] * s
            bound[:, a] += np.abs(slope[:, a]) * b
    return grad, bound


def assert_close(got, ref, bound, rel=1e-5, what=""):
    """|got - ref| <= rel * A entry by entry (plus a denormal floor)."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    lim = rel * bound + 1e-30
    bad = ~(err <= lim)
    assert not bad.any(), (f"{what}: {int(bad.sum())} entries beyond {rel} * A; worst at "
                           f"{np.unravel_index(np.argmax(np.where(bad, err / lim, 0)), err.shape)}: "
                           f"got {got[bad][:4]}, ref {ref[bad][:4]}")
