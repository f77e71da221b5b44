"""fp64 oracle of the positional-encoding row kernels (include/shacira_hip.h, shacira_posenc_*), in numpy.

Inputs are fp32 arrays. The argument of every sin / cos is the fp32 product ``fl32(coords[j] * bands[k])`` -- what the kernel and
the torch composite both form -- and everything after it is fp64. Every derivative comes with its MAGNITUDE: the same sum with
each term replaced by its absolute value, the scale against which an fp32 evaluation's rounding error is bounded.

Row layout (P prefix columns, I = d with the input included, else 0):
    [0, P) prefix | [P, P+I) coords | P+I + k*d + j: sin | P+I + d*F + k*d + j: cos
"""
import numpy as np

U = 2.0 ** -24          # half an fp32 ulp at 1: the unit of the tests' bounds


def widths(d, F, include_input, P=0):
    I = d if include_input else 0
    return I, P + I + 2 * d * F


def args(coords, bands):
    """fl32(coords[:, j] * bands[k]) as fp64 [N, F*d], frequency-major (column k*d + j)."""
    coords = np.asarray(coords, np.float32)
    bands = np.asarray(bands, np.float32)
    with np.errstate(all="ignore"):
        prod = (coords[:, None, :] * bands[None, :, None]).astype(np.float32)
    return prod.reshape(coords.shape[0], bands.shape[0] * coords.shape[1]).astype(np.float64)


def forward(coords, bands, include_input=True, prefix=None):
    """The row as fp64 [N, P + E]. Prefix and coordinate columns are exact copies (compare their BITS in fp32)."""
    coords = np.asarray(coords, np.float32)
    a = args(coords, bands)
    with np.errstate(all="ignore"):
        parts = [np.sin(a), np.cos(a)]
    if include_input:
        parts.insert(0, coords.astype(np.float64))
    if prefix is not None:
        parts.insert(0, np.asarray(prefix, np.float32).astype(np.float64))
    return np.concatenate(parts, axis=1)


def _split(x, d, F, include_input, P):
    I, width = widths(d, F, include_input, P)
    x = np.asarray(x).astype(np.float64)
    assert x.shape[1] == width, (x.shape, width)
    return x[:, P:P + I], x[:, P + I:P + I + d * F], x[:, P + I + d * F:]


def backward(row, grad_out, bands, d, include_input=True, P=0):
    """(grad_coords, magnitude) fp64 [N, d] from a row (the oracle's, or a kernel's saved one) and grad_out [N, P + E]."""
    bands = np.asarray(bands, np.float32).astype(np.float64)
    F = bands.shape[0]
    _, s, c = _split(row, d, F, include_input, P)
    g_in, g_s, g_c = _split(grad_out, d, F, include_input, P)
    n = s.shape[0]
    b = np.repeat(bands, d)[None, :]
    with np.errstate(all="ignore"):
        pos, neg = b * c * g_s, b * s * g_c
        gc = (pos - neg).reshape(n, F, d).sum(1)
        mag = (np.abs(pos) + np.abs(neg)).reshape(n, F, d).sum(1)
        if include_input:
            gc, mag = gc + g_in, mag + np.abs(g_in)
    return gc, mag


def backward2(gg, row, grad_out, bands, d, include_input=True, P=0):
    """(grad_row, grad_grad_out) fp64 [N, P + E]: the gradients of (backward(row, grad_out) * gg).sum() with respect to the row
    and to grad_out. Every entry is one product: it is its own magnitude."""
    bands = np.asarray(bands, np.float32).astype(np.float64)
    F = bands.shape[0]
    I, width = widths(d, F, include_input, P)
    _, s, c = _split(row, d, F, include_input, P)
    _, g_s, g_c = _split(grad_out, d, F, include_input, P)
    gg = np.asarray(gg, np.float32).astype(np.float64)
    n = gg.shape[0]
    b = np.repeat(bands, d)[None, :]
    w = np.tile(gg, (1, F))                         # column k*d + j -> gg[:, j]
    grad_row = np.zeros((n, width))
    grad_go = np.zeros((n, width))
    e = P + I
    with np.errstate(all="ignore"):
        grad_row[:, e:e + d * F] = -b * g_c * w
        grad_row[:, e + d * F:] = b * g_s * w
        grad_go[:, e:e + d * F] = b * c * w
        grad_go[:, e + d * F:] = -b * s * w
    if include_input:
        grad_go[:, P:e] = gg
    return grad_row, grad_go


def chain(coords, bands, v, include_input=True, P=0):
    """f(x) = row(x) . v per sample, L = sum |df/dx|^2: (dL/dx, its magnitude) fp64 [N, d]. dL/dprefix is exactly zero (f is
    linear in the prefix and df/dx does not depend on it)."""
    bands64 = np.asarray(bands, np.float32).astype(np.float64)
    F = bands64.shape[0]
    coords = np.asarray(coords, np.float32)
    n, d = coords.shape
    a = args(coords, bands)
    v_in, v_s, v_c = _split(np.broadcast_to(np.asarray(v, np.float32), (n, widths(d, F, include_input, P)[1])), d, F,
                            include_input, P)
    b = np.repeat(bands64, d)[None, :]
    with np.errstate(all="ignore"):
        s, c = np.sin(a), np.cos(a)
        t1, t2 = b * c * v_s, b * s * v_c               # df/dx_j = v_in_j + sum_k (t1 - t2)
        fx = (t1 - t2).reshape(n, F, d).sum(1)
        fx_mag = (np.abs(t1) + np.abs(t2)).reshape(n, F, d).sum(1)
        if include_input:
            fx, fx_mag = fx + v_in, fx_mag + np.abs(v_in)
        u1, u2 = b * b * s * v_s, b * b * c * v_c       # d2f/dx_j2 = -sum_k (u1 + u2)
        fxx = -(u1 + u2).reshape(n, F, d).sum(1)
        fxx_mag = (np.abs(u1) + np.abs(u2)).reshape(n, F, d).sum(1)
    return 2.0 * fx * fxx, 2.0 * fx_mag * fxx_mag
