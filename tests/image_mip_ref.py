"""Host restatements for the mip-level tests (shacira_image_mip / shacira_raygen_sums, include/shacira_hip.h). Nothing here was
tuned on a kernel's output.

OpenCV is not installed where the suite runs, so its definition is used by restatement, the way tests/ssim_ref.py restates
skimage: a power-of-two INTER_AREA resize of a size the factor divides is the mean of each 2^mip x 2^mip block.

Three things are restated:
  * ``block_sums``: the exact integer block sums, numpy int64 -- what the kernel must equal element for element;
  * ``colors_chain``: this project's colour chain from those sums in fp32 on the host, one torch operator at a time, dividing
    by a TENSOR 255 * 4^mip (a Python scalar divisor becomes a product with a reciprocal on some devices) -- what the ray kernel
    and ``composite_colors(mip=...)`` must equal bit for bit;
  * ``reference_chain``: the REFERENCE's chain (nerf_standard_dataset.py:215-221 and :415-428): every byte to fp32 / 255, the
    block's 4^mip quotients summed in fp32 (row by row, left to right) and multiplied by 1 / 4^mip, then the composite in fp32.

``chain_bounds`` carries tests/raygen_ref._V through both chains: per value a bound on |fp32 chain - exact real result|, U = 2^-24
per rounding. The reference's colour carries one division per term and 4^mip - 1 additions, ours one division; both then run
the composite's operators. Two fp32 results of the same real number differ by at most the sum of their bounds: that sum is the
tolerance between the two chains, not a picked constant."""
import numpy as np
import torch

from raygen_ref import _V

U = 2.0 ** -24


def block_sums(images, mip):
    """uint8 [..., H, W, C] -> int64 [..., H >> mip, W >> mip, C], exact."""
    images = np.asarray(images)
    assert images.dtype == np.uint8
    f = 1 << mip
    *lead, H, W, C = images.shape
    assert H % f == 0 and W % f == 0
    return images.reshape(*lead, H // f, f, W // f, f, C).astype(np.int64).sum(axis=(-4, -2))


def _composite(rgb, alpha, bg_black):
    if bg_black:
        rgb = rgb - (1 - alpha)
    else:
        rgb = rgb * alpha
        rgb = rgb + (1 - alpha)
    return rgb.clamp(0.0, 1.0)


def colors_chain(sums, mip, bg_black):
    """integer sums [n, 3 or 4] -> (rgb fp32 [n, 3], mask bool [n]): the fp32 chain on the host, one operator at a time."""
    s = torch.from_numpy(np.ascontiguousarray(np.asarray(sums, np.int64)))
    img = s.to(torch.float32) / torch.full((1,), 255.0 * 4 ** mip, dtype=torch.float32)
    rgb = img[:, :3].clone()
    if img.shape[1] == 3:
        return rgb, torch.ones(img.shape[0], dtype=torch.bool)
    alpha = img[:, 3:4]
    return _composite(rgb, alpha, bg_black), (alpha > 0.5)[:, 0]


def mask_exact(sums_alpha, mip):
    """The integer form of alpha > 0.5: 2 S > 255 * 4^mip."""
    return 2 * np.asarray(sums_alpha, np.int64) > 255 * 4 ** mip


def _blocks(images, mip):
    """uint8 [V, H, W, C] -> [f * f, V * h * w, C]: term k of every block, rows first."""
    f = 1 << mip
    V, H, W, C = images.shape
    b = images.reshape(V, H // f, f, W // f, f, C).transpose(2, 4, 0, 1, 3, 5)
    return b.reshape(f * f, -1, C)


def reference_chain(images, mip, bg_black):
    """uint8 [V, H, W, 4] -> (rgb fp32 [V h w, 3], mask bool [V h w]) by the reference's float chain."""
    terms = torch.from_numpy(np.ascontiguousarray(_blocks(np.asarray(images), mip))).to(torch.float32)
    terms = terms / torch.full((1,), 255.0, dtype=torch.float32)
    acc = terms[0].clone()
    for k in range(1, terms.shape[0]):
        acc = acc + terms[k]
    img = acc * (1.0 / 4 ** mip)                     # a power of two: exact
    alpha = img[:, 3:4]
    return _composite(img[:, :3].clone(), alpha, bg_black), (alpha > 0.5)[:, 0]


def _composite_v(c, a, bg_black):
    one = _V(np.ones_like(a.v))
    rest = one - a
    return c - rest if bg_black else c * a + rest     # the clamp rounds nothing and moves no two values apart


def chain_bounds(images, mip, bg_black):
    """uint8 [V, H, W, 4] -> dict of fp64 arrays over the V h w pixels of the level:
      rgb [n, 3]          the exact composite (before the clamp) of the exact block means
      ours, theirs [n, 3] bounds on |colors_chain - exact| and |reference_chain - exact|
      alpha [n]           the exact alpha mean;  alpha_theirs [n]: the bound on the reference's fp32 alpha"""
    terms = _blocks(np.asarray(images), mip).astype(np.float64)
    full = _V(np.full(terms.shape[1:], 255.0))
    acc = _V(terms[0]) / full
    for k in range(1, terms.shape[0]):
        acc = acc + _V(terms[k]) / full
    theirs = acc.exact_scale(1.0 / 4 ** mip)
    ours = _V(terms.sum(axis=0)) / _V(np.full(terms.shape[1:], 255.0 * 4 ** mip))

    def split(v):
        return [_V(v.v[:, c], v.e[:, c]) for c in range(4)]

    out = {}
    for name, v in (("ours", ours), ("theirs", theirs)):
        ch = split(v)
        comp = [_composite_v(ch[c], ch[3], bg_black) for c in range(3)]
        out[name] = np.stack([c.e for c in comp], 1)
        if name == "ours":
            # the exact composite of the exact means, in fp64 from the integers (ours.v is that mean to 1e-16)
            out["rgb"] = np.stack([c.v for c in comp], 1)
            out["alpha"] = ch[3].v
        else:
            out["alpha_theirs"] = ch[3].e
    return out


def resize_ref(img, mip, mode):
    """(value, scale, ops, ref_ops): the fp64 definition of an interpolation mode at a factor 2^mip (mode: 'area', 'nearest',
    'linear') and what bounds an evaluation's distance from the exact real result. A mean of N terms summed in any order takes
    N - 1 additions and one division, each rounding once at unit roundoff u: |result - exact| <= ((1 + u)^N - 1) mean(|terms|).
    The linear mode's two 0.5 / 0.5 passes round twice (the halvings are exact). ``ref_ops`` counts the roundings of this
    function's own fp64 mean, which matters when the code under test runs in fp64 as well."""
    x = np.asarray(img, np.float64)
    f = 1 << mip
    H, W = x.shape[:2]
    if mode == "nearest":
        return x[::f, ::f], None, 0, 0
    b = x.reshape(H // f, f, W // f, f, *x.shape[2:])
    if mode == "area":
        return b.mean(axis=(1, 3)), np.abs(b).mean(axis=(1, 3)), f * f, f * f
    m = f // 2
    c = b[:, m - 1:m + 1][:, :, :, m - 1:m + 1]
    return c.mean(axis=(1, 3)), np.abs(c).mean(axis=(1, 3)), 2, 4


def resize_tolerance(scale, ops, ref_ops, u):
    """The code's bound at its unit roundoff ``u`` plus the fp64 definition's own."""
    gamma = lambda n, unit: n * unit / (1.0 - n * unit)          # >= (1 + unit)^n - 1, and computable in fp64 at unit = 2^-53
    return (gamma(ops, u) + gamma(ref_ops, 2.0 ** -53)) * scale


def s_table(mip, seed=0):
    """The sums the colour tests use: the ends, the three values around the mask's threshold and 64 seeded random ones."""
    D = 255 * 4 ** mip
    rng = np.random.default_rng(seed + mip)
    return np.concatenate([[0, 1, D // 2 - 1, D // 2, D // 2 + 1, D - 1, D], rng.integers(0, D + 1, 64)]).astype(np.int64)


def s_pixels(mip, channels=4):
    """Every (S_colour, S_alpha) pair of the table as an [n * n, channels] array: red carries the pair's colour, green and blue
    other entries of the table."""
    S = s_table(mip)
    n = len(S)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    px = np.stack([S[i], S[(i + 7) % n], S[(i + 13) % n], S[j]], -1).reshape(n * n, 4)
    return px[:, :channels]
