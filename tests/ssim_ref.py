"""SSIM as skimage.metrics.structural_similarity(a, b, data_range=R, gaussian_weights=True, sigma=1.5, channel_axis=2) defines
it, restated on numpy and scipy.ndimage.gaussian_filter in a chosen dtype. Imports nothing from the package: it is the reference
of tests/test_ssim_cpu.py and tests/test_gpu_ssim.py. skimage itself is not a dependency, so parity with it is by this
restatement, not by a recorded run."""
import numpy as np
from scipy.ndimage import gaussian_filter

SIGMA, TRUNCATE = 1.5, 3.5
RADIUS = int(TRUNCATE * SIGMA + 0.5)        # 5
WIN = 2 * RADIUS + 1                        # 11


def window():
    """The 11 normalised weights, from an impulse through the filter itself."""
    e = np.zeros(4 * RADIUS + 1, np.float64)
    e[2 * RADIUS] = 1.0
    return gaussian_filter(e, sigma=SIGMA, truncate=TRUNCATE, mode="reflect")[RADIUS:-RADIUS]


def ssim(a, b, dtype=np.float64, data_range=1.0, shift=False):
    """(value, map): a, b [H, W, C]; every step in `dtype`, the mean of the valid pixels in fp64, then the mean of the channels.
    map is [H, W, C] in `dtype` with 'reflect' borders. With `shift` the five fields are taken of a - sa and b - sb, sa and sb
    the channel's image means rounded to `dtype`: variance and covariance do not change under a shift, the means get it back.
    The same definition (to rounding in fp64), without the cancellation of uxx - ux * ux on an image far from zero."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("two [H, W, C] images of one shape")
    if a.shape[0] < WIN or a.shape[1] < WIN:
        raise ValueError("win_size exceeds image extent")
    G = lambda p: gaussian_filter(p, sigma=SIGMA, truncate=TRUNCATE, mode="reflect")
    cov = WIN * WIN / (WIN * WIN - 1.0)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    values, maps = [], []
    for ch in range(a.shape[2]):
        x, y = a[..., ch], b[..., ch]
        if shift:
            sa, sb = dtype(x.mean(dtype=np.float64)), dtype(y.mean(dtype=np.float64))
            x, y = x - sa, y - sb
        ux, uy = G(x), G(y)
        uxx, uyy, uxy = G(x * x), G(y * y), G(x * y)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        if shift:
            ux, uy = sa + ux, sb + uy
        a1, a2 = 2 * ux * uy + c1, 2 * vxy + c2
        b1, b2 = ux ** 2 + uy ** 2 + c1, vx + vy + c2
        S = (a1 * a2) / (b1 * b2)
        assert S.dtype == dtype
        values.append(S[RADIUS:-RADIUS, RADIUS:-RADIUS].mean(dtype=np.float64))
        maps.append(S)
    return float(np.mean(values)), np.stack(maps, axis=-1)
