"""fp64 numpy restatement of the four view-shading contracts of include/shacira_hip.h (shacira_shade_view, shacira_shadow_rays,
shacira_shadow_apply, shacira_sdf_slice_colors). Inputs are taken as float32 and every step runs in float64; the slice colours
are the exception: their contract IS float32, one operator at a time, so they run in np.float32. Philox and Box-Muller come from
tests/mesh_sample_ref.py."""
import numpy as np

import mesh_sample_ref as msr

F32 = np.float32
RB, NORMAL, MATCAP = 0, 1, 2
SHADOW_STREAM = 0x53484457
BLUR_RADIUS = 8


def _f64(x):
    return np.ascontiguousarray(x, dtype=F32).astype(np.float64)


def envmap(dirs, normal, mm=None):
    """(uv [n, 2], m [n]) in fp64: the matcap coordinates and the divisor m = 2 |r| that sets their conditioning."""
    d, nr = _f64(dirs).reshape(-1, 3), _f64(normal).reshape(-1, 3)
    v = d.copy()
    if mm is not None:
        v = d @ _f64(mm).reshape(3, 3).T
    v[:, 2] = -v[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = 2.0 * (nr * v).sum(-1, keepdims=True)
        r = v - p * nr
        r[:, 2] -= 1.0
        m = 2.0 * np.sqrt((r * r).sum(-1))
        uv = 1.0 - (r[:, :2] / m[:, None] + 0.5)
        uv = np.where(uv > 0, np.where(uv < 1, uv, 1.0), 0.0)        # clamp; NaN -> 0
    return uv, m


def sample_matcap(tex, uv):
    """fp64 [n, 3]: the bilinear sample of the uint8 [mh, mw, mc] texture at uv in [0, 1]^2, over 255."""
    tex = np.asarray(tex, dtype=np.uint8)
    mh, mw = tex.shape[:2]
    t = tex[..., :3].astype(np.float64)
    uv = np.asarray(uv, dtype=np.float64)
    x, y = uv[:, 0] * (mw - 1), uv[:, 1] * (mh - 1)
    x0 = np.minimum(np.floor(x).astype(np.int64), mw - 2)
    y0 = np.minimum(np.floor(y).astype(np.int64), mh - 2)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    c = ((1 - fx) * (1 - fy) * t[y0, x0] + fx * (1 - fy) * t[y0, x0 + 1] + (1 - fx) * fy * t[y0 + 1, x0]
         + fx * fy * t[y0 + 1, x0 + 1])
    return c / 255.0


def level8(rgb):
    """uint8: saturating truncation of rgb * 255 (NaN -> 0), from the float32 colours the kernel stored."""
    v = np.asarray(rgb, dtype=F32) * F32(255.0)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.where(v < 255, np.nan_to_num(np.clip(v, 0, 255)), 255), 0).astype(np.uint8)


def shade_view(mode, normal, dirs=None, hit=None, mm=None, tex=None, rgb=None, uv=None):
    """dict(rgb fp64 [n, 3], normal fp64 [n, 3], uv fp64 [n, 2] or None, m). ``uv`` given: the sampler runs at those coordinates
    (the kernel's own) instead of the oracle's."""
    nr = _f64(normal).reshape(-1, 3).copy()
    out_uv = m = None
    if mode == MATCAP:
        out_uv, m = envmap(dirs, normal, mm)
        c = sample_matcap(tex, out_uv if uv is None else uv) if tex is not None else None
    elif mode == NORMAL:
        c = (nr + 1.0) / 2.0
    else:
        c = _f64(rgb).reshape(-1, 3).copy()
    if hit is not None and c is not None:
        miss = ~np.asarray(hit).astype(bool).reshape(-1)
        nr[miss] = 1.0
        c[miss] = 1.0
    return dict(rgb=c, normal=nr, uv=out_uv, m=m)


def shadow_gaussians(n, seed):
    """fp64 [n, 3]: g of rays 0 .. n - 1."""
    idx = np.arange(n, dtype=np.uint64)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    w = np.stack(msr.philox4x32_10(idx & msr.MASK, idx >> np.uint64(32), SHADOW_STREAM, 0, k0, k1), axis=1).astype(np.uint32)
    return msr.gaussians64(np.concatenate([w, w], axis=1))      # gaussians64 reads words 4..7


def shadow_rays(origins, dirs, depth, xyz, normal, hit, light, min_y, seed):
    """The contract in fp64. Returns the updated depth / xyz / normal / hit, so, sd, the two flags and the two deciding
    quantities: plane_margin (how far plane_t is from the nearest of its three thresholds; inf where NaN decides) and
    light_dot."""
    o, d = _f64(origins), _f64(dirs)
    depth, xyz, nr = _f64(depth).reshape(-1).copy(), _f64(xyz).copy(), _f64(normal).copy()
    hit = np.asarray(hit).astype(bool).reshape(-1).copy()
    n = o.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = -d[:, 1]
        plane_t = (o[:, 1] - float(F32(min_y))) / rate
        ph = (plane_t > 0) & (plane_t < 500) & (plane_t < depth)
        margin = np.minimum(np.minimum(np.abs(plane_t), np.abs(plane_t - 500)), np.abs(plane_t - depth))
        margin = np.where(np.isnan(margin), np.inf, margin)
    hit[ph] = False
    depth[ph] = plane_t[ph]
    xyz[ph] = o[ph] + d[ph] * plane_t[ph, None]
    nr[ph] = (0.0, 1.0, 0.0)
    so = xyz + float(F32(0.01)) * nr
    g = shadow_gaussians(n, seed)
    x = (_f64(light).reshape(1, 3) + float(F32(0.01)) * g) - so
    with np.errstate(invalid="ignore"):
        sd = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), float(F32(1e-12)))
        dot = (sd * nr).sum(-1)
    return dict(depth=depth, xyz=xyz, normal=nr, hit=hit, so=so, sd=sd, light_hit=dot > 0, plane_hit=ph,
                plane_margin=margin, plane_t=plane_t, light_dot=dot, g=g)


def blur_taps():
    """fp64 [17]: scipy.ndimage.gaussian_filter's taps for sigma = 2 (radius 8), normalised."""
    k = np.arange(-BLUR_RADIUS, BLUR_RADIUS + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / 4.0)
    return w / w.sum()


def reflect_index(i, n):
    """scipy's mode='reflect' (d c b a | a b c d | d c b a), periodic with period 2 n."""
    j = np.mod(i, 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def gaussian_blur(image):
    """fp64 [H, W]: the 17-tap separable blur, axis 0 then axis 1, reflect borders, for any H, W >= 1."""
    a = np.asarray(image, dtype=np.float64)
    w = blur_taps()
    for axis in (0, 1):
        n = a.shape[axis]
        out = np.zeros_like(a)
        for t, k in enumerate(range(-BLUR_RADIUS, BLUR_RADIUS + 1)):
            out += w[t] * np.take(a, reflect_index(np.arange(n) + k, n), axis=axis)
        a = out
    return a


def shadow_apply(H, W, occluded, light_hit, rgb):
    """dict(shadow bool [H W], map fp64 [H, W] (blurred), rgb fp64 [H W, C])."""
    s = np.asarray(occluded).astype(bool).reshape(-1) & np.asarray(light_hit).astype(bool).reshape(-1)
    m = gaussian_blur(np.clip((1.0 - s.astype(np.float64)) + float(F32(0.7)), 0.0, 1.0).reshape(H, W))
    c = _f64(rgb).reshape(H * W, -1).copy()
    c[:, :3] *= m.reshape(-1, 1)
    return dict(shadow=s, map=m, rgb=c)


SLICE_BASE, SLICE_INSIDE, SLICE_LINE, SLICE_ZERO, SLICE_NAN = 0, 1, 2, 3, 4


def sdf_slice_colors(d):
    """(vis float32 [n, 3], class int [n]) in np.float32, one operator at a time. Class SLICE_NAN: a NaN row."""
    d = np.ascontiguousarray(d, dtype=F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        dd = np.clip((d + F32(1.0)) / F32(2.0), F32(0.0), F32(1.0))
        blue = np.clip((dd - F32(0.5)) * F32(2.0), F32(0.0), F32(1.0))
        yellow = F32(1.0) - blue
        vis = np.stack([(F32(0.0) + yellow * F32(0.4)) + F32(0.2), (F32(0.0) + yellow * F32(0.3)) + F32(0.2),
                        (blue + yellow * F32(0.0)) + F32(0.2)], axis=1).astype(F32)
        cls = np.full(d.shape, SLICE_BASE)
        cls[np.isnan(dd)] = SLICE_NAN
        inside = dd - F32(0.5) < 0
        vis[inside] = (F32(1.0), F32(0.38), F32(0.0))
        cls[inside] = SLICE_INSIDE
        for i in range(50):
            line = np.abs(dd - F32(0.02 * i)) < F32(0.0015)
            vis[line] = F32(0.8)
            cls[line] = SLICE_LINE
        zero = np.abs(dd - F32(0.5)) < F32(0.004)
        vis[zero] = F32(0.0)
        cls[zero] = SLICE_ZERO
    return vis, cls
