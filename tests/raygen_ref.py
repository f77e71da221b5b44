"""fp64 restatement of shacira_raygen (include/shacira_hip.h) with an error bound carried through the kernel's fp32 operation
sequence, in the manner of tests/latent_mlp_ref.py. Nothing here was tuned on the kernel's output.

The kernel's inputs are fp32 numbers, so the fp64 evaluation of the same formula is exact to about 1e-16 relative. Every fp32
operator the kernel executes rounds once: fl(z) = z (1 + d), |d| <= U = 2^-24 (+, -, *, / and sqrt are correctly rounded; the
library is built without contraction). ``_V`` carries a value and a bound on |fp32 value - exact value| through the sequence:
      fl(a + b)   err = ea + eb + U (|a + b| + ea + eb)
      fl(a * b)   err = |a| eb + |b| ea + ea eb + U (|a b| + ...)
      fl(a / b)   err = (ea + |a / b| eb) / (|b| - eb) + U (|a / b| + ...)
      fl(sqrt a)  err = ea / (2 sqrt(a - ea)) + U (sqrt(a) + ...)
An operation the kernel performs exactly (x + 0.5 for integer x < 2^23, the product by 2, by -1, or by a lens constant that is
exactly 0 or -1) adds no rounding term. Directions are unit vectors, so the bound is absolute per component; for the shapes the
tests use it stays below CAP = 32 U, which the tests assert so that a loose derivation cannot hide an error.

Colours and masks are exact: the fp32 torch chain on the host, one rounding per operator, which the kernel must match bit for
bit."""
import numpy as np
import torch

U = 2.0 ** -24
CAP = 32 * U
K = 20                  # SHACIRA_RAYGEN_RECORD_FLOATS


class _V:
    """value (fp64 array) and an absolute bound on the fp32 computation's distance from it."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    def _round(self):
        self.e = self.e + U * (np.abs(self.v) + self.e)
        return self

    def __add__(self, o):
        return _V(self.v + o.v, self.e + o.e)._round()

    def __sub__(self, o):
        return _V(self.v - o.v, self.e + o.e)._round()

    def __mul__(self, o):
        return _V(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)._round()

    def __truediv__(self, o):
        q = self.v / o.v
        return _V(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))._round()

    def sqrt(self):
        return _V(np.sqrt(self.v), self.e / (2.0 * np.sqrt(self.v - self.e)))._round()

    def exact_scale(self, c):          # a product the hardware performs without rounding (c = 2, -1)
        return _V(self.v * c, self.e * abs(c))


def make_record(rot, pos, tanx, tany, x0=0.0, y0=0.0, fov_distance=None, aspect=1.0):
    """One fp32 record from fp64 camera quantities (rot: camera to world, row-major)."""
    rec = np.zeros(K, np.float64)
    rec[0:9] = np.asarray(rot, np.float64).reshape(9)
    rec[9:12] = pos
    rec[12:16] = tanx, tany, x0, y0
    if fov_distance is not None:
        rec[16], rec[17], rec[18] = 1.0, fov_distance * aspect, fov_distance
    return rec.astype(np.float32)


def colors_ref(pixels, bg_black):
    """uint8 [n, C] -> (rgb fp32 [n, 3], mask bool [n]): the fp32 torch chain, one operator at a time."""
    img = torch.from_numpy(np.ascontiguousarray(pixels)).to(torch.float32) / 255.0
    rgb = img[:, :3].clone()
    if img.shape[1] == 3:
        return rgb, torch.ones(img.shape[0], dtype=torch.bool)
    alpha = img[:, 3:4]
    if bg_black:
        rgb -= (1 - alpha)
    else:
        rgb *= alpha
        rgb += (1 - alpha)
    return rgb.clamp(0.0, 1.0), (alpha > 0.5)[:, 0]


def raygen_ref(records, width, height, view_idx=None, pixel_idx=None, jitter=None, images=None, bg_black=False, n=None):
    """records fp32 [V, K] numpy; view_idx / pixel_idx integer arrays [n] or None (whole-view form, first n rays); jitter fp32
    [n, 2] or None; images uint8 [V, H, W, C] or None. Returns a dict of numpy arrays:
      valid [n] bool, origins / dirs fp64 [n, 3] (NaN where invalid), origins_bound / dirs_bound [n, 3], origins_exact [n] bool
      (the origin is the record's position, bit for bit), rgb fp32 [n, 3] and mask bool [n] (with images)."""
    records = np.asarray(records)
    assert records.dtype == np.float32 and records.shape[1] == K
    V, hw = records.shape[0], width * height
    if view_idx is None:
        n = V * hw if n is None else n
        flat = np.arange(n, dtype=np.int64)
        view_idx, pixel_idx = flat // hw, flat % hw
    view_idx, pixel_idx = np.asarray(view_idx, np.int64), np.asarray(pixel_idx, np.int64)
    n = view_idx.shape[0]
    valid = (view_idx >= 0) & (view_idx < V) & (pixel_idx >= 0) & (pixel_idx < hw)
    vi, pi = np.where(valid, view_idx, 0), np.where(valid, pixel_idx, 0)
    rec = records[vi].astype(np.float64)
    R = [[_V(rec[:, 3 * i + j]) for j in range(3)] for i in range(3)]
    t = [_V(rec[:, 9 + i]) for i in range(3)]
    tanx, tany, x0, y0 = (_V(rec[:, 12 + i]) for i in range(4))
    ortho = rec[:, 16] != 0
    fda, fd = _V(rec[:, 17]), _V(rec[:, 18])
    x, y = _V((pi % width) + 0.5), _V((pi // width) + 0.5)                 # exact in fp32
    jit = np.zeros((n, 2)) if jitter is None else np.asarray(jitter, np.float64)
    px, py = x + _V(jit[:, 0]), y + _V(jit[:, 1])
    if jitter is None:                                                     # + 0 is exact
        px, py = x, y
    px_p, py_p = px - x0, py + y0                                          # pinhole: the principal point

    def pick(a, b):                                                        # per ray: the orthographic or the pinhole chain
        return _V(np.where(ortho, a.v, b.v), np.where(ortho, a.e, b.e))

    px, py = pick(px, px_p), pick(py, py_p)
    one = _V(np.ones(n))
    u = (px / _V(np.full(n, float(width)))).exact_scale(2.0) - one
    v = (py / _V(np.full(n, float(height)))).exact_scale(2.0) - one
    zero = _V(np.zeros(n))
    dx = pick(zero, u * tanx)
    dy = pick(zero, v.exact_scale(-1.0) * tany)
    ox, oy = u * fda, v.exact_scale(-1.0) * fd
    origins, obound, w = [], [], []
    for i in range(3):
        o = (R[i][0] * ox + R[i][1] * oy) + t[i]
        origins.append(np.where(ortho, o.v, t[i].v))
        obound.append(np.where(ortho, o.e, 0.0))
        w.append((R[i][0] * dx + R[i][1] * dy) + R[i][2].exact_scale(-1.0))
    norm = ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]).sqrt()
    d = [wi / norm for wi in w]
    nanrow = np.where(valid, 0.0, np.nan)[:, None]
    out = dict(valid=valid, origins=np.stack(origins, 1) + nanrow, origins_bound=np.stack(obound, 1),
               origins_exact=valid & ~ortho, dirs=np.stack([c.v for c in d], 1) + nanrow,
               dirs_bound=np.stack([c.e for c in d], 1))
    if images is not None:
        images = np.asarray(images)
        pix = images.reshape(V, hw, images.shape[-1])[vi, pi]
        rgb, mask = colors_ref(pix, bg_black)
        rgb, mask = rgb.numpy().copy(), mask.numpy().copy()
        rgb[~valid] = np.nan
        mask[~valid] = False
        out.update(rgb=rgb, mask=mask)
    return out


def check_against_ref(ref, origins, dirs, rgb=None, mask=None):
    """Every element of the fp32 outputs (numpy) against ``ref``; asserts, and returns the largest direction error in units of
    U."""
    valid = ref["valid"]
    assert origins.shape == ref["origins"].shape and dirs.shape == ref["dirs"].shape
    assert np.isnan(origins[~valid]).all() and np.isnan(dirs[~valid]).all()
    assert float(ref["dirs_bound"][valid].max(initial=0.0)) < CAP, ref["dirs_bound"][valid].max() / U
    exact = ref["origins_exact"]
    assert np.array_equal(origins[exact], ref["origins"][exact].astype(np.float32))          # the record's bits
    rest = valid & ~exact
    assert (np.abs(origins[rest].astype(np.float64) - ref["origins"][rest]) <= ref["origins_bound"][rest]).all()
    err = np.abs(dirs[valid].astype(np.float64) - ref["dirs"][valid])
    assert (err <= ref["dirs_bound"][valid]).all(), (err / U).max()
    if "rgb" in ref:
        assert rgb is not None and mask is not None
        assert np.array_equal(rgb[valid], ref["rgb"][valid]) and np.isnan(rgb[~valid]).all()
        assert np.array_equal(mask.astype(bool).reshape(-1), ref["mask"])
    else:
        assert rgb is None and mask is None
    return float((err / U).max(initial=0.0))
