"""fp64 numpy restatement of the triplane sampling (include/shacira_hip.h, shacira_triplane_forward): forward, plane
gradient and coordinate gradient of torch's grid_sample(bilinear, align_corners=True, padding_mode='reflection') on the
three planes of each LOD. ``index_dtype`` is the precision of the index math: float64 to compare with torch's own fp64 op,
float32 to restate what the fp32 kernels compute (their weights exactly, the sums in fp64)."""
import numpy as np

PLANE_AXES = ((1, 2), (0, 2), (0, 1))   # fmx (y, z), fmy (x, z), fmz (x, y): first component = width axis


def reflect_info(c, S, index_dtype=np.float32):
    """Where a coordinate goes in reflect_coordinates, per element of ``c`` on a plane side of S texels:
    (flips, negative, reflected). ``flips`` = floor(|x| / (S - 1)) of the unnormalised index x (its parity picks the
    branch; not finite where x is not), ``negative`` = x < 0 (the sign branch of the gradient twin), ``reflected`` = the
    index after reflection and before clipping (exactly 0 or S - 1: the clip's gradient is 0). A test proves with these
    that its inputs reach the branch it claims to reach."""
    dt = index_dtype
    c = np.asarray(c, dtype=dt)
    one, two = dt(1), dt(2)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((c + one) / two) * dt(S - 1)
        span = dt(2 * (S - 1)) / two
        a = np.abs(x)
        extra = np.fmod(a, span)
        flips = np.floor(a / span)
        odd = np.where(np.isfinite(flips), np.fmod(flips, 2) == 1, True)
        r = np.where(odd, span - extra, extra)
    return flips, x < 0, r


def _index(c, S, dt, with_grad):
    """source index (and d index / d coord) of GridSampler.cuh for an array of coordinates."""
    one, two = dt(1), dt(2)
    flips, neg, r = reflect_info(c, S, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        odd = np.where(np.isfinite(flips), np.fmod(flips, 2) == 1, True)
        if not with_grad:
            r = np.fmin(dt(S - 1), np.fmax(r, dt(0)))
            return np.where(np.isfinite(r), r, dt(-100)), None
        grefl = np.where(odd, -1.0, 1.0) * np.where(neg, -1.0, 1.0)
        gclip = np.where((r <= 0) | (r >= S - 1), 0.0, 1.0)
        r = np.where(r <= 0, dt(0), np.where(r >= S - 1, dt(S - 1), r))
        mult = (dt(S - 1) / two).astype(np.float64) * grefl * gclip
        return np.where(np.isfinite(r), r, dt(-100)), mult


def coord_mult(c, S, index_dtype=np.float32):
    """d(source index) / d(coordinate) per element of ``c``: 0 where the reflected index sits on a border."""
    return _index(c, S, index_dtype, True)[1]


def _corners(ix, iy, dt):
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    w = [(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)]
    xs = [x0, x1, x0, x1]
    ys = [y0, y0, y1, y1]
    return [a.astype(np.int64) for a in xs], [a.astype(np.int64) for a in ys], [np.asarray(a, dt).astype(np.float64)
                                                                             for a in w]


def _scatter_add(dst, y, x, vals):
    """dst [F, S, S] += vals [n, F] at texels (y, x), repeated texels included (fp64 sums per distinct texel)."""
    S = dst.shape[-1]
    texel, inv = np.unique(y * S + x, return_inverse=True)
    flat = dst.reshape(dst.shape[0], -1)
    for f in range(dst.shape[0]):
        flat[f, texel] += np.bincount(inv.reshape(-1), weights=vals[:, f], minlength=texel.size)


def forward(coords, planes, multiscale_sum, index_dtype=np.float64, absolute=False):
    """coords [N, 3]; planes: per LOD (fmx, fmy, fmz), each [F, S, S] -> [N, 3F] or [N, L * 3F] float64."""
    coords = np.asarray(coords)
    out = []
    for lod in planes:
        cols = []
        for p, (a, b) in enumerate(PLANE_AXES):
            pl = np.asarray(lod[p])
            S = pl.shape[-1]
            ix, _ = _index(coords[:, a], S, index_dtype, False)
            iy, _ = _index(coords[:, b], S, index_dtype, False)
            xs, ys, ws = _corners(ix, iy, index_dtype)
            v = np.zeros((coords.shape[0], pl.shape[0]))
            for x, y, w in zip(xs, ys, ws):
                ok = (x >= 0) & (x < S) & (y >= 0) & (y < S)
                t = pl[:, y[ok], x[ok]].T.astype(np.float64)
                v[ok] += (np.abs(t) if absolute else t) * w[ok, None]
            cols.append(v)
        out.append(np.concatenate(cols, axis=1))
    return np.sum(out, axis=0) if multiscale_sum else np.concatenate(out, axis=1)


def abs_forward(coords, planes, multiscale_sum, index_dtype=np.float64):
    """sum |w * v| per output (the scale of a forward's rounding error)."""
    return forward(coords, planes, multiscale_sum, index_dtype, absolute=True)


def backward(coords, planes, grad_output, multiscale_sum, index_dtype=np.float64):
    """(plane gradients in the planes' layout, coordinate gradient [N, 3], sum of |terms| of the coordinate gradient)."""
    coords = np.asarray(coords)
    g_all = np.asarray(grad_output, np.float64)
    N = coords.shape[0]
    gplanes, gc, gscale = [], np.zeros((N, 3)), np.zeros((N, 3))
    for l, lod in enumerate(planes):
        F = np.asarray(lod[0]).shape[0]
        g = g_all if multiscale_sum else g_all[:, l * 3 * F:(l + 1) * 3 * F]
        out = []
        for p, (a, b) in enumerate(PLANE_AXES):
            pl = np.asarray(lod[p])
            S = pl.shape[-1]
            gp = np.zeros(pl.shape)
            ix, mx = _index(coords[:, a], S, index_dtype, True)
            iy, my = _index(coords[:, b], S, index_dtype, True)
            xs, ys, ws = _corners(ix, iy, index_dtype)
            ixd, iyd = ix.astype(np.float64), iy.astype(np.float64)
            x0, y0 = xs[0].astype(np.float64), ys[0].astype(np.float64)
            # d w_k / d ix and d w_k / d iy for nw, ne, sw, se
            dwx = [-(y0 + 1 - iyd), (y0 + 1 - iyd), -(iyd - y0), (iyd - y0)]
            dwy = [-(x0 + 1 - ixd), -(ixd - x0), (x0 + 1 - ixd), (ixd - x0)]
            gpl = g[:, p * F:(p + 1) * F]
            gix, giy, six, siy = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
            for k, (x, y, w) in enumerate(zip(xs, ys, ws)):
                ok = (x >= 0) & (x < S) & (y >= 0) & (y < S)
                _scatter_add(gp, y[ok], x[ok], w[ok, None] * gpl[ok])
                vals = np.zeros((N, F))
                vals[ok] = pl[:, y[ok], x[ok]].T.astype(np.float64)
                t = (vals * gpl).sum(1)
                ta = (np.abs(vals * gpl)).sum(1)
                gix += t * dwx[k]
                giy += t * dwy[k]
                six += ta * np.abs(dwx[k])
                siy += ta * np.abs(dwy[k])
            gc[:, a] += mx * gix
            gc[:, b] += my * giy
            gscale[:, a] += np.abs(mx) * six
            gscale[:, b] += np.abs(my) * siy
            out.append(gp)
        gplanes.append(out)
    return gplanes, gc, gscale


def backward_scale(coords, sides, fdim, grad_output, multiscale_sum, index_dtype=np.float64):
    """The scale of the plane gradient's rounding error, next to ``backward``: per LOD and plane (count int64 [S, S],
    abs_sum float64 [F, S, S]). ``count`` = the in-bounds corner contributions a texel receives, zero-weight ones
    included; ``abs_sum`` A = sum |w_k * g| over them, with the weights of ``backward`` (``index_dtype=np.float32``: the
    kernels' weights exactly). ``sides``: texels per plane side, one per LOD."""
    coords = np.asarray(coords)
    g_all = np.abs(np.asarray(grad_output, np.float64))
    F = int(fdim)
    out = []
    for l, S in enumerate(sides):
        g = g_all if multiscale_sum else g_all[:, l * 3 * F:(l + 1) * 3 * F]
        per = []
        for p, (a, b) in enumerate(PLANE_AXES):
            ix, _ = _index(coords[:, a], S, index_dtype, True)
            iy, _ = _index(coords[:, b], S, index_dtype, True)
            xs, ys, ws = _corners(ix, iy, index_dtype)
            count = np.zeros((S, S), dtype=np.int64)
            asum = np.zeros((F, S, S))
            gpl = g[:, p * F:(p + 1) * F]
            for x, y, w in zip(xs, ys, ws):
                ok = (x >= 0) & (x < S) & (y >= 0) & (y < S)
                count += np.bincount(y[ok] * S + x[ok], minlength=S * S).reshape(S, S)
                _scatter_add(asum, y[ok], x[ok], np.abs(w[ok, None]) * gpl[ok])
            per.append((count, asum))
        out.append(per)
    return out
