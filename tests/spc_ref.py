"""fp64 / int64 restatement of the structured-point-cloud contracts of include/shacira_hip.h ("Structured point clouds"),
written from the header, not from the kernels of shacira_amd/csrc/spc.hip.

Points. The point of a valid pixel is p_i = fl(o_i + fl(d_i * depth)): two fp32 roundings on top of shacira_raygen's origin and
direction. tests/raygen_ref.py carries a bound on |fp32 - exact| through the ray's operation sequence; ``points_ref`` continues
that chain with the same ``_V`` arithmetic: the product with the (exact) depth multiplies the direction's bound by |depth| and
rounds once, the sum with the origin adds the origin's bound and rounds once.

Cells, slots, colours. Integers: the cell of an fp32 point is the fp32 expression floorf((x + 1) * 0.5f * G) evaluated with
numpy float32 operators (one rounding each, as the kernel's); keys, words, ranks, slots, colour sums and the rounded means
(2 sum + n) // (2 n) are int64 and exact.

The walk and the first hit. ``walk_ref`` is the slab test and the Amanatides-Woo walk of shacira_raytrace_dense in numpy float32
scalars: every occupied cell whose stay has positive length, in depth order; ``first_hit_ref``, "the first nugget of a flat fp32
DDA", is its first nugget per finite ray. The one fused operation of the walk's set-up, fmaf(d, tin, o), is evaluated in fp64 and
rounded to fp32 (the product is exact in fp64; the sum rounds twice, which can differ from the fused result only when the fp64
sum lands within 2^-29 relative of an fp32 tie) -- it only chooses the start cell. The authority is what the device computed:
tests/golden/grid_walk.npz, which tests/test_spc_cpu.py holds this restatement to, bit for bit."""
import numpy as np
import torch

import raygen_ref as R

F32 = np.float32


def points_ref(records, width, height, depth):
    """records fp32 [V, K], depth fp32 [V, H, W] (numpy). -> dict: valid [n] bool (depth finite), points fp64 [n, 3] and bound
    [n, 3] (rows of invalid pixels are NaN / 0), in (view, pixel) order, n = V H W."""
    depth = np.asarray(depth, F32).reshape(-1)
    ray = R.raygen_ref(records, width, height)
    valid = np.isfinite(depth)
    dep = R._V(np.where(valid, depth, 0.0).astype(np.float64))
    pts, bound = [], []
    for i in range(3):
        o = R._V(ray["origins"][:, i], ray["origins_bound"][:, i])
        d = R._V(ray["dirs"][:, i], ray["dirs_bound"][:, i])
        p = o + d * dep
        pts.append(np.where(valid, p.v, np.nan))
        bound.append(np.where(valid, p.e, 0.0))
    return dict(valid=valid, points=np.stack(pts, 1), bound=np.stack(bound, 1), dirs_bound=ray["dirs_bound"])


def colour_bytes_ref(pixels, bg_black, mip=0):
    """integer pixels [n, 3 or 4] (bytes, or the block sums of ``mip``) -> uint8 [n, 3]: the fp32 composite, one operator at a
    time, then q = rint(255 c)."""
    full = torch.full((1,), 255.0 * 4 ** mip, dtype=torch.float32)
    img = torch.from_numpy(np.ascontiguousarray(pixels).astype(np.int64)).to(torch.float32) / full
    rgb = img[:, :3].clone()
    if img.shape[1] == 4:
        alpha = img[:, 3:4]
        if bg_black:
            rgb = rgb - (1 - alpha)
        else:
            rgb = rgb * alpha
            rgb = rgb + (1 - alpha)
        rgb = rgb.clamp(0.0, 1.0)
    return torch.round(255.0 * rgb).to(torch.uint8).numpy()


def cells_ref(points, level):
    """fp32 points [N, 3] -> (keys int64 [M], keep bool [N]): a point with a cell that is not finite is dropped, every other
    cell is clamped to 0 .. G - 1; key = (x G + y) G + z."""
    G = 1 << level
    p = np.asarray(points, F32)
    with np.errstate(all="ignore"):
        cell = np.floor(((p + F32(1.0)) * F32(0.5)) * F32(G))
    keep = np.isfinite(cell).all(axis=1)
    c = np.clip(cell[keep], 0, G - 1).astype(np.int64)
    return (c[:, 0] * G + c[:, 1]) * G + c[:, 2], keep


def num_words(level):
    return max(1, (1 << (3 * level)) // 32)


def words_ref(keys, level):
    """keys -> the packed occupancy, uint32 [num_words]."""
    words = np.zeros(num_words(level), np.uint32)
    for k in np.unique(keys):
        words[k >> 5] |= np.uint32(1) << np.uint32(k & 31)
    return words


def occupancy_bits(occupancy):
    """bool [G, G, G] -> uint8 bytes: cell key is bit key & 7 of byte key >> 3 -- the bytes of the packed words, unpadded."""
    return np.packbits(np.asarray(occupancy, bool).reshape(-1), bitorder="little")


def occupancy_from_bits(bits, level):
    G = 1 << level
    return np.unpackbits(np.asarray(bits, np.uint8), count=G ** 3, bitorder="little").astype(bool).reshape(G, G, G)


def popcount(words):
    w = np.asarray(words, np.uint32).astype(np.int64)
    return sum((w >> b) & 1 for b in range(32))


def rank_ref(words):
    """(rank int32 [num_words], cells): the exclusive prefix of the popcounts and their total."""
    pop = popcount(words)
    ends = np.cumsum(pop)
    return (ends - pop).astype(np.int32), int(ends[-1])


def slots_ref(keys, words, rank):
    keys = np.asarray(keys, np.int64)
    w = np.asarray(words, np.uint32).astype(np.int64)[keys >> 5]
    return np.asarray(rank, np.int64)[keys >> 5] + popcount(w & ((1 << (keys & 31)) - 1))


def colors_ref(keys, colours, words, rank, cells):
    """keys [M], colour bytes [M, 3] -> (sums int64 [cells, 4], colors uint8 [cells, 4])."""
    sums = np.zeros((cells, 4), np.int64)
    slots = slots_ref(keys, words, rank)
    np.add.at(sums, slots, np.concatenate([np.asarray(colours, np.int64), np.ones((len(keys), 1), np.int64)], axis=1))
    n = sums[:, 3:4]
    colors = np.full((cells, 4), 255, np.int64)
    colors[:, :3] = np.where(n > 0, (2 * sums[:, :3] + n) // np.maximum(2 * n, 1), 0)
    return sums, colors.astype(np.uint8)


def morton(x, y, z, level):
    m = 0
    for b in range(level):
        m |= (((x >> b) & 1) << (3 * b + 2)) | (((y >> b) & 1) << (3 * b + 1)) | (((z >> b) & 1) << (3 * b))
    return m


def _fma32(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def walk_ref(origins, dirs, occupancy, level, finite_gate, first=False):
    """origins, dirs fp32 [N, 3]; occupancy bool [G, G, G] indexed [x][y][z]. -> every nugget, in ray and then depth order:
    (ridx int32 [K], cells int32 [K, 3], depth fp32 [K, 2] = t_enter, t_exit). ``finite_gate``: a ray with a component that is
    not finite has no nugget (shacira_spc_first_hit's contract; shacira_raytrace_dense has no such gate). ``first``: a ray's
    walk stops after its first nugget."""
    G = 1 << level
    origins, dirs = np.asarray(origins, F32), np.asarray(dirs, F32)
    ridx, cells, depth = [], [], []
    inf, one, zero = F32(np.inf), F32(1.0), F32(0.0)
    with np.errstate(all="ignore"):
        for r in range(origins.shape[0]):
            o, d = origins[r], dirs[r]
            if finite_gate and not (np.isfinite(o).all() and np.isfinite(d).all()):
                continue
            tn, tf, miss = -inf, inf, False
            for a in range(3):
                if d[a] == zero:
                    miss = miss or o[a] < -one or o[a] > one
                else:
                    inv = one / d[a]
                    t0, t1 = (-one - o[a]) * inv, (one - o[a]) * inv
                    tn, tf = max(tn, min(t0, t1)), min(tf, max(t0, t1))
            if miss or not tf > max(tn, zero):
                continue
            t = max(tn, zero)
            cell = F32(2.0) / F32(G)
            c, step, tmax, tdelta = [0] * 3, [0] * 3, [inf] * 3, [inf] * 3
            for a in range(3):
                p = _fma32(d[a], t, o[a])
                q = int(np.floor(((p + one) * F32(0.5)) * F32(G)))
                q = min(max(q, 0), G - 1)
                c[a] = q
                if d[a] > zero:
                    step[a], tdelta[a] = 1, cell / d[a]
                    tmax[a] = ((-one + F32(q + 1) * cell) - o[a]) / d[a]
                elif d[a] < zero:
                    step[a], tdelta[a] = -1, -cell / d[a]
                    tmax[a] = ((-one + F32(q) * cell) - o[a]) / d[a]
            for _ in range(3 * G + 3):
                a = (0 if tmax[0] <= tmax[2] else 2) if tmax[0] <= tmax[1] else (1 if tmax[1] <= tmax[2] else 2)
                texit = min(tmax[a], tf)
                if texit > t and occupancy[c[0], c[1], c[2]]:
                    ridx.append(r), cells.append(tuple(c)), depth.append((t, texit))
                    if first:
                        break
                t = max(t, texit)
                if tmax[a] >= tf:
                    break
                c[a] += step[a]
                if c[a] < 0 or c[a] >= G:
                    break
                tmax[a] = F32(tmax[a] + tdelta[a])
    return (np.array(ridx, np.int32), np.array(cells, np.int32).reshape(-1, 3), np.array(depth, F32).reshape(-1, 2))


def first_hit_ref(origins, dirs, occupancy, level):
    """origins, dirs fp32 [N, 3]; occupancy bool [G, G, G] indexed [x][y][z]. -> (depth fp32 [N], hit bool [N], pidx int32 [N]):
    the first nugget of every finite ray that has one."""
    N = np.asarray(origins).shape[0]
    depth, hit, pidx = np.zeros(N, F32), np.zeros(N, bool), np.full(N, -1, np.int32)
    ridx, cells, t = walk_ref(origins, dirs, occupancy, level, finite_gate=True, first=True)
    depth[ridx], hit[ridx] = t[:, 0], True
    pidx[ridx] = [morton(int(x), int(y), int(z), level) for x, y, z in cells]
    return depth, hit, pidx
