"""Best-fp32 restatement of the volume-integration kernels (render.hip) in plain numpy, and the tau families the edge tests
use. TEST INFRASTRUCTURE ONLY.

`integrate_fwd` / `integrate_bwd` walk every pack in chunks of 64 samples exactly as one wave does: a Hillis-Steele
inclusive scan in float32 over the chunk, a float32 carry across chunks, float32 exp. The exclusive prefix of a sample comes
in one of two forms:

  prefix="shuffle"   the inclusive sum of the lane before it (lane 0: nothing) -- the kernels' form;
  prefix="subtract"  `incl - t`, the form the kernels had before. It cancels when one sample's tau dwarfs the ones before
                     it in the chunk: the small prefix is read back out of a sum whose ulp is as large as the prefix.

What this file is for: it shows on the CPU that the bars of tests/test_gpu_render_edges.py can be met by fp32 arithmetic
(shuffle form) and that the subtract form misses them on the wall families (tests/test_oracle_render.py).
"""
import numpy as np

F = np.float32


def tau_families(rng):
    """name -> float32 [n] optical depths of ONE pack. (a) is the family the older tests use; the others put a sample that
    dwarfs its predecessors ("wall") at chosen places of the 64-sample chunks."""
    fam = {}
    fam["a"] = (rng.random(257) ** 3 * 2.0).astype(F)
    fam["b"] = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), 129)).astype(F)      # log-uniform over 1e-6 .. 1e3
    c = np.zeros(128, F)
    c[70] = 1.0
    fam["c"] = c
    fam["d"] = np.concatenate([np.full(40, 1e-3), [1e3], np.full(20, 1e-3)]).astype(F)
    fam["e"] = np.concatenate([np.full(138, 1e-3), [1e3]]).astype(F)               # the wall sits in the third chunk
    fam["f"] = np.concatenate([np.full(63, 2e-4), [2e4]]).astype(F)
    fam["g"] = np.full(100, 3e-3, F)
    return fam


def _scan(v):
    """Inclusive Hillis-Steele scan of 64 float32 lanes (wave_incl_scan)."""
    v = v.copy()
    off = 1
    while off < 64:
        n = v.copy()
        n[off:] = v[off:] + v[:-off]
        v = n
        off <<= 1
    return v


def _wave_sum(v):
    """xor-butterfly sum of 64 float32 lanes (wave_sum); every lane ends with the same value."""
    v = v.copy()
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ off]
    return v[0]


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _exclusive(incl, t, prefix):
    if prefix == "subtract":
        return incl - t
    assert prefix == "shuffle"
    out = np.zeros(64, F)
    out[1:] = incl[:-1]
    return out


def _chunk(x, lo, hi):
    out = np.zeros((64,) + x.shape[1:], F)
    out[:hi - lo] = x[lo:hi]
    return out


def integrate_fwd(feats, tau, pack_start, prefix="shuffle"):
    """feats float32 [S, C], tau float32 [S], pack_start int [R + 1] -> ray float32 [R, C], weights float32 [S]."""
    feats, tau = np.asarray(feats, F), np.asarray(tau, F).reshape(-1)
    R, C = len(pack_start) - 1, feats.shape[1]
    ray, w_out = np.zeros((R, C), F), np.zeros(tau.shape[0], F)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            begin, end = int(pack_start[r]), int(pack_start[r + 1])
            carry, acc = F(0), np.zeros((64, C), F)
            for base in range(begin, end, 64):
                hi = min(base + 64, end)
                t = _chunk(tau, base, hi)
                incl = _scan(t)
                excl = carry + _exclusive(incl, t, prefix)
                w = np.exp(-excl) * (F(1) - np.exp(-t))
                w[hi - base:] = 0
                w_out[base:hi] = w[:hi - base]
                f = _chunk(feats, base, hi)
                for c in range(C):
                    acc[:, c] = _fma(w, f[:, c], acc[:, c])
                carry = carry + incl[63]
            for c in range(C):
                ray[r, c] = _wave_sum(acc[:, c])
    return ray, w_out


def integrate_bwd(feats, tau, pack_start, g_ray, g_w, prefix="shuffle"):
    """The backward of `integrate_fwd`: g_feats float32 [S, C], g_tau float32 [S]; g_w may be None (taken as zero)."""
    feats, tau = np.asarray(feats, F), np.asarray(tau, F).reshape(-1)
    g_ray = np.asarray(g_ray, F)
    R, C = len(pack_start) - 1, feats.shape[1]
    g_feats, g_tau = np.zeros_like(feats), np.zeros_like(tau)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            begin, end = int(pack_start[r]), int(pack_start[r + 1])
            carry = F(0)
            for base in range(begin, end, 64):
                hi = min(base + 64, end)
                t = _chunk(tau, base, hi)
                incl = _scan(t)
                g_tau[base:hi] = (carry + _exclusive(incl, t, prefix))[:hi - base]
                carry = carry + incl[63]
            suffix = F(0)
            for base in reversed(range(begin, end, 64)):
                hi = min(base + 64, end)
                n = hi - base
                t, excl, f = _chunk(tau, base, hi), _chunk(g_tau, base, hi), _chunk(feats, base, hi)
                T, et = np.exp(-excl), np.exp(-t)
                w = T * (F(1) - et)
                G = _chunk(np.asarray(g_w, F).reshape(-1), base, hi) if g_w is not None else np.zeros(64, F)
                for c in range(C):
                    G = _fma(np.full(64, g_ray[r, c], F), f[:, c], G)
                    g_feats[base:hi, c] = (w * g_ray[r, c])[:n]
                gw_term, e_term = G * w, G * T * et
                gw_term[n:] = 0
                incl_rev = _scan(gw_term[::-1])[::-1]                      # suffix sums: lane i gets sum_{k >= i}
                after = (incl_rev - gw_term) if prefix == "subtract" else np.concatenate([incl_rev[1:], [F(0)]]).astype(F)
                g_tau[base:hi] = (e_term - (suffix + after))[:n]
                suffix = suffix + incl_rev[0]
    return g_feats, g_tau


# The bars of tests/test_gpu_render.py, in one place for the GPU edge tests and for the CPU test that keeps them honest.
def assert_forward_close(ray, w, ray_ref, w_ref):
    np.testing.assert_allclose(np.asarray(ray), np.asarray(ray_ref), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.asarray(w).reshape(-1), np.asarray(w_ref).reshape(-1), rtol=1e-5, atol=1e-7)


def assert_backward_close(g_feats, g_tau, g_feats_ref, g_tau_ref, pack_start):
    """g_tau's absolute term scales with the largest reference gradient of the SAME pack, so that a wall pack (whose
    gradients are large) does not loosen its neighbours."""
    np.testing.assert_allclose(np.asarray(g_feats), np.asarray(g_feats_ref), rtol=1e-5, atol=1e-6)
    got, ref = np.asarray(g_tau).reshape(-1), np.asarray(g_tau_ref).reshape(-1)
    for r in range(len(pack_start) - 1):
        b, e = int(pack_start[r]), int(pack_start[r + 1])
        if e > b:
            np.testing.assert_allclose(got[b:e], ref[b:e], rtol=1e-4, atol=2e-6 * float(np.abs(ref[b:e]).max()),
                                       err_msg=f"g_tau, pack {r} rows [{b}, {e})")
