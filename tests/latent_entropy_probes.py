"""Probe set of the per-element entropy tests (CPU: tests/test_oracle_golden.py; GPU: tests/test_gpu_latent_edges.py).
TEST INFRASTRUCTURE ONLY.

Eight parameter sets x eight inputs w = 64 probes per (num_layers, LD). For LD = 8 the sets are the eight channels of one
parameter tensor and the inputs its eight rows; for LD = 1 each set is a tensor of its own.

Parameter sets (the same h / b / a in every layer, so whichever layers ``num_layers`` applies see them -- except h = -10,
which sits in the final layer only, over h = 0 in the layers before it: with softplus(-10) = 4.5e-5 in every layer the CDF of
two or more layers is flat to 1e-10, prob is 0 in fp32 at every w and no probe of the set would be resolvable):
  h in {-10, 0, 19.9, 20.0, 20.1, 30}: softplus far below, at, just under / on / over torch's threshold 20 and far above it;
  a in {-5, 0, 5}: tanh(a) saturated either way; b != 0 places the mode off zero.
Inputs of each set: both far tails (-40, 40), the mode, a mid tail, w + 0.5 and w - 0.5 landing within 1e-4 of the first
layer's u = 0 (where 1 - 2 / (e + 1) cancels), and -- found by scanning the float32 restatement -- the w where prob first
rounds to 0 in the upper tail and where prob (+ 1e-10) first rounds to 1 (else the w of the largest prob).
"""
import numpy as np

from oracle import latent as ol

EPS32 = float(np.finfo(np.float32).eps)

#        name          h      b      a
SETS = [("h-10",     -10.0,  0.0,   0.0),
        ("h0",         0.0,  0.0,   0.0),
        ("h19.9",     19.9,  0.25,  0.0),
        ("h20.0",     20.0, -0.25,  0.0),
        ("h20.1",     20.1,  0.0,   0.3),
        ("h30",       30.0,  3.0,  -0.3),
        ("a5_b0.3",    0.5,  0.3,   5.0),
        ("a-5_b-0.7",  0.5, -0.7,  -5.0)]
INPUTS = ["w-40", "w40", "mode", "midtail", "u_hi~+1e-4", "u_lo~-1e-4", "first_prob0", "first_prob1_or_max"]


def set_params(i):
    """[4, 3, 1] float32 of parameter set i."""
    _, h, b, a = SETS[i]
    p = np.zeros((4, 3, 1), np.float32)
    p[:, 0, 0], p[:, 1, 0] = h, b
    if h == -10.0:
        p[:3, 0, 0] = 0.0
    p[:3, 2, 0] = a
    return p


def set_inputs(i, num_layers):
    """The eight float32 inputs w of parameter set i (they depend on num_layers through the scan)."""
    prm = set_params(i)
    first = 0 if num_layers > 1 else 3
    h, b = float(prm[first, 0, 0]), float(prm[first, 1, 0])
    sp = h if h > 20.0 else float(np.log1p(np.exp(h)))
    x0 = -b / sp                                            # u = 0 of the first applied layer
    grid = np.arange(-40.0, 40.0 + 1e-9, 0.03125).astype(np.float32).reshape(-1, 1)
    r = ol.entropy_elements_f32(grid, np.zeros_like(grid), prm, num_layers)
    prob, q = r["prob"][:, 0], r["q"][:, 0]
    top = int(np.argmax(prob))
    zero = np.nonzero((prob == 0) & (np.arange(prob.size) > top))[0]
    one = np.nonzero(q == 1)[0]
    w = [-40.0, 40.0, float(np.clip(x0, -39.0, 39.0)), float(np.clip(x0 + 3.3, -39.0, 39.0)),
         float(np.clip((1e-4 - b) / sp - 0.5, -39.0, 39.0)), float(np.clip((-1e-4 - b) / sp + 0.5, -39.0, 39.0)),
         float(grid[zero[0], 0]) if zero.size else 39.5, float(grid[one[0], 0]) if one.size else float(grid[top, 0])]
    return np.asarray(w, np.float32)


def probes(num_layers, ld):
    """-> list of (names [R][ld], latent [R, ld] float32, params [4, 3, ld] float32): one entry for ld = 8 (eight rows), eight
    for ld = 1 (eight rows each). The noise of every probe is 0: w = latent."""
    assert ld in (1, 8)
    per_set = [(set_params(i), set_inputs(i, num_layers)) for i in range(8)]
    if ld == 1:
        return [([[f"{SETS[i][0]}/{n}"] for n in INPUTS], w.reshape(8, 1), p) for i, (p, w) in enumerate(per_set)]
    names = [[f"{SETS[i][0]}/{INPUTS[r]}" for i in range(8)] for r in range(8)]
    latent = np.stack([w for _, w in per_set], axis=1)
    params = np.concatenate([p for p, _ in per_set], axis=2)
    return [(names, np.ascontiguousarray(latent), np.ascontiguousarray(params))]


TINY32 = float(np.finfo(np.float32).tiny)      # below it float32 has no full-precision values: the floor of every allowance


def prob_error_units(num_layers):
    """Largest |prob_fp32 - prob_fp64| of the float32 restatement against the fp64 oracle over the probe set, in units of
    eps32 * (s_hi + s_lo) (+ TINY32) -- the measured constant of the kernel's allowance (see delta())."""
    worst = 0.0
    for _, lat, prm in probes(num_layers, 8):
        z = np.zeros_like(lat)
        a, b = ol.entropy_elements_f32(lat, z, prm, num_layers), ol.entropy_elements(lat, z, prm, num_layers)
        unit = EPS32 * (b["s_hi"] + b["s_lo"]) + TINY32
        worst = max(worst, float((np.abs(a["prob"].astype(np.float64) - b["prob"]) / unit).max()))
    return worst


# Measured by tests/test_oracle_golden.py::test_float32_entropy_restatement_against_fp64 (which prints it and pins it to
# these figures): the largest error of the float32 restatement's prob over the probes of each num_layers, in units of
# eps32 * (s_hi + s_lo). It is reached in the lower tail (w = -40), where the sigmoid's argument z ~ -30 is rounded to
# eps32 |z| and the sigmoid, ~ exp(z) there, takes that as a RELATIVE error.
MEASURED_PROB_UNITS = {1: 6.25, 2: 14.44, 3: 26.99, 4: 26.34}
KERNEL_FACTOR = 2.0          # the kernel adds __expf, __frcp_rn and __log2f (1-2 ulp each) to what the restatement rounds
LN2 = float(np.log(2.0))


def kernel_units(num_layers):
    return KERNEL_FACTOR * MEASURED_PROB_UNITS[num_layers]


def delta(s_hi, s_lo, num_layers):
    """Allowance on the kernel's prob: twice the measured error of the float32 restatement."""
    return kernel_units(num_layers) * EPS32 * (s_hi + s_lo) + TINY32


def bits64(prob):
    """float64 bits of a (possibly non-positive) prob: clamp(-log2(prob + 1e-10), 0, 50); the log of q <= 0 counts as +inf."""
    q = np.asarray(prob, np.float64) + 1e-10
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q > 0, np.clip(-np.log2(np.where(q > 0, q, 1.0)), 0.0, 50.0), 50.0)


def bits_interval(prob, d):
    """[lo, hi] of the bits for a prob known to +-d, widened by the 4 fp32 roundings of the value itself (log2 at 1-2 ulp, the
    negation and clamp exact, one more for a different but equivalent order such as log / ln 2)."""
    lo, hi = bits64(prob + d), bits64(prob - d)
    return lo * (1 - 4 * EPS32) - TINY32, hi * (1 + 4 * EPS32) + TINY32


def grad_interval(q32, d, el, num_layers, grad_total):
    """[lo, hi] of d(total bits)/dw * grad_total per element: -grad_total / (ln 2 q) * (ds_hi - ds_lo), or 0 where the clamp
    masks (bits outside [0, 50], i.e. q > 1 or q < 2^-50), for every q within +-d of the float32 restatement's q32 and ds
    within its rounding bound. ``el`` = oracle.latent.entropy_elements(...).

    Bound on D = ds_hi - ds_lo, ds = s (1 - s) * chain: s is known to C eps32 s (C = kernel_units), hence 1 - s to the same
    ABSOLUTE error and s (1 - s) to (C + 2) eps32 s; per Bitparm layer tanh is known to 4 eps32 absolutely (tanhf_fast), so
    1 - th^2 to 8, the factor 1 + (1 - th^2) tanh(a) with its two roundings to 10 relative to its absolute counterpart, and two
    more multiplications: 12 per layer; 3 for the products with 1/q, grad_total and the final sum."""
    C = kernel_units(num_layers)
    c_d = (C + 2) + 12 * (num_layers - 1) + 3
    D = el["ds_hi"] - el["ds_lo"]
    tol_d = c_d * EPS32 * (el["s_hi"] * el["slope_hi"] + el["s_lo"] * el["slope_lo"]) + TINY32
    q32 = np.asarray(q32, np.float64)
    q_lo, q_hi = q32 - d, q32 + d
    with np.errstate(divide="ignore"):
        gp_max = np.where(q_lo > 0, 1.0 / (LN2 * np.where(q_lo > 0, q_lo, 1.0)), np.inf)      # largest |d bits / d prob|
    gp_min = np.where((q_hi >= 1.0) | (q_lo <= 2.0 ** -50), 0.0, 1.0 / (LN2 * q_hi))          # 0: the mask may apply
    gp_max = np.where(q_lo > 1.0, 0.0, gp_max)                                                # certainly masked
    d_lo, d_hi = D - tol_d, D + tol_d
    with np.errstate(invalid="ignore"):
        cands = np.stack([-gp_min * d_lo, -gp_min * d_hi, -gp_max * d_lo, -gp_max * d_hi]) * grad_total
    cands = np.where(np.isnan(cands), 0.0, cands)                                             # inf * 0
    lo, hi = cands.min(0), cands.max(0)
    unbounded = np.isinf(gp_max)
    return np.where(unbounded, -np.inf, lo), np.where(unbounded, np.inf, hi)


def legit_differences(r32):
    """The probes where fp32 and fp64 legitimately part (``r32`` = oracle.latent.entropy_elements_f32(...)): -> (tail, one)
    boolean masks. tail: the upper tail, both sigmoids above 1/2 and prob 0 or within 8 ulps of 1 of it; one: prob + 1e-10
    rounds to exactly 1, the bits are -0.0 and the clamp passes the gradient."""
    tail = (r32["s_lo"] > 0.5) & (r32["prob"] <= 8 * EPS32)
    return tail, r32["q"] == 1
