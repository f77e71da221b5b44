"""numpy reference of the "rans64" channel format (include/shacira_hip.h, "Interleaved rANS"): 64 coder states per block
advance in lockstep and share one stream of 16-bit words. Vectorised over lanes and blocks, loops over the step k. This is
the oracle of tests/test_rans_cpu.py, tests/test_gpu_rans.py and tests/test_gpu_rans_edges.py; it shares no code with the
library. The edge models, corruptions and limit latents those files share are built below the coder."""
import numpy as np

LANES = 64
X0 = 1 << 16


def _cdf(freq):
    freq = np.asarray(freq, dtype=np.int64)
    assert int(freq.sum()) == 1 << 16
    return np.concatenate([[0], np.cumsum(freq)]).astype(np.int64)


def _geometry(T, K):
    nblocks = -(-T // (LANES * K))
    idx = (np.arange(nblocks, dtype=np.int64)[:, None, None] * K + np.arange(K, dtype=np.int64)[None, :, None]) * LANES \
        + np.arange(LANES, dtype=np.int64)[None, None, :]
    return nblocks, idx                                            # idx [nblocks, K, 64]: the symbol a lane owns at a step


def encode_blocks(sym, freq, K):
    """-> (n_b uint32 [nblocks], states uint32 [nblocks, 64], words uint16 [sum n_b] in block order)."""
    sym = np.asarray(sym, dtype=np.int64)
    freq = np.asarray(freq, dtype=np.int64)
    cdf = _cdf(freq)
    T = sym.size
    nblocks, idx = _geometry(T, K)
    x = np.full((nblocks, LANES), X0, dtype=np.int64)
    emitted = np.zeros((nblocks, K, LANES), dtype=bool)            # second axis: order of emission (k descending)
    values = np.zeros((nblocks, K, LANES), dtype=np.uint16)
    for step, k in enumerate(range(K - 1, -1, -1)):
        i = idx[:, k, :]
        active = i < T
        s = sym[np.minimum(i, max(T - 1, 0))] if T else np.zeros_like(i)
        f = np.where(active, freq[s], 1)
        c = np.where(active, cdf[s], 0)
        emit = active & (x >= (f << 16))
        emitted[:, step, :] = emit
        values[:, step, :] = (x & 0xFFFF).astype(np.uint16)
        x = np.where(emit, x >> 16, x)
        x = np.where(active, ((x // f) << 16) + (x % f) + c, x)
    n_b = emitted.reshape(nblocks, -1).sum(axis=1).astype(np.uint32)
    return n_b, x.astype(np.uint32), values[emitted]               # boolean indexing walks block, step, lane in order


def decode_blocks(n_b, states, words, freq, T, K):
    """Inverse of encode_blocks -> (symbols int64 [T], ok): ok is False when p underflows or the end state is wrong."""
    freq = np.asarray(freq, dtype=np.int64)
    cdf = _cdf(freq)
    nblocks, idx = _geometry(T, K)
    n_b = np.asarray(n_b, dtype=np.int64)
    assert n_b.shape == (nblocks,) and int(n_b.sum()) == len(words)
    start = np.concatenate([[0], np.cumsum(n_b)[:-1]]) if nblocks else np.zeros(0, np.int64)
    words = np.concatenate([np.asarray(words, dtype=np.int64), [0]])          # a dummy slot for lanes that read nothing
    x = np.asarray(states, dtype=np.int64).reshape(nblocks, LANES).copy()
    p = n_b.copy()
    out = np.zeros(T, dtype=np.int64)
    ok = True
    for k in range(K):
        i = idx[:, k, :]
        active = i < T
        slot = x & 0xFFFF
        s = np.searchsorted(cdf, slot, side="right") - 1
        s = np.clip(s, 0, freq.size - 1)
        x = np.where(active, freq[s] * (x >> 16) + slot - cdf[s], x)
        out[i[active]] = s[active]
        need = active & (x < X0)
        n = need.sum(axis=1)
        rank = np.cumsum(need, axis=1) - need
        pos = (p - n)[:, None] + rank
        if np.any((p - n) < 0):
            ok = False
        pos = np.clip(pos, 0, np.maximum(n_b - 1, 0)[:, None]) + start[:, None]
        w = words[np.where(need, pos, len(words) - 1)]
        x = np.where(need, (x << 16) | w, x)
        p = p - n
    ok = ok and bool(np.all(p == 0)) and bool(np.all(x == X0))
    return out, ok


def encode_payload(sym, freq, K):
    """Channel payload: n_b u32 x nblocks, states u32 x 64 x nblocks (block-major), words u16; little endian."""
    n_b, states, words = encode_blocks(sym, freq, K)
    return n_b.astype("<u4").tobytes() + states.astype("<u4").tobytes() + words.astype("<u2").tobytes()


def split_payload(payload, T, K):
    nblocks = -(-T // (LANES * K))
    n_b = np.frombuffer(payload, dtype="<u4", count=nblocks)
    states = np.frombuffer(payload, dtype="<u4", count=nblocks * LANES, offset=4 * nblocks).reshape(nblocks, LANES)
    words = np.frombuffer(payload, dtype="<u2", offset=260 * nblocks)
    return n_b, states, words


def decode_payload(payload, freq, T, K):
    n_b, states, words = split_payload(payload, T, K)
    return decode_blocks(n_b, states, words, freq, T, K)


def block_starts(n_b):
    """exclusive prefix of the per-block word counts: the index of a block's first word in the channel's stream"""
    n_b = np.asarray(n_b, dtype=np.int64)
    return np.cumsum(n_b) - n_b


# ---- one-step corruptions of a well-formed payload (the sections keep their sizes; the count sum is preserved) ----
def flip_word(payload, T, K, index, bit):
    nblocks = -(-T // (LANES * K))
    out = bytearray(payload)
    out[260 * nblocks + 2 * index + bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def flip_state(payload, T, K, block, lane, bit):
    nblocks = -(-T // (LANES * K))
    out = bytearray(payload)
    out[4 * nblocks + 4 * (block * LANES + lane) + bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def swap_counts(payload, T, K, b0, b1):
    out = bytearray(payload)
    out[4 * b0:4 * b0 + 4], out[4 * b1:4 * b1 + 4] = payload[4 * b1:4 * b1 + 4], payload[4 * b0:4 * b0 + 4]
    return bytes(out)


# ---- hand-built models at the coder's edges: name -> (symbols int64 [T, ld], [freq per channel], lo per channel, K) ----
T_EDGE = 64 * 4 * 3 + 5            # K = 4: three full blocks and one of five symbols


def _sparse(T, at, common, rare):
    sym = np.full(T, common, dtype=np.int64)
    sym[list(at)] = rare
    return sym[:, None]


def _u32(*f):
    return np.array(f, dtype=np.uint32)


def gauss_case(normalise, T=64 * 16 * 2 + 37, ld=2, sigma=6.0, seed=24):
    """~40 bins per channel under `normalise` (counts -> frequencies that sum to 2^16) of each channel's own counts, so
    bin 0 and the last bin are present as in a container; K = 16: two full blocks and one of 37 symbols that emits nothing."""
    rng = np.random.default_rng(seed)
    sym = np.rint(rng.standard_normal((T, ld)) * sigma).astype(np.int64)
    lo = sym.min(axis=0)
    sym = sym - lo[None, :]
    freqs = [normalise(np.bincount(sym[:, c])) for c in range(ld)]
    return sym, freqs, [int(v) for v in lo], 16


def model_edge_cases(normalise):
    rng = np.random.default_rng(17)
    T, at = T_EDGE, (10, 64 * 4 * 3 + 2)                             # outliers in the first and the last block only
    cases = {
        "dominant_first": (_sparse(T, at, 0, 1), [_u32(65535, 1)], [7], 4),
        "dominant_first_plateau": (_sparse(T, at, 0, 3), [_u32(65535, 0, 0, 1)], [-5], 4),
        "dominant_last": (_sparse(T, at, 1, 0), [_u32(1, 65535)], [0], 4),
        "flat_65536": (rng.integers(0, 65536, (64 * 4 * 2 + 37, 1)), [np.ones(65536, np.uint32)], [-32768], 4),
    }
    f4095 = np.full(4095, 16, dtype=np.uint32)
    f4095[:16] += 1                                                  # 4095 * 16 + 16 = 65536
    f4096 = np.concatenate([f4095, [1]]).astype(np.uint32)           # the extra bin at f = 1 ...
    f4096[0] -= 1                                                    # ... taken from bin 0
    below = rng.integers(0, 4095, (T, 1))
    below[:3, 0] = (0, 4094, 15)
    cases["lds_4095"] = (below, [f4095], [3], 4)
    cases["lds_4096"] = (below, [f4096], [3], 4)
    cases["lds_4095_beside_4096"] = (np.concatenate([below, below[::-1]], axis=1), [f4095, f4096], [-4000, 100], 4)
    cases["gauss"] = gauss_case(normalise)
    return cases


def sparse_outliers(T, rate, seed):
    """symbols of a (65535, 1) model: 0 except for 1s at `rate`; the last symbol is a 0"""
    sym = (np.random.default_rng(seed).random(T) < rate).astype(np.int64)
    sym[-1] = 0
    return sym


def container_limit_latents():
    """name -> fp32 [T, ld] latents whose containers sit on the format's limits (the values carry fractions that round away)"""
    rng = np.random.default_rng(23)
    cases = {"permutation_65536": (rng.permutation(65536) - 30000).astype(np.float32)[:, None]}   # every f = 1
    spike = np.zeros((70_000, 1), dtype=np.float32)
    spike[41_234] = 3.0                                              # counts (69999, 0, 0, 1) -> freq (65535, 0, 0, 1)
    cases["spike_in_zeros"] = spike
    T = 4301
    dominant = np.zeros(T)
    dominant[[5, 2000, T - 1]] = 3.0
    kinds = [np.full(T, -3.0), rng.integers(0, 2, T).astype(np.float64), dominant, np.rint(rng.standard_normal(T) * 2.0),
             rng.permutation(T) % 4095, rng.permutation(T) % 4096]
    cols = [kinds[c % 6] + (0, 11, -700, 2500)[c % 4] * (c // 6) for c in range(16)]
    mix = np.stack(cols, axis=1) + rng.uniform(-0.3, 0.3, (T, 16))
    cases["sixteen_kinds"] = mix.astype(np.float32)
    return cases


def payload_corruptions(payload, T, K):
    """[(name, corrupt payload)]: single flipped bits in words and final states, and swapped block counts. Deterministic."""
    n_b, states, words = split_payload(payload, T, K)
    nblocks = n_b.size
    starts = block_starts(n_b)
    rng = np.random.default_rng(5)
    out = []
    picks = {0: 0, int(words.size) - 1: 15}                          # word index -> bit
    for b in range(nblocks):
        if n_b[b]:
            picks.setdefault(int(starts[b]), 7)                      # first and last word of every block that has any
            picks.setdefault(int(starts[b] + n_b[b]) - 1, 8)
    for w in rng.integers(0, words.size, 10):
        picks.setdefault(int(w), int(rng.integers(0, 16)))
    out += [(f"word{w}^bit{bit}", flip_word(payload, T, K, w, bit)) for w, bit in sorted(picks.items())]
    for b in range(nblocks):
        live = min(LANES, T - b * LANES * K)                         # lanes of the block that own a symbol
        lanes = {0: 0, live - 1: 31, live // 2: 16}
        if live < LANES:
            lanes.update({live: 0, LANES - 1: 16})                   # idle lanes hold 2^16: bit 16 pushes them to 0
        out += [(f"state{b}.{l}^bit{bit}", flip_state(payload, T, K, b, l, bit)) for l, bit in sorted(lanes.items())]
    low = np.argwhere(states < (1 << 17))                            # bit 16 of these pushes the state below 2^16
    out += [(f"state{b}.{l}->below", flip_state(payload, T, K, int(b), int(l), 16)) for b, l in low[:4]]
    out += [(f"counts{b}<->{b + 1}", swap_counts(payload, T, K, b, b + 1)) for b in range(nblocks - 1)]
    return out


def model_bytes(sym, freq):
    """Hq of the issue: the model's cross-entropy of the symbols, in bytes."""
    counts = np.bincount(np.asarray(sym, dtype=np.int64), minlength=len(freq))
    m = counts > 0
    return float(-(counts[m] * np.log2(np.asarray(freq, dtype=np.float64)[m] / 65536.0)).sum()) / 8.0


def known_answer_symbols(T):
    i = np.arange(T, dtype=np.int64)
    return np.array([0, 0, 1, 0, 2, 0, 1, 3, 0, 4], dtype=np.int64)[(i * i) % 10]


KNOWN_FREQ = np.array([40000, 20000, 5000, 500, 36], dtype=np.uint32)
# (T, K) -> (n_b, payload bytes, CRC-32 of the payload, first four states of block 0, first word or None)
KNOWN_ANSWERS = {
    (1000, 8): ([83, 79], 844, 0xC8991B9C, [0x43404, 0x2E62C38, 0x2FC12, 0x3FFFFFF3], 0xFFEC),
    (130, 2): ([7, 0], 534, 0x507F7427, [0x60860, 0x22B40, 0x30F2C0, 0x32FFF0], None),
}
