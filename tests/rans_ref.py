"""numpy reference of the "rans64" channel format (include/shacira_hip.h, "Interleaved rANS"): 64 coder states per block
advance in lockstep and share one stream of 16-bit words. Vectorised over lanes and blocks, loops over the step k. This is
the oracle of tests/test_rans_cpu.py and tests/test_gpu_rans.py; it shares no code with the library."""
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
