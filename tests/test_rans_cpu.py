"""The "rans64" codec without a GPU: the numpy reference (tests/rans_ref.py), the library's host coder (shacira_rans_*) and
the version-2 container of shacira_amd/codec.py. Integer work: every comparison is bit for bit."""
import ctypes
import json
import struct
import zlib

import numpy as np
import pytest
import torch

import rans_ref as R
from shacira_amd import _lib, codec


def _check_case(sym, freq, K):
    """host bytes == reference bytes, both decoders restore the symbols, and the words obey the rate condition."""
    sym = np.asarray(sym, dtype=np.int64)
    T = sym.size
    ref = R.encode_payload(sym, freq, K)
    host = codec.rans_encode(sym.astype(np.int32), freq, K)
    assert host == ref
    assert np.array_equal(codec.rans_decode(host, freq, T, K), sym)
    back, ok = R.decode_payload(ref, freq, T, K)
    assert ok and np.array_equal(back, sym)
    # rate: the final states hold at least the bits of the initial ones, so the words carry at most the model's
    # cross-entropy Hq; 0.1 % and 8 bytes per block of slack, as the format's description states it
    n_b, _, words = R.split_payload(ref, T, K)
    assert int(n_b.sum()) == words.size and len(ref) == 260 * n_b.size + 2 * words.size
    assert 2 * int(n_b.sum()) <= R.model_bytes(sym, freq) * 1.001 + 8 * n_b.size
    return ref


def _model_of(sym):
    sym = np.asarray(sym, dtype=np.int64)
    sym = sym - sym.min()
    return sym, codec.normalise_frequencies(np.bincount(sym))


@pytest.mark.parametrize("T,K", sorted(R.KNOWN_ANSWERS))
def test_known_answers(T, K):
    n_b, nbytes, crc, first_states, first_word = R.KNOWN_ANSWERS[(T, K)]
    sym = R.known_answer_symbols(T)
    ref = R.encode_payload(sym, R.KNOWN_FREQ, K)
    host = codec.rans_encode(sym.astype(np.int32), R.KNOWN_FREQ, K)
    for payload in (ref, host):
        counts, states, words = R.split_payload(payload, T, K)
        assert counts.tolist() == n_b and len(payload) == nbytes
        assert zlib.crc32(payload) == crc
        assert states[0, :4].tolist() == first_states
        if first_word is not None:
            assert int(words[0]) == first_word
    _check_case(sym, R.KNOWN_FREQ, K)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_lane_masks_and_partial_blocks(T):
    rng = np.random.default_rng(T)
    sym, freq = _model_of(np.round(rng.standard_normal(T) * 2))
    if freq.size == 1:                       # T == 1: a one-symbol model has no payload; code it under a wider one
        sym, freq = np.zeros(T, np.int64), np.array([65535, 1], dtype=np.uint32)
    _check_case(sym, freq, 4)


@pytest.mark.parametrize("K", [1, 4, 64, 4096])
def test_steps_per_block(K):
    rng = np.random.default_rng(K)
    sym, freq = _model_of(np.round(rng.standard_normal(3000) * 3))
    _check_case(sym, freq, K)


@pytest.mark.parametrize("kind", ["two", "skew", "gauss0.3", "gauss1", "gauss3", "wide"])
def test_distributions(kind):
    rng = np.random.default_rng(11)
    K = 64
    if kind == "two":
        sym = rng.integers(0, 2, 20_000)
    elif kind == "skew":
        sym = (rng.random(60_000) < 1e-4).astype(np.int64)
        sym[17] = 1                                                  # the rare symbol is present whatever the draw
    elif kind == "wide":
        sym = rng.integers(0, 36_000, 30_000)                        # ~20 000 distinct symbols over 36 000 bins
        assert 19_000 < np.unique(sym).size < 21_500
    else:
        sym = np.round(rng.standard_normal(40_000) * float(kind[5:]))
    sym, freq = _model_of(sym)
    if kind == "wide":
        assert freq.size > 16_384                                    # beyond any LDS-sized cdf table
    _check_case(sym, freq, K)


def test_fuzz_over_length_steps_and_bins():
    rng = np.random.default_rng(2)
    for it in range(60):
        nbins = int(rng.integers(2, 600))
        T = int(rng.integers(1, 5000))
        K = int(rng.choice([1, 2, 3, 5, 8, 16, 33, 4096]))
        w = rng.random(nbins) ** int(rng.integers(1, 8))
        sym = rng.choice(nbins, size=T, p=w / w.sum())
        counts = np.bincount(sym, minlength=nbins)
        if (counts > 0).sum() < 2:
            continue
        freq = codec.normalise_frequencies(counts)
        _check_case(sym, freq, K)


# ---- the host-coder twins of tests/test_gpu_rans_edges.py: the same inputs, held to the reference without a GPU ----
EDGE_CASES = R.model_edge_cases(codec.normalise_frequencies)


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_model_edges(name):
    sym, freqs, lo, K = EDGE_CASES[name]
    T = sym.shape[0]
    for c, freq in enumerate(freqs):
        n_b, _, words = R.split_payload(_check_case(sym[:, c], freq, K), T, K)
        if name.startswith("dominant"):
            assert n_b.tolist() == [1, 0, 0, 1]                      # only the outliers emit: the middle blocks are empty
        if name == "flat_65536":
            assert n_b.tolist() == [256, 256, 37] and words.size == T    # one word per symbol: the slot bound is met
        if name == "gauss":
            assert n_b[:2].min() > 0 and n_b[2] == 0 and 35 <= freq.size <= 60


@pytest.mark.parametrize("T", [1, 63, 64, 65, 128, 129])
def test_one_step_per_block(T):
    sym = R.known_answer_symbols(T)
    n_b, _, _ = R.split_payload(_check_case(sym, R.KNOWN_FREQ, 1), T, 1)
    assert n_b.size == -(-T // 64) and not n_b.any()                 # a state's first symbol never emits (every f > 1)
    _check_case(R.sparse_outliers(T, 0.1, T) ^ 1, np.array([1, 65535], dtype=np.uint32), 1)


def test_payload_corruptions_host_verdict_is_the_references():
    sym, freqs, lo, K = EDGE_CASES["gauss"]
    T, c = sym.shape[0], 1
    good = R.encode_payload(sym[:, c], freqs[c], K)
    lat = torch.from_numpy((sym + np.asarray(lo)[None, :]).astype(np.float32))
    blob = codec.compress_latents(lat, coder="rans", steps=K)
    off = codec._parse_rans(blob)[3][c]["payload_off"]
    assert blob[off:off + len(good)] == good
    cases = R.payload_corruptions(good, T, K)
    names = " ".join(n for n, _ in cases)
    assert len(cases) >= 25 and "word" in names and "below" in names and "state2." in names and "counts1<->2" in names
    for name, bad in cases:
        assert len(bad) == len(good) and bad != good, name
        want, ok = R.decode_payload(bad, freqs[c], T, K)
        container = blob[:off] + bad + blob[off + len(bad):]
        if ok:
            assert np.array_equal(codec.rans_decode(bad, freqs[c], T, K), want), name
            assert torch.equal(codec.decompress_latents(container)[:, c], torch.from_numpy(want + lo[c]).float()), name
        else:
            with pytest.raises(ValueError):
                codec.rans_decode(bad, freqs[c], T, K)
            with pytest.raises(ValueError):
                codec.decompress_latents(container)


LIMIT_LATENTS = R.container_limit_latents()


@pytest.mark.parametrize("name", sorted(LIMIT_LATENTS))
def test_containers_at_the_limits(name):
    lat = torch.from_numpy(LIMIT_LATENTS[name])
    blob = codec.compress_latents(lat, coder="rans", steps=4)
    T, ld, K, chans = codec._parse_rans(blob)
    sym = np.rint(LIMIT_LATENTS[name]).astype(np.int64)
    for c, ch in enumerate(chans):
        if ch["nbins"] > 1:
            size = 260 * -(-T // (64 * K)) + 2 * ch["words"]
            assert blob[ch["payload_off"]:ch["payload_off"] + size] == R.encode_payload(sym[:, c] - ch["lo"], ch["freq"], K)
    assert torch.equal(codec.decompress_latents(blob), torch.round(lat))
    if name == "permutation_65536":
        assert chans[0]["nbins"] == codec.RC_TOTAL and chans[0]["words"] == T and (chans[0]["freq"] == 1).all()
        wider = torch.arange(-7, 65530, dtype=torch.float32)[torch.randperm(65537, generator=torch.Generator().manual_seed(1))]
        with pytest.raises(ValueError):
            codec.compress_latents(wider[:, None], coder="rans", steps=4)         # 65 537 consecutive integers
    if name == "spike_in_zeros":
        assert chans[0]["freq"].tolist() == [65535, 0, 0, 1] and chans[0]["words"] == 1
        assert chans[0]["n_b"].size == 274 and int((chans[0]["n_b"] == 0).sum()) == 273
    if name == "sixteen_kinds":
        assert [ch["nbins"] for ch in chans[:6]] == [1, 2, 4, chans[3]["nbins"], 4095, 4096] and 8 < chans[3]["nbins"] < 30


SHAPES = [(5000, 1), (4096, 2), (777, 3), (0, 2), (1, 16)]


def _tie_latents(shape, constant_channel=True):
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(shape, generator=g) * 2.0
    if shape[0] > 10:
        ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0])
        lat[3:3 + ties.numel(), 0] = ties                             # torch.round is half to even
    if constant_channel and shape[1] > 1:
        lat[:, shape[1] - 1] = -3.25                                  # one bin: no payload
    return lat


def _sections(blob):
    """walk a version-2 container -> (header, [(table bytes, payload bytes)]) and check the padding"""
    assert blob[:6] == b"SHCR\x02\x00"
    (hl,) = struct.unpack_from("<I", blob, 6)
    header = json.loads(blob[10:10 + hl].decode())
    off = 10 + hl
    off += -off % 4
    T, K = header["rows"], header["steps"]
    nblocks = -(-T // (64 * K))
    out = []
    for ch in header["channels"]:
        if T == 0:
            continue
        table = blob[off:off + 2 * ch["nbins"]]
        off += 2 * ch["nbins"] + (-2 * ch["nbins"]) % 4
        size = 260 * nblocks + 2 * ch["words"] if ch["nbins"] > 1 else 0
        out.append((table, blob[off:off + size]))
        off += size + (-size) % 4
    assert off == len(blob) and len(blob) % 4 == 0
    return header, out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("steps", [None, 4])
def test_container_round_trip(shape, steps):
    lat = _tie_latents(shape)
    blob = codec.compress_latents(lat, coder="rans", steps=steps)
    header, sections = _sections(blob)
    assert header["coder"] == "rans64" and header["rows"] == shape[0] and header["latent_dim"] == shape[1]
    assert header["steps"] == (4096 if steps is None else steps)
    back = codec.decompress_latents(blob)
    assert back.dtype == torch.float32 and tuple(back.shape) == tuple(shape)
    assert torch.equal(back, torch.round(lat))
    assert codec.payload_bits(blob) == 8 * sum(len(p) for _, p in sections)
    if shape[0] and shape[1] > 1:
        ch = header["channels"][-1]
        assert ch["nbins"] == 1 and ch["words"] == 0 and sections[-1] == (b"\x00\x00", b"")
    # each payload is the reference's, under the model stored next to it
    sym = torch.round(lat).long().numpy()
    for c, (table, payload) in enumerate(sections):
        ch = header["channels"][c]
        if ch["nbins"] > 1:
            freq = np.frombuffer(table, dtype="<u2").astype(np.uint32)
            assert payload == R.encode_payload(sym[:, c] - ch["lo"], freq, header["steps"])


def test_default_coder_is_unchanged():
    lat = _tie_latents((4096, 2), constant_channel=False)
    blob = codec.compress_latents(lat)
    assert blob == codec.compress_latents(lat, coder="range") and blob[:6] == b"SHCR\x01\x00"
    assert torch.equal(codec.decompress_latents(blob), torch.round(lat))
    header = json.loads(blob[10:10 + struct.unpack_from("<I", blob, 6)[0]].decode())
    assert codec.payload_bits(blob) == 8 * sum(ch["payload"] for ch in header["channels"])
    with pytest.raises(ValueError):
        codec.compress_latents(lat, coder="huffman")
    with pytest.raises(ValueError):
        codec.compress_latents(lat, coder="rans", steps=0)


def test_limits():
    with pytest.raises(ValueError):
        codec.compress_latents(torch.zeros(4, 17), coder="rans")
    bad = torch.zeros(8, 1)
    bad[2] = float("inf")
    with pytest.raises(ValueError):
        codec.compress_latents(bad, coder="rans")
    bad[2] = 2.0 ** 30
    with pytest.raises(ValueError):
        codec.compress_latents(bad, coder="rans")
    wide = torch.arange(70_000, dtype=torch.float32)[:, None]         # more than 65536 distinct symbols in a channel
    with pytest.raises(ValueError):
        codec.compress_latents(wide, coder="rans")


def test_model_file_round_trip_with_the_rans_coder():
    from shacira_amd import harness
    torch.manual_seed(3)
    grid, _, _ = harness.kodak_like_grid(num_lods=6, max_grid_res=64)
    nef = harness.NeuralImage(grid, hidden_dim=16, num_layers=1)
    with torch.no_grad():
        grid.codebook.mul_(2.5)
    before = {k: v.clone() for k, v in nef.state_dict().items()}
    data = codec.save_model(nef, coder="rans")
    assert b"SHCR\x02\x00" in data and b"SHCR\x01\x00" not in data
    assert b"SHCR\x01\x00" in codec.save_model(nef)
    with torch.no_grad():
        for p in nef.parameters():
            p.add_(1.0)
    codec.load_model(nef, data)
    for k, v in before.items():
        assert torch.equal(nef.state_dict()[k], torch.round(v) if k.endswith("grid.codebook") else v), k
    assert grid.compress(coder="rans")[:6] == b"SHCR\x02\x00" and grid.compress()[:6] == b"SHCR\x01\x00"
    blob = grid.compress(coder="rans")
    want = grid.codebook.detach().clone()
    with torch.no_grad():
        grid.codebook.add_(3.0)
    grid.load_compressed(blob)
    assert torch.equal(grid.codebook.detach(), want)                 # the table held integers already


def _one_channel_container(T=1000, K=4):
    g = torch.Generator().manual_seed(9)
    lat = torch.randn((T, 1), generator=g) * 3.0
    blob = codec.compress_latents(lat, coder="rans", steps=K)
    header, sections = _sections(blob)
    payload_off = len(blob) - len(sections[0][1]) - (-len(sections[0][1])) % 4
    nblocks = -(-T // (64 * K))
    return lat, bytearray(blob), payload_off, nblocks


def test_corrupt_containers_raise_value_error():
    lat, blob, off, nblocks = _one_channel_container()
    assert torch.equal(codec.decompress_latents(bytes(blob)), torch.round(lat))
    for cut in (4, 9, 40, off - 2, off + 10, len(blob) - 4):          # truncated: magic, header, table, payload
        with pytest.raises(ValueError):
            codec.decompress_latents(bytes(blob[:cut]))
    bad = bytearray(blob)                                             # a count table whose sum disagrees
    struct.pack_into("<I", bad, off, struct.unpack_from("<I", bad, off)[0] + 1)
    with pytest.raises(ValueError):
        codec.decompress_latents(bytes(bad))
    bad = bytearray(blob)                                             # ... or moves a word from one block to the next
    struct.pack_into("<I", bad, off, struct.unpack_from("<I", bad, off)[0] + 1)
    struct.pack_into("<I", bad, off + 4, struct.unpack_from("<I", bad, off + 4)[0] - 1)
    with pytest.raises(ValueError):
        codec.decompress_latents(bytes(bad))
    bad = bytearray(blob)                                             # a state below 2^16
    struct.pack_into("<I", bad, off + 4 * nblocks + 4 * 5, 0xFFFF)
    with pytest.raises(ValueError):
        codec.decompress_latents(bytes(bad))
    words_off = off + 260 * nblocks
    rng = np.random.default_rng(4)
    for pos in [off + 4 * nblocks + 1, words_off, words_off + 1, len(blob) - 1] + \
            [int(p) for p in rng.integers(off + 4 * nblocks, len(blob), 40)]:
        bad = bytearray(blob)                                         # a flipped payload byte: p underflows or the end
        bad[pos] ^= 0x10                                              # states are not the encoder's initial ones
        with pytest.raises(ValueError):
            codec.decompress_latents(bytes(bad))


def test_host_decoder_survives_random_bytes():
    """whatever the bytes, the host decoder returns 0 or EINVAL (its reads are checked against `len`)"""
    rng = np.random.default_rng(5)
    L = _lib.lib()
    freq = np.array([40000, 20000, 5000, 500, 36], dtype=np.uint32)
    out = np.zeros(300, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for it in range(200):
        K = int(rng.choice([1, 2, 4]))
        nblocks = -(-300 // (64 * K))
        words = int(rng.integers(0, 300))
        buf = rng.integers(0, 256, 260 * nblocks + 2 * words, dtype=np.uint8)
        if it % 2:                                                    # legal counts and states, random words
            n_b = rng.multinomial(words, np.ones(nblocks) / nblocks).astype("<u4")
            buf[:4 * nblocks] = np.frombuffer(n_b.tobytes(), np.uint8)
            st = (rng.integers(1 << 16, 1 << 32, 64 * nblocks)).astype("<u4")
            buf[4 * nblocks:260 * nblocks] = np.frombuffer(st.tobytes(), np.uint8)
        rc = L.shacira_rans_decode(p(buf), buf.size, p(freq), 5, 300, K, p(out))
        assert rc in (0, _lib.EINVAL)
        assert out.min() >= 0 and out.max() < 5


def test_argument_checks_of_the_new_entry_points():
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    freq = np.array([65535, 1], dtype=np.uint32)
    sym = np.array([0, 1, 0], dtype=np.int32)
    out = np.zeros(1024, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    enc, dec = L.shacira_rans_encode, L.shacira_rans_decode
    assert L.shacira_rans_encode_bound(1000, 8) == 2 * 260 + 2000 and L.shacira_rans_encode_bound(0, 8) == 0
    assert L.shacira_rans_encode_bound(10, 0) == 0
    assert enc(p(sym), 3, p(freq), 2, 4, p(out), 1024, ctypes.byref(n)) == 0 and n.value >= 260
    good = out[:n.value].copy()
    assert enc(p(sym), 3, p(np.array([65535, 2], np.uint32)), 2, 4, p(out), 1024, ctypes.byref(n)) == _lib.EINVAL
    assert enc(p(sym), 3, p(np.array([65536], np.uint32)), 1, 4, p(out), 1024, ctypes.byref(n)) == _lib.EINVAL
    assert enc(p(np.array([2], np.int32)), 1, p(freq), 2, 4, p(out), 1024, ctypes.byref(n)) == _lib.EINVAL
    assert enc(p(np.array([1], np.int32)), 1, p(np.array([65535, 0, 1], np.uint32)), 3, 4, p(out), 1024,
               ctypes.byref(n)) == _lib.EINVAL                                               # symbol of frequency 0
    assert enc(p(sym), 3, p(freq), 2, 0, p(out), 1024, ctypes.byref(n)) == _lib.EINVAL        # steps
    assert enc(p(sym), 3, p(freq), 2, 65537, p(out), 1024, ctypes.byref(n)) == _lib.EINVAL
    assert enc(None, 3, p(freq), 2, 4, p(out), 1024, ctypes.byref(n)) == _lib.EINVAL
    assert enc(p(sym), 3, p(freq), 2, 4, p(out), 100, ctypes.byref(n)) == _lib.EWORKSPACE and n.value == good.size
    assert enc(None, 0, p(freq), 2, 4, p(out), 1024, ctypes.byref(n)) == 0 and n.value == 0   # empty: no block
    back = np.zeros(3, dtype=np.int32)
    assert dec(p(good), good.size, p(freq), 2, 3, 4, p(back)) == 0 and back.tolist() == [0, 1, 0]
    assert dec(p(good), good.size - 1, p(freq), 2, 3, 4, p(back)) == _lib.EINVAL
    assert dec(p(good), good.size, p(freq), 2, 3, 0, p(back)) == _lib.EINVAL
    assert dec(p(good), good.size, p(freq), 2, 3, 4, None) == _lib.EINVAL
    assert dec(None, 0, p(freq), 2, 0, 4, None) == 0
    # device entry points: everything is refused before any HIP call (no GPU here), and zero rows launch nothing
    one = ctypes.c_void_p(16)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    e = L.shacira_latent_rans_encode
    assert e(-1, 1, one, i32(0), i32(5), one, 6, 4, one, one, one, None) == _lib.EINVAL
    assert e(100, 0, one, i32(0), i32(5), one, 6, 4, one, one, one, None) == _lib.EINVAL
    assert e(100, 17, one, i32(*[0] * 17), i32(*[5] * 17), one, 6, 4, one, one, one, None) == _lib.EDTYPE
    assert e(100, 1, one, i32(0), i32(5), one, 5, 4, one, one, one, None) == _lib.EINVAL      # cdf_stride < nbins + 1
    assert e(100, 1, one, i32(0), i32(65537), one, 70000, 4, one, one, one, None) == _lib.EINVAL
    assert e(100, 1, one, i32(0), i32(5), one, 6, 0, one, one, one, None) == _lib.EINVAL      # steps
    assert e(100, 1, None, i32(0), i32(5), one, 6, 4, one, one, one, None) == _lib.EINVAL     # NULL latents
    assert e(100, 1, one, None, i32(5), one, 6, 4, one, one, one, None) == _lib.EINVAL
    assert e(0, 1, None, i32(0), i32(5), None, 6, 4, None, None, None, None) == 0
    k = L.shacira_latent_rans_pack
    size = 260 * 1 + 2 * 60
    assert k(100, 1, i32(5), 4, one, one, one, one, i64(0), i64(60), one, size - 1, None) == _lib.EINVAL   # ends beyond
    assert k(100, 1, i32(5), 4, one, one, one, one, i64(2), i64(60), one, size + 4, None) == _lib.EINVAL   # misaligned
    assert k(100, 1, i32(5), 4, one, one, one, one, i64(0), i64(101), one, 1 << 20, None) == _lib.EINVAL   # words > rows
    assert k(100, 1, i32(5), 4, one, one, one, one, None, i64(60), one, size, None) == _lib.EINVAL
    assert k(100, 1, i32(5), 4, one, one, one, None, i64(0), i64(60), one, size, None) == _lib.EINVAL
    assert k(0, 1, i32(5), 4, None, None, None, None, i64(0), i64(0), None, 0, None) == 0
    d = L.shacira_latent_rans_decode
    assert d(100, 1, one, size - 1, i32(0), i32(5), i64(0), i64(60), one, 6, one, 4, one, one, None) == _lib.EINVAL
    assert d(100, 1, one, size, i32(0), i32(5), i64(-4), i64(60), one, 6, one, 4, one, one, None) == _lib.EINVAL
    assert d(100, 1, one, size, i32(0), i32(5), i64(0), i64(60), one, 5, one, 4, one, one, None) == _lib.EINVAL
    assert d(100, 1, one, size, i32(0), i32(5), i64(0), i64(60), one, 6, one, 4, one, None, None) == _lib.EINVAL
    assert d(100, 1, None, size, i32(0), i32(5), i64(0), i64(60), one, 6, one, 4, one, one, None) == _lib.EINVAL
    assert d(100, 17, one, size, i32(*[0] * 17), i32(*[5] * 17), i64(*[0] * 17), i64(*[60] * 17), one, 6, one, 4, one,
             one, None) == _lib.EDTYPE
    assert d(0, 1, None, 0, i32(0), i32(5), i64(0), i64(0), None, 6, None, 4, None, one, None) == 0
