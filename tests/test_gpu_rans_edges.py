"""The rans64 kernels and the two symbol-statistics kernels of symbols.hip at their edges, against numpy (tests/rans_ref.py,
np.unique / np.bincount): hand-built models driven straight into the kernels (a symbol that owns all but one slot, cdf plateaus,
65 536 bins of f = 1, the two sides of the LDS cdf limit), 1 and 65 536 steps per block, payloads with one flipped bit or two
swapped counts -- refused exactly where the reference refuses them -- containers on the format's limits, and histograms on the
LDS-bin boundary, past the workgroup cap and at the rounding ties, the clamp and the non-finite values. Integer work: every
comparison is exact. tests/test_rans_cpu.py holds the host coder to the same inputs without a GPU."""
import numpy as np
import pytest
import torch

import rans_ref as R
from shacira_amd import codec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from shacira_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ops():
    from shacira_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------ direct-model harness
def _latent(sym, lo, dev):
    return torch.from_numpy((sym + np.asarray(lo, dtype=np.int64)[None, :]).astype(np.float32)).to(dev)


def _encode(dev, sym, freqs, lo, K):
    """device payloads of sym [T, ld] under hand-built models == the reference's == the host coder's"""
    payloads = _ops().latent_rans_encode(_latent(sym, lo, dev), lo, [len(f) for f in freqs], codec.cdf_table(freqs), K)
    assert len(payloads) == len(freqs)
    for c, freq in enumerate(freqs):
        ref = R.encode_payload(sym[:, c], freq, K)
        assert payloads[c] == ref, f"channel {c}: device bytes differ from the reference"
        assert codec.rans_encode(sym[:, c].astype(np.int32), freq, K) == ref, f"channel {c}: host bytes differ"
    return payloads


def _pack(payloads, T, K):
    """-> (bytes of the payloads, each padded to 4; offsets; words; block_start [ld, nblocks] from each channel's own n_b)"""
    nblocks = -(-T // (64 * K))
    blob, offsets, words, starts = b"", [], [], []
    for p in payloads:
        offsets.append(len(blob))
        words.append((len(p) - 260 * nblocks) // 2)
        starts.append(R.block_starts(np.frombuffer(p, dtype="<u4", count=nblocks)))
        blob += p + b"\x00" * (-len(p) % 4)
    return blob, offsets, words, np.stack(starts)


def _decode(dev, payloads, T, freqs, lo, K):
    blob, offsets, words, start = _pack(payloads, T, K)
    out = _ops().latent_rans_decode(blob, T, len(freqs), lo, [len(f) for f in freqs], offsets, words, codec.cdf_table(freqs),
                                    start, K, dev)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (T, len(freqs))
    return out.cpu().numpy()


def _round_trip(dev, sym, freqs, lo, K):
    payloads = _encode(dev, sym, freqs, lo, K)
    want = (sym + np.asarray(lo, dtype=np.int64)[None, :]).astype(np.float32)
    assert np.array_equal(_decode(dev, payloads, sym.shape[0], freqs, lo, K), want)
    return [R.split_payload(p, sym.shape[0], K) for p in payloads]


# ---------------------------------------------------------------------------------------------------------- model edges
EDGE_CASES = R.model_edge_cases(codec.normalise_frequencies)


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_model_edges(dev, name):
    sym, freqs, lo, K = EDGE_CASES[name]
    T = sym.shape[0]
    parts = _round_trip(dev, sym, freqs, lo, K)
    n_b, _, words = parts[0]
    if name.startswith("dominant"):
        assert n_b.tolist() == [1, 0, 0, 1]                          # empty blocks between blocks that emit
    if name == "flat_65536":
        live = np.minimum(256, T - 256 * np.arange(n_b.size))
        assert n_b.tolist() == live.tolist() == [256, 256, 37] and words.size == T    # the slot buffer at capacity
    if name.startswith("lds"):
        assert [len(f) for f in freqs] == {"lds_4095": [4095], "lds_4096": [4096], "lds_4095_beside_4096": [4095, 4096]}[name]
    if name == "gauss":
        assert all(p[0][:2].min() > 0 and p[0][2] == 0 for p in parts)


def test_lds_and_global_cdf_code_the_same_symbols_alike(dev):
    """the same symbols under 4095 bins (cdf in LDS) and beside a 4096-bin channel (both searched in global memory)"""
    sym, freqs, lo, K = EDGE_CASES["lds_4095"]
    sym2, freqs2, lo2, _ = EDGE_CASES["lds_4095_beside_4096"]
    assert np.array_equal(sym2[:, 0], sym[:, 0]) and np.array_equal(freqs2[0], freqs[0])
    assert _encode(dev, sym, freqs, lo, K)[0] == _encode(dev, sym2, freqs2, lo2, K)[0]


# ------------------------------------------------------------------------------------------------------- geometry edges
@pytest.mark.parametrize("T", [1, 63, 64, 65, 128, 129])
def test_one_step_per_block(dev, T):
    sym = np.stack([R.known_answer_symbols(T), R.sparse_outliers(T, 0.1, T) ^ 1], axis=1)
    parts = _round_trip(dev, sym, [R.KNOWN_FREQ, np.array([1, 65535], dtype=np.uint32)], [-2, 9], 1)
    assert parts[0][0].size == -(-T // 64) and not parts[0][0].any()
    assert int(parts[1][0].sum()) == int((sym[:, 1] == 0).sum())     # only the f = 1 symbol emits on a state's first step


def test_most_steps_per_block(dev):
    """K = 65 536: two blocks, the second holds one symbol on lane 0; only the outliers of the (65535, 1) model emit."""
    K = 1 << 16
    T = 64 * K + 1
    sym = R.sparse_outliers(T, 1e-4, 3)[:, None]
    parts = _round_trip(dev, sym, [np.array([65535, 1], dtype=np.uint32)], [0], K)
    assert parts[0][0].tolist() == [int(sym.sum()), 0] and 300 < int(sym.sum()) < 550
    assert (parts[0][1][1, 1:] == R.X0).all()                        # the idle lanes of the last block keep 2^16


def _container(dev, x, steps):
    """device container == host container; every payload is the reference's; both decoders restore round(x)"""
    lat = torch.from_numpy(x)
    want = torch.round(lat)
    host = codec.compress_latents(lat, coder="rans", steps=steps)
    blob = codec.compress_latents(lat.to(dev), coder="rans", steps=steps)
    assert blob == host
    T, ld, K, chans = codec._parse_rans(blob)
    sym = np.rint(x).astype(np.int64)
    for c, ch in enumerate(chans):
        if ch["nbins"] > 1:
            size = 260 * -(-T // (64 * K)) + 2 * ch["words"]
            ref = R.encode_payload(sym[:, c] - ch["lo"], ch["freq"], K)
            assert blob[ch["payload_off"]:ch["payload_off"] + size] == ref, f"channel {c}"
    back = codec.decompress_latents(blob, dev)
    assert back.is_cuda and torch.equal(back.cpu(), want)
    assert torch.equal(codec.decompress_latents(blob, "cpu"), want)
    return chans


@pytest.mark.parametrize("T", [262_143, 262_144, 262_145])
def test_default_steps_around_one_block(dev, T):
    x = (np.random.default_rng(T).standard_normal((T, 2)) * (1.5, 0.2)).astype(np.float32)
    chans = _container(dev, x, None)
    assert chans[0]["n_b"].size == (1 if T <= 262_144 else 2)


# ------------------------------------------------------------------------------ the decoder refuses what it cannot decode
@pytest.fixture(scope="module")
def gauss(dev):
    """the Gaussian case as payloads and as a container (the container's model is the case's: same bytes); channel 1 is the
    one that gets corrupted, channel 0 stays intact in front of it"""
    sym, freqs, lo, K = EDGE_CASES["gauss"]
    T = sym.shape[0]
    payloads = [R.encode_payload(sym[:, c], freqs[c], K) for c in range(2)]
    blob = codec.compress_latents(_latent(sym, lo, "cpu"), coder="rans", steps=K)
    off = codec._parse_rans(blob)[3][1]["payload_off"]
    assert blob[off:off + len(payloads[1])] == payloads[1]
    want = (sym + np.asarray(lo)[None, :]).astype(np.float32)
    return dict(sym=sym, freqs=freqs, lo=lo, K=K, T=T, payloads=payloads, blob=blob, off=off, want=want)


def _with_payload(g, bad):
    return g["blob"][:g["off"]] + bad + g["blob"][g["off"] + len(bad):]


def test_corrupt_payloads_get_the_references_verdict(dev, gauss):
    g = gauss
    T, K, freqs, lo = g["T"], g["K"], g["freqs"], g["lo"]
    cases = R.payload_corruptions(g["payloads"][1], T, K)
    names = " ".join(n for n, _ in cases)
    assert len(cases) >= 25 and "word" in names and "below" in names and "state2." in names and "counts1<->2" in names
    refused = 0
    for name, bad in cases:
        assert len(bad) == len(g["payloads"][1]) and bad != g["payloads"][1], name
        sym1, ok = R.decode_payload(bad, freqs[1], T, K)
        container = _with_payload(g, bad)
        if ok:                                                       # the reference accepts it: so must the device, alike
            want = g["want"].copy()
            want[:, 1] = (sym1 + lo[1]).astype(np.float32)
            assert np.array_equal(_decode(dev, [g["payloads"][0], bad], T, freqs, lo, K), want), name
            assert np.array_equal(codec.decompress_latents(container, dev).cpu().numpy(), want), name
            continue
        refused += 1
        with pytest.raises(ValueError):
            _decode(dev, [g["payloads"][0], bad], T, freqs, lo, K)
            pytest.fail(f"{name}: the device decoded a payload the reference refuses")
        with pytest.raises(ValueError):
            codec.decompress_latents(container, dev)
            pytest.fail(f"{name}: the device decoded a container the reference refuses")
    print(f"{refused} of {len(cases)} corruptions refused by the reference and by the device")


def test_a_refusal_leaves_nothing_behind(dev, gauss):
    """the error word is per call: a well-formed decode right after a refusal returns the right table"""
    g = gauss
    bad = R.flip_state(g["payloads"][1], g["T"], g["K"], 2, 63, 16)  # an idle lane of the empty block: 2^16 -> 0
    assert not R.decode_payload(bad, g["freqs"][1], g["T"], g["K"])[1]
    for _ in range(2):
        with pytest.raises(ValueError):
            _decode(dev, [g["payloads"][0], bad], g["T"], g["freqs"], g["lo"], g["K"])
        assert np.array_equal(_decode(dev, g["payloads"], g["T"], g["freqs"], g["lo"], g["K"]), g["want"])
    with pytest.raises(ValueError):
        codec.decompress_latents(_with_payload(g, bad), dev)
    assert np.array_equal(codec.decompress_latents(g["blob"], dev).cpu().numpy(), g["want"])


def test_load_compressed_of_a_corrupt_payload_keeps_the_codebook(dev):
    from shacira_amd import harness
    torch.manual_seed(3)
    grid, _, _ = harness.kodak_like_grid(num_lods=6, max_grid_res=64)
    grid = grid.to(dev)
    with torch.no_grad():                                            # latents wide enough to need a payload
        grid.codebook.copy_(torch.randn(grid.codebook.shape, generator=torch.Generator().manual_seed(4)) * 2.5)
    blob = grid.compress(coder="rans")
    T, ld, K, chans = codec._parse_rans(blob)
    ch = chans[0]
    assert ch["nbins"] > 8 and ch["words"] > 0
    nblocks = -(-T // (64 * K))
    size = 260 * nblocks + 2 * ch["words"]
    payload = blob[ch["payload_off"]:ch["payload_off"] + size]
    want = torch.round(grid.codebook.detach()).clone()
    with torch.no_grad():
        grid.codebook.add_(0.25)
    before = grid.codebook.detach().clone()
    for bad in (R.flip_word(payload, T, K, ch["words"] // 2, 3), R.flip_state(payload, T, K, nblocks - 1, 0, 20)):
        assert not R.decode_payload(bad, ch["freq"], T, K)[1]
        with pytest.raises(ValueError):
            grid.load_compressed(blob[:ch["payload_off"]] + bad + blob[ch["payload_off"] + size:])
        assert torch.equal(grid.codebook.detach(), before)           # bit-identical: nothing was copied in
    grid.load_compressed(blob)
    assert torch.equal(grid.codebook.detach(), want)


# ------------------------------------------------------------------------------------------- containers at the limits
LIMIT_LATENTS = R.container_limit_latents()


@pytest.mark.parametrize("name", sorted(LIMIT_LATENTS))
def test_containers_at_the_limits(dev, name):
    chans = _container(dev, LIMIT_LATENTS[name], 4)
    if name == "permutation_65536":
        assert chans[0]["nbins"] == codec.RC_TOTAL and chans[0]["words"] == 65536 and (chans[0]["freq"] == 1).all()
    if name == "spike_in_zeros":
        assert chans[0]["freq"].tolist() == [65535, 0, 0, 1] and chans[0]["words"] == 1
        assert chans[0]["n_b"].size == 274 and int((chans[0]["n_b"] == 0).sum()) == 273
    if name == "sixteen_kinds":
        assert [ch["nbins"] for ch in chans[:6]] == [1, 2, 4, chans[3]["nbins"], 4095, 4096] and 8 < chans[3]["nbins"] < 30


def test_one_bin_too_many_is_refused(dev):
    wider = torch.arange(-7, 65530, dtype=torch.float32)[torch.randperm(65537, generator=torch.Generator().manual_seed(1))]
    with pytest.raises(ValueError):
        codec.compress_latents(wider[:, None].to(dev), coder="rans", steps=4)     # 65 537 consecutive integers


# ---------------------------------------------------------------------------------------------------- symbol statistics
def _counts(dev, x):
    """(lo, counts) of the kernels == np.unique of np.rint per channel, with every other bin 0"""
    lo, counts = _ops().latent_symbol_counts(torch.from_numpy(x).to(dev))
    lo, counts = lo.numpy(), counts.cpu().numpy()
    assert lo.dtype == np.int64 and counts.dtype == np.int64 and counts.shape[0] == x.shape[1]
    sym = np.rint(x.astype(np.float64)).astype(np.int64)
    assert counts.shape[1] == int((sym.max(axis=0) - sym.min(axis=0)).max()) + 1
    for c in range(x.shape[1]):
        vals, cnt = np.unique(sym[:, c], return_counts=True)
        assert lo[c] == vals[0]
        want = np.zeros(counts.shape[1], dtype=np.int64)
        want[vals - vals[0]] = cnt
        assert np.array_equal(counts[c], want), f"channel {c}"
    return lo, counts


@pytest.mark.parametrize("ld,span", [(3, 4096), (3, 4097), (1, 12288), (1, 12289), (16, 768), (16, 769)])
def test_histogram_on_the_lds_bin_boundary(dev, ld, span):
    """ld * nbins = 12 288 is the last size counted in LDS; one more bin per channel (12 291 at ld = 3, 12 289 -- a prime --
    at ld = 1 only, 12 304 at ld = 16) goes through global atomics. The widest channel spans exactly `span` values."""
    rng = np.random.default_rng(span)
    T = 9001
    wide = ld // 2
    x = np.empty((T, ld), dtype=np.float32)
    x[:, :] = rng.integers(40, 47, (T, ld))                          # narrow channels: seven bins, the rest 0
    x[:, 0] = 5.0                                                    # constant: one bin
    x[:, wide] = rng.integers(-1000, -1000 + span, T)
    x[[0, T - 1], wide] = (-1000, -1000 + span - 1)
    x += rng.uniform(-0.4, 0.4, x.shape).astype(np.float32)
    lo, counts = _counts(dev, x)
    assert counts.shape == (ld, span) and (ld * span <= 12288) == (span in (4096, 12288, 768))
    assert counts[wide, 0] > 0 and counts[wide, -1] > 0
    if ld > 1:
        assert counts[0, 0] == T and not counts[0, 1:].any() and not counts[ld - 1, 7:].any()


@pytest.mark.parametrize("rows,ld", [(1_398_101, 3), (1_398_102, 3), (838_861, 5)])
def test_histogram_past_the_workgroup_cap(dev, rows, ld):
    """rows * ld = 4 194 303 (2048 workgroups, uncapped), 4 194 306 (the first multiple of 3 past the cap of 2048 workgroups
    at 4 194 304 elements) and 4 194 305 = 5 * 838 861 exactly; the capped stride 524 288 is no multiple of 3 or 5"""
    rng = np.random.default_rng(rows)
    sym = rng.integers(0, 50, (rows, ld)) + np.arange(ld)[None, :] * 7 - 20
    sym[0], sym[-1] = np.arange(ld) * 7 - 20, np.arange(ld) * 7 + 29
    lo, counts = _ops().latent_symbol_counts(torch.from_numpy(sym.astype(np.float32)).to(dev))
    counts = counts.cpu().numpy()
    assert lo.tolist() == (np.arange(ld) * 7 - 20).tolist() and counts.shape == (ld, 50)
    for c in range(ld):
        assert np.array_equal(counts[c], np.bincount(sym[:, c] - int(lo[c]), minlength=50)), f"channel {c}"


def test_histogram_ties_signed_zero_and_the_clamp(dev):
    T = 777
    x = np.zeros((T, 4), dtype=np.float32)
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0, 3.5, -3.5, 0.49999997, -0.49999997, 0.50000006], dtype=np.float32)
    x[:, 0] = np.resize(ties, T)                                     # half to even: -4, -2, 0, 2, 4 and one 1
    x[:, 1] = -0.0
    x[:, 2] = 2.0 ** 30 - 64                                         # the largest fp32 below the clamp, alone: lo is exact
    x[:, 3] = -(2.0 ** 30 - 64)
    lo, counts = _counts(dev, x)
    assert lo.tolist() == [-4, 0, 2 ** 30 - 64, -(2 ** 30 - 64)] and counts.shape == (4, 9)
    assert counts[0, [1, 3, 7]].tolist() == [0, 0, 0] and counts[0, 5] == T // 12       # -3, -1 and 3 never; 1 once a period


def test_histogram_of_non_finite_values(dev):
    """at this layer only (codec refuses them earlier): NaN counts as 0, +-inf land on +-2^30"""
    T = 300
    x = np.zeros((T, 5), dtype=np.float32)
    x[:, 0] = np.nan                                                 # alone: lo must be 0
    x[:, 1] = np.inf
    x[:, 2] = -np.inf
    x[:, 3] = 3.0e9                                                  # finite, beyond the clamp
    x[:, 4] = -3.0e9
    lo, counts = _ops().latent_symbol_counts(torch.from_numpy(x).to(dev))
    assert lo.tolist() == [0, 2 ** 30, -(2 ** 30), 2 ** 30, -(2 ** 30)]
    assert counts.cpu().numpy().tolist() == [[T]] * 5
    y = np.zeros((T, 2), dtype=np.float32)                           # NaN among ordinary values joins the zeros
    y[:, 0] = np.resize(np.array([np.nan, 1.0, -2.0, 0.0, -np.nan], dtype=np.float32), T)
    y[:, 1] = np.resize(np.array([2.0, np.nan], dtype=np.float32), T)
    lo, counts = _ops().latent_symbol_counts(torch.from_numpy(y).to(dev))
    assert lo.tolist() == [-2, 0]
    assert counts.cpu().numpy().tolist() == [[T // 5, 0, 3 * T // 5, T // 5], [T // 2, 0, T // 2, 0]]
