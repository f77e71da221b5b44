"""Entropy-coded storage of a LatentGrid ("next" row f3 of SURVEY.md section 8).

The reference never writes a bitstream: LatentGrid.size (latent_grid.py:138-174) only *estimates* the size of the
rounded latents, or counts the bytes torchac would produce with the per-channel empirical distribution, and its
checkpoints are raw ``torch.save`` files (image_trainer.py:477-483). This module makes the size real:

  * symbols  = ``round(latent)`` per channel (``torch.round``, half to even) -- on the GPU the min/max and the
    histogram come from libshacira_hip.so (``shacira_latent_symbol_range/_histogram``), on the CPU from numpy;
  * model    = the empirical per-channel histogram, scaled to a total of 2^16 with every present symbol >= 1
    (stored in the container: 2 bytes per bin);
  * coder    = the library's static range coder (``shacira_rc_encode/_decode``, host side like the reference's use of
    torchac); ``decode(encode(x)) == round(x)`` exactly;
  * container = ``SHCR`` magic, JSON header, per channel: frequency table + payload;
  * ``coder="rans"`` (opt-in) = the 64-lane interleaved rANS of include/shacira_hip.h ("rans64", container version 2):
    same symbols and model, coded by HIP kernels for device tensors (no copy of the table leaves the GPU, only the
    bytes do) and by the library's host coder for CPU tensors -- the two write the same bytes, and either decodes the
    other's. ``decompress_latents`` picks the coder from the magic.

Byte counts are those of THIS coder (torchac is an un-pinned third-party dependency of the reference, so its exact
counts cannot be reproduced); they sit within a fraction of a percent of the entropy estimate that *is* pinned by
the golden vectors (``LatentGrid.size(use_torchac=False)``).
"""
import ctypes
import json
import struct

import numpy as np
import torch

from . import _lib

MAGIC = b"SHCR\x01\x00"
MAGIC_RANS = b"SHCR\x02\x00"       # version 2: "rans64" payloads, every section padded to a multiple of 4 bytes
RC_TOTAL = 1 << 16
RANS_STEPS = 4096                  # default steps per block: 262 144 symbols share one 260-byte flush
RANS_MAX_STEPS = 1 << 16
MAX_LATENT_DIM = 16


def normalise_frequencies(counts):
    """int counts [nbins] -> uint32 freq [nbins], sum == 65536, freq >= 1 wherever counts > 0 (deterministic)."""
    counts = np.asarray(counts, dtype=np.int64)
    present = counts > 0
    k = int(present.sum())
    if k == 0:
        raise ValueError("cannot build a model for an empty histogram")
    if k > RC_TOTAL:
        raise ValueError(f"{k} distinct symbols exceed the coder's 16-bit frequency scale")
    total = int(counts.sum())
    freq = np.zeros(counts.shape, dtype=np.int64)
    freq[present] = np.maximum(1, (counts[present] * RC_TOTAL) // total)
    diff = RC_TOTAL - int(freq.sum())
    if diff != 0:
        # give / take the remainder to / from the most frequent symbols (largest first, stable order)
        order = np.argsort(-counts, kind="stable")
        i = 0
        while diff != 0:
            j = order[i % len(order)]
            if diff > 0:
                freq[j] += 1
                diff -= 1
            elif freq[j] > 1:
                freq[j] -= 1
                diff += 1
            i += 1
    assert int(freq.sum()) == RC_TOTAL and np.all(freq[present] >= 1)
    return freq.astype(np.uint32)


def rc_encode(symbols, freq):
    """symbols: int32 indices into ``freq``; returns the coded bytes."""
    symbols = np.ascontiguousarray(symbols, dtype=np.int32)
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    L = _lib.lib()
    cap = L.shacira_rc_encode_bound(symbols.size)
    out = np.empty(cap, dtype=np.uint8)
    n_out = ctypes.c_size_t(0)
    _lib.check(L.shacira_rc_encode(symbols.ctypes.data_as(ctypes.c_void_p), symbols.size,
                                   freq.ctypes.data_as(ctypes.c_void_p), freq.size,
                                   out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n_out)), "shacira_rc_encode")
    return out[:n_out.value].tobytes()


def rc_decode(data, freq, n):
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(n, dtype=np.int32)
    _lib.check(_lib.lib().shacira_rc_decode(buf.ctypes.data_as(ctypes.c_void_p) if buf.size else None, buf.size,
                                            freq.ctypes.data_as(ctypes.c_void_p), freq.size, n,
                                            out.ctypes.data_as(ctypes.c_void_p)), "shacira_rc_decode")
    return out


def symbol_counts(latent):
    """(lo [ld] int64 numpy, counts [ld, nbins] int64 numpy) of round(latent); HIP kernels for device tensors."""
    if latent.is_cuda:
        from . import hip_ops
        lo, counts = hip_ops.latent_symbol_counts(latent.float())
        return lo.numpy(), counts.cpu().numpy()
    sym = torch.round(latent.detach().float()).long().numpy()
    if sym.shape[0] == 0:
        return np.zeros(sym.shape[1], np.int64), np.zeros((sym.shape[1], 1), np.int64)
    lo = sym.min(axis=0)
    nbins = int((sym.max(axis=0) - lo).max()) + 1
    counts = np.stack([np.bincount(sym[:, c] - lo[c], minlength=nbins) for c in range(sym.shape[1])])
    return lo.astype(np.int64), counts.astype(np.int64)


def entropy_bits(counts):
    """Reference estimate (latent_grid.py:150-152) from a histogram: sum clamp(-log2(p + 1e-10), 0, 1000) * count,
    evaluated in fp32 like the reference."""
    c = torch.as_tensor(np.asarray(counts)[np.asarray(counts) > 0])
    probs = c / torch.sum(c)
    bits = torch.clamp(-1.0 * torch.log(probs + 1e-10) / np.log(2.0), 0, 1000)
    return torch.sum(bits * c).item()


def rans_encode(symbols, freq, steps=RANS_STEPS):
    """symbols: int32 indices into ``freq`` (at least two bins) -> rans64 channel payload (host coder)."""
    symbols = np.ascontiguousarray(symbols, dtype=np.int32)
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    L = _lib.lib()
    cap = max(int(L.shacira_rans_encode_bound(symbols.size, steps)), 1)
    out = np.empty(cap, dtype=np.uint8)
    n_out = ctypes.c_size_t(0)
    _lib.check(L.shacira_rans_encode(symbols.ctypes.data_as(ctypes.c_void_p), symbols.size,
                                     freq.ctypes.data_as(ctypes.c_void_p), freq.size, steps,
                                     out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n_out)), "shacira_rans_encode")
    return out[:n_out.value].tobytes()


def rans_decode(data, freq, n, steps=RANS_STEPS):
    """Inverse of rans_encode (host coder). ValueError when the bytes are not a valid payload of n symbols."""
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(n, dtype=np.int32)
    rc = _lib.lib().shacira_rans_decode(buf.ctypes.data_as(ctypes.c_void_p) if buf.size else None, buf.size,
                                        freq.ctypes.data_as(ctypes.c_void_p), freq.size, n, steps,
                                        out.ctypes.data_as(ctypes.c_void_p))
    if rc == _lib.EINVAL:
        raise ValueError("corrupt rans64 payload (counts, states or words do not fit the model and the length)")
    _lib.check(rc, "shacira_rans_decode")
    return out


def cdf_table(freqs):
    """per-channel frequency tables -> uint32 [ld, max nbins + 1] of cumulative frequencies, as the kernels read them
    (row c: cdf[0 .. nbins_c], 65536 beyond)."""
    cdf = np.full((len(freqs), max(len(f) for f in freqs) + 1), RC_TOTAL, dtype=np.uint32)
    for c, f in enumerate(freqs):
        cdf[c, 0] = 0
        cdf[c, 1:len(f) + 1] = np.cumsum(f)
    return cdf


def _pad4(blob):
    return blob + b"\x00" * (-len(blob) % 4)


def _check_latents(latent):
    T, ld = latent.shape
    if not bool(torch.isfinite(latent).all()):
        raise ValueError("latents must be finite to be entropy coded")
    if T and float(latent.detach().abs().max()) >= 2.0 ** 30:
        raise ValueError("latents beyond +-2^30 are outside the coder's symbol range")
    return int(T), int(ld)


def _compress_rans(latent, steps):
    steps = RANS_STEPS if steps is None else int(steps)
    if not 1 <= steps <= RANS_MAX_STEPS:
        raise ValueError(f"steps must be in [1, {RANS_MAX_STEPS}], got {steps}")
    T, ld = _check_latents(latent)
    if not 1 <= ld <= MAX_LATENT_DIM:
        raise ValueError(f"latent_dim must be in [1, {MAX_LATENT_DIM}], got {ld}")
    header = {"coder": "rans64", "rows": T, "latent_dim": ld, "steps": steps, "channels": []}
    tables, payloads = [], []
    if T:
        lo, counts = symbol_counts(latent)
        nbins = [int(np.nonzero(counts[c])[0].max()) + 1 for c in range(ld)]
        if max(nbins) > RC_TOTAL:
            raise ValueError(f"a channel spans {max(nbins)} integer values; the rans64 model holds at most {RC_TOTAL} bins")
        freqs = [normalise_frequencies(counts[c, :nbins[c]]) for c in range(ld)]
        tables = [(f % RC_TOTAL).astype("<u2").tobytes() for f in freqs]   # a single bin's 65536 is stored as 0
        if latent.is_cuda:
            from . import hip_ops
            payloads = hip_ops.latent_rans_encode(latent.float(), lo, nbins, cdf_table(freqs), steps)
        else:
            sym = torch.round(latent.detach().float()).to(torch.int64).numpy()
            payloads = [rans_encode((sym[:, c] - lo[c]).astype(np.int32), freqs[c], steps) if nbins[c] > 1 else b""
                        for c in range(ld)]
        nblocks = -(-T // (64 * steps))
        for c in range(ld):
            words = (len(payloads[c]) - 260 * nblocks) // 2 if nbins[c] > 1 else 0
            header["channels"].append({"lo": int(lo[c]), "nbins": nbins[c], "words": words})
    else:
        header["channels"] = [{"lo": 0, "nbins": 0, "words": 0} for _ in range(ld)]
    hj = json.dumps(header, separators=(",", ":")).encode()
    parts = [_pad4(MAGIC_RANS + struct.pack("<I", len(hj)) + hj)]
    for table, payload in zip(tables, payloads):
        parts += [_pad4(table), _pad4(payload)]
    return b"".join(parts)


def compress_latents(latent, coder="range", steps=None):
    """[T, ld] float latents -> container bytes holding round(latent) exactly.

    ``coder="range"`` (default): the host range coder, container version 1. ``coder="rans"``: the 64-lane interleaved
    rANS, container version 2 -- HIP kernels for device tensors, the host coder for CPU tensors, the same bytes from both;
    ``steps`` = steps per block (default 4096; stored in the header). rANS limits: latent_dim <= 16 and at most 65536
    integer values between a channel's smallest and largest symbol."""
    if coder == "rans":
        return _compress_rans(latent, steps)
    if coder != "range":
        raise ValueError(f"unknown coder {coder!r} (expected 'range' or 'rans')")
    if steps is not None:
        raise ValueError("steps applies to coder='rans' only")
    T, ld = _check_latents(latent)
    lo, counts = symbol_counts(latent)
    sym = torch.round(latent.detach().float()).to(torch.int64).cpu().numpy()
    header = {"rows": int(T), "latent_dim": int(ld), "channels": []}
    blobs = []
    for c in range(ld):
        if T == 0:
            header["channels"].append({"lo": 0, "nbins": 0, "payload": 0})
            continue
        hi_bin = int(np.nonzero(counts[c])[0].max()) + 1
        freq = normalise_frequencies(counts[c, :hi_bin])
        payload = rc_encode((sym[:, c] - lo[c]).astype(np.int32), freq)
        # 2 bytes per bin; only a single-bin channel has freq 65536, stored as 0 (bin 0 and the last bin are present)
        table = (freq % RC_TOTAL).astype("<u2").tobytes()
        header["channels"].append({"lo": int(lo[c]), "nbins": hi_bin, "payload": len(payload)})
        blobs += [table, payload]
    hj = json.dumps(header, separators=(",", ":")).encode()
    return MAGIC + struct.pack("<I", len(hj)) + hj + b"".join(blobs)


def _read_header(data):
    """(header dict, offset of the first byte after it) of either container version; ValueError if there is none."""
    if len(data) < len(MAGIC) + 4 or data[:len(MAGIC)] not in (MAGIC, MAGIC_RANS):
        raise ValueError("not a SHCR container")
    (hl,) = struct.unpack_from("<I", data, len(MAGIC))
    off = len(MAGIC) + 4
    if off + hl > len(data):
        raise ValueError("truncated SHCR container (header)")
    try:
        header = json.loads(bytes(data[off:off + hl]).decode())
    except (UnicodeDecodeError, json.JSONDecodeError) as exc:
        raise ValueError("corrupt SHCR header") from exc
    return header, off + hl


def container_shape(data):
    """(rows, latent_dim) a container of either version declares, read from its header alone."""
    header, _ = _read_header(data)
    try:
        return int(header["rows"]), int(header["latent_dim"])
    except (KeyError, TypeError) as exc:
        raise ValueError("corrupt SHCR header") from exc


def _parse_rans(data):
    """Check a version-2 container against its own size: everything the decoders index is inside `data` afterwards.
    -> (T, ld, steps, channels) with channels = [{lo, nbins, words, freq, payload_off, n_b}]."""
    header, off = _read_header(data)
    off += -off % 4
    try:
        T, ld, steps, chans = int(header["rows"]), int(header["latent_dim"]), int(header["steps"]), header["channels"]
        if header["coder"] != "rans64":
            raise ValueError(f"unknown coder {header['coder']!r} in a version-2 SHCR container")
        chans = [{"lo": int(ch["lo"]), "nbins": int(ch["nbins"]), "words": int(ch["words"])} for ch in chans]
    except (KeyError, TypeError) as exc:
        raise ValueError("corrupt SHCR header") from exc
    if T < 0 or not 1 <= ld <= MAX_LATENT_DIM or not 1 <= steps <= RANS_MAX_STEPS or len(chans) != ld:
        raise ValueError("corrupt SHCR header (rows, latent_dim, steps or channel count)")
    nblocks = -(-T // (64 * steps))
    for ch in chans:
        if T == 0:
            continue
        nb, words = ch["nbins"], ch["words"]
        if not 1 <= nb <= RC_TOTAL or not 0 <= words <= T or abs(ch["lo"]) > 2 ** 30:
            raise ValueError("corrupt SHCR header (channel)")
        if off + 2 * nb > len(data):
            raise ValueError("truncated SHCR container (frequency table)")
        freq = np.frombuffer(data, dtype="<u2", count=nb, offset=off).astype(np.uint32)
        off += 2 * nb + (-2 * nb) % 4
        if nb == 1:
            freq = np.array([RC_TOTAL], dtype=np.uint32)
            if words:
                raise ValueError("corrupt SHCR header (a single-bin channel has no payload)")
        if int(freq.sum()) != RC_TOTAL:
            raise ValueError("corrupt frequency table")
        ch["freq"], ch["payload_off"], ch["n_b"] = freq, off, np.zeros(0, np.int64)
        if nb > 1:
            size = 260 * nblocks + 2 * words
            if off + size > len(data):
                raise ValueError("truncated SHCR container (payload)")
            ch["n_b"] = np.frombuffer(data, dtype="<u4", count=nblocks, offset=off).astype(np.int64)
            if int(ch["n_b"].sum()) != words:
                raise ValueError("corrupt rans64 payload: the block counts do not add up to the channel's words")
            off += size + (-size) % 4
    return T, ld, steps, chans


def _decompress_rans(data, device):
    T, ld, steps, chans = _parse_rans(data)
    device = torch.device(device)
    if T == 0:
        return torch.zeros((0, ld), dtype=torch.float32, device=device)
    nblocks = -(-T // (64 * steps))
    if device.type == "cuda":
        from . import hip_ops
        nbins = [ch["nbins"] for ch in chans]
        start = np.zeros((ld, nblocks), dtype=np.int64)
        for c, ch in enumerate(chans):
            if nbins[c] > 1:
                start[c] = np.cumsum(ch["n_b"]) - ch["n_b"]
        return hip_ops.latent_rans_decode(data, T, ld, [ch["lo"] for ch in chans], nbins,
                                          [ch["payload_off"] for ch in chans], [ch["words"] for ch in chans],
                                          cdf_table([ch["freq"] for ch in chans]), start, steps, device)
    out = np.zeros((T, ld), dtype=np.float32)
    for c, ch in enumerate(chans):
        if ch["nbins"] > 1:
            size = 260 * nblocks + 2 * ch["words"]
            sym = rans_decode(data[ch["payload_off"]:ch["payload_off"] + size], ch["freq"], T, steps)
            out[:, c] = sym.astype(np.float32)
        out[:, c] += np.float32(ch["lo"])
    return torch.from_numpy(out).to(device)


def decompress_latents(data, device="cpu"):
    """Inverse of compress_latents: fp32 [T, ld] tensor of the rounded latents. The magic selects the coder; a version-2
    ("rans64") container decodes on the GPU when `device` is one (the container's bytes and its parsed tables are
    uploaded, never the symbols) and with the host coder otherwise. Malformed containers raise ValueError."""
    if data[:len(MAGIC_RANS)] == MAGIC_RANS:
        return _decompress_rans(data, device)
    if data[:len(MAGIC)] != MAGIC:
        raise ValueError("not a SHCR container")
    (hl,) = struct.unpack_from("<I", data, len(MAGIC))
    off = len(MAGIC) + 4
    header = json.loads(data[off:off + hl].decode())
    off += hl
    T, ld = header["rows"], header["latent_dim"]
    out = np.zeros((T, ld), dtype=np.float32)
    for c, ch in enumerate(header["channels"]):
        if T == 0:
            continue
        nb = ch["nbins"]
        freq = np.frombuffer(data, dtype="<u2", count=nb, offset=off).astype(np.uint32)
        off += 2 * nb
        if nb == 1:                       # one symbol only: its frequency 65536 is stored as 0
            freq = np.array([RC_TOTAL], dtype=np.uint32)
        if int(freq.sum()) != RC_TOTAL:
            raise ValueError("corrupt frequency table")
        payload = data[off:off + ch["payload"]]
        off += ch["payload"]
        out[:, c] = rc_decode(payload, freq, T).astype(np.float32) + np.float32(ch["lo"])
    return torch.from_numpy(out).to(device)


def payload_bits(data):
    """Bits of the entropy-coded payloads only (what torchac's byte_stream length measures in the reference): not the
    header, the frequency tables or padding. For a version-2 ("rans64") container the flush IS counted -- each block's
    word count and 64 final states, 260 bytes -- because the decoder cannot start without it."""
    header, _ = _read_header(data)
    if data[:len(MAGIC_RANS)] == MAGIC_RANS:
        nblocks = -(-int(header["rows"]) // (64 * int(header["steps"])))
        return 8 * sum(260 * nblocks + 2 * ch["words"] for ch in header["channels"] if ch["nbins"] > 1)
    return 8 * sum(ch["payload"] for ch in header["channels"])


# ------------------------------------------------------------------------------------------------- whole-model files
MODEL_MAGIC = b"SHCM\x01\x00"


def save_model(module, path=None, latent_key_suffix="grid.codebook", coder="range"):
    """Serialise a neural field that owns a LatentGrid: the latent table goes through `compress_latents` (entropy
    coded with `coder`, restores round(latent)); every other entry of the state dict is stored raw (fp32 / int as is).
    Returns the bytes (and writes them to `path` when given). The reference only ever `torch.save`s the fp32 state
    (image_trainer.py:477-483), so its reported sizes are estimates; this file IS the size."""
    state = module.state_dict()
    entries, blobs, off = [], [], 0
    for name, t in state.items():
        if name.endswith(latent_key_suffix) and t.dim() == 2 and t.is_floating_point():
            blob, kind = compress_latents(t, coder=coder), "latents"
            meta = {"shape": list(t.shape)}
        else:
            arr = t.detach().cpu().contiguous().numpy()
            blob, kind = arr.tobytes(), "raw"
            meta = {"shape": list(arr.shape), "dtype": str(arr.dtype)}
        entries.append({"name": name, "kind": kind, "offset": off, "nbytes": len(blob), **meta})
        blobs.append(blob)
        off += len(blob)
    hj = json.dumps({"entries": entries}, separators=(",", ":")).encode()
    data = MODEL_MAGIC + struct.pack("<I", len(hj)) + hj + b"".join(blobs)
    if path is not None:
        with open(path, "wb") as fh:
            fh.write(data)
    return data


def load_model(module, data):
    """Inverse of save_model (`data`: bytes or a path). Parameters are overwritten in place; the latent table receives
    the stored integers, i.e. exactly what the decoder sees at validation time (round(latent))."""
    if isinstance(data, (str, bytes)) and not isinstance(data, bytes):
        with open(data, "rb") as fh:
            data = fh.read()
    if data[:len(MODEL_MAGIC)] != MODEL_MAGIC:
        raise ValueError("not a SHCM model file")
    (hl,) = struct.unpack_from("<I", data, len(MODEL_MAGIC))
    base = len(MODEL_MAGIC) + 4 + hl
    header = json.loads(data[len(MODEL_MAGIC) + 4:base].decode())
    state = module.state_dict()
    seen = set()
    with torch.no_grad():
        for e in header["entries"]:
            if e["name"] not in state:
                raise KeyError(f"file entry {e['name']} has no counterpart in the module")
            dst = state[e["name"]]
            blob = data[base + e["offset"]:base + e["offset"] + e["nbytes"]]
            if e["kind"] == "latents":
                val = decompress_latents(blob, device=dst.device)
            else:
                val = torch.from_numpy(np.frombuffer(blob, dtype=np.dtype(e["dtype"])).reshape(e["shape"]).copy())
            if tuple(val.shape) != tuple(dst.shape):
                raise ValueError(f"{e['name']}: file holds {tuple(val.shape)}, module {tuple(dst.shape)}")
            dst.copy_(val.to(dst.device).to(dst.dtype))
            seen.add(e["name"])
    missing = [k for k in state if k not in seen]
    if missing:
        raise KeyError(f"module entries missing from the file: {missing[:5]}")
    return module
