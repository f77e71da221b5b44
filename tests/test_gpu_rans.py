"""The "rans64" kernels of symbols.hip on the MI355X: device containers equal host containers byte for byte, and the device
decoder restores round(latent) bit for bit -- from containers written by either side. The host coder is held to the numpy
reference by tests/test_rans_cpu.py. Only well-formed payloads reach the device decoder here; corrupt ones, hand-built models
and the format's limits are in tests/test_gpu_rans_edges.py."""
import struct

import numpy as np
import pytest
import torch

from shacira_amd import codec

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _gauss(T, ld, scale=2.0, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * T + ld)
    lat = torch.randn((T, ld), generator=g) * scale
    if T > 10:
        ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -0.0])
        lat[3:3 + ties.numel(), 0] = ties
    return lat


def _check(lat, steps=None):
    """device bytes == host bytes; all four (writer, reader) pairs restore round(lat)"""
    want = torch.round(lat)
    host = codec.compress_latents(lat, coder="rans", steps=steps)
    dev = codec.compress_latents(lat.to(DEV), coder="rans", steps=steps)
    assert dev == host
    back = codec.decompress_latents(host, DEV)                       # written by the host, decoded by the kernels
    assert back.is_cuda and back.dtype == torch.float32 and tuple(back.shape) == tuple(lat.shape)
    assert torch.equal(back.cpu(), want)
    assert torch.equal(codec.decompress_latents(dev, "cpu"), want)   # and the reverse
    return host


@pytest.mark.parametrize("ld", [1, 3, 16])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_lane_masks_and_partial_blocks(T, ld):
    _check(_gauss(T, ld), steps=4)                                   # T == 1: every channel is a single bin


def test_second_known_answer_has_an_empty_block():
    """T = 130, K = 2 under the issue's model: block 1 holds two symbols and emits no word (n_b = [7, 0])."""
    import zlib
    import rans_ref as R
    sym = R.known_answer_symbols(130)
    # the container codes under the table's empirical model, not KNOWN_FREQ: the CRC is the reference's under that model
    lat = sym.astype(np.float32)[:, None]
    blob = _check(torch.from_numpy(lat), steps=2)
    T, ld, steps, chans = codec._parse_rans(blob)
    assert chans[0]["n_b"].shape == (2,) and int(chans[0]["n_b"][1]) == 0
    size = 260 * 2 + 2 * chans[0]["words"]
    payload = blob[chans[0]["payload_off"]:chans[0]["payload_off"] + size]
    assert zlib.crc32(payload) == zlib.crc32(R.encode_payload(sym, chans[0]["freq"], 2))


def test_default_steps_two_blocks():
    _check(_gauss(300_000, 2, scale=1.5))


def test_single_bin_channel_between_ordinary_ones():
    lat = _gauss(3000, 3)
    lat[:, 1] = 7.0
    blob = _check(lat, steps=4)
    _, _, _, chans = codec._parse_rans(blob)
    assert chans[1]["nbins"] == 1 and chans[1]["words"] == 0
    lat[:, :] = -2.0                                                 # every channel constant: nothing but tables
    _check(lat, steps=4)


def test_wide_alphabet_searches_the_cdf_in_global_memory():
    g = torch.Generator().manual_seed(3)
    lat = torch.randint(0, 20_000, (30_000, 1), generator=g).float()
    blob = _check(lat, steps=64)
    _, _, _, chans = codec._parse_rans(blob)
    assert chans[0]["nbins"] > 16_384
    lat2 = torch.cat([lat, _gauss(30_000, 1)], dim=1)                # a narrow channel beside the wide one
    _check(lat2, steps=64)


def test_empty_table():
    lat = torch.zeros((0, 2))
    blob = _check(lat)
    assert tuple(codec.decompress_latents(blob, DEV).shape) == (0, 2)


def test_input_forms():
    base = _gauss(2000, 4).to(DEV)
    want = codec.compress_latents(base.cpu()[:, 1:3].contiguous(), coder="rans", steps=4)
    view = base[:, 1:3]                                              # non-contiguous view
    assert not view.is_contiguous()
    assert codec.compress_latents(view, coder="rans", steps=4) == want
    param = torch.nn.Parameter(view.clone(), requires_grad=True)
    assert codec.compress_latents(param, coder="rans", steps=4) == want
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blob = codec.compress_latents(view, coder="rans", steps=4)
        back = codec.decompress_latents(blob, DEV)
    side.synchronize()
    assert blob == want and torch.equal(back, torch.round(view))


def test_latent_grid_compress_and_load_on_the_device():
    from shacira_amd import harness
    torch.manual_seed(3)
    grid, _, _ = harness.kodak_like_grid(num_lods=6, max_grid_res=64)
    grid = grid.to(DEV)
    with torch.no_grad():
        grid.codebook.mul_(2.5)
    want = torch.round(grid.codebook.detach()).clone()
    blob = grid.compress(coder="rans")
    assert blob[:6] == b"SHCR\x02\x00" and blob == codec.compress_latents(grid.codebook.detach().cpu(), coder="rans")
    with torch.no_grad():
        grid.codebook.add_(0.25)
    grid.load_compressed(blob)
    assert grid.codebook.is_cuda and torch.equal(grid.codebook.detach(), want)
    old = grid.compress()                                            # a version-1 container still loads
    grid.load_compressed(old)
    assert torch.equal(grid.codebook.detach(), want)


def test_header_level_rejections_launch_nothing():
    from shacira_amd import harness
    lat = _gauss(1000, 1)
    blob = bytearray(codec.compress_latents(lat, coder="rans", steps=4))
    _, _, _, chans = codec._parse_rans(bytes(blob))
    with pytest.raises(ValueError):
        codec.decompress_latents(b"SHCR\x03\x00" + bytes(blob[6:]), DEV)          # bad magic
    with pytest.raises(ValueError):
        codec.decompress_latents(bytes(blob[:len(blob) - 8]), DEV)                # truncated
    bad = bytearray(blob)
    off = chans[0]["payload_off"]
    struct.pack_into("<I", bad, off, struct.unpack_from("<I", bad, off)[0] + 1)   # count sum != words
    with pytest.raises(ValueError):
        codec.decompress_latents(bytes(bad), DEV)
    torch.manual_seed(3)
    grid, _, _ = harness.kodak_like_grid(num_lods=6, max_grid_res=64)
    grid = grid.to(DEV)
    before = grid.codebook.detach().clone()
    with pytest.raises(ValueError):
        grid.load_compressed(bytes(blob))                                         # shape mismatch with the grid
    assert torch.equal(grid.codebook.detach(), before)
