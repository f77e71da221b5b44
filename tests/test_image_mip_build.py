"""Build check on the mip-level code objects (no GPU): the block-sum kernels of shacira_amd/csrc/image_mip.hip -- the packed RGBA
form at every mip and load width, and the byte form -- and both forms of the ray kernel on sums (raygen.hip) keep everything in
registers: no private (scratch) segment and no LDS allocation (the cross-lane exchange of the shared-block forms needs none). The
ray kernel on sums stays at 8 waves per SIMD like the uint8 one. The method of tests/test_raygen_build.py: the code objects'
notes only."""
from test_raygen_build import _metadata

RGBA = [f"mip_rgba_kernelILi{mip}ELb{wide}E" for mip in (1, 2, 3, 4) for wide in (0, 1)]
RAYS = ["raysums_kernelILb0E", "raysums_kernelILb1E"]


def test_mip_kernels_use_no_scratch_and_no_lds():
    meta = _metadata()
    every = [name for name in meta if "mip_rgba_kernel" in name or "mip_bytes_kernel" in name or "raysums_kernel" in name]
    assert len(every) == len(RGBA) + len(RAYS) + 1, every          # no kernel of the two files escapes the lists
    for want in RGBA + RAYS + ["mip_bytes_kernel"]:
        hits = [v for name, v in meta.items() if want in name]
        assert len(hits) == 1, f"{want}: {len(hits)} kernels in the code objects"
        private, lds, vgprs = hits[0]
        assert private == 0, f"{want}: {private} bytes of private segment ({vgprs} vgprs)"
        assert lds == 0, f"{want}: {lds} bytes of LDS"
        if want in RAYS:
            assert vgprs <= 64, f"{want}: {vgprs} vgprs: below 8 waves per SIMD"
