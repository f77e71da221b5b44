"""Build check on the structured-point-cloud code objects (no GPU), in the manner of tests/test_raygen_build.py: every
``depthcloud_`` / ``spc_`` kernel of shacira_amd/csrc/spc.hip is listed here, and none has a private (scratch) segment -- the
first-hit walk in particular is written with select chains, not indexed arrays. No VGPR limit is fixed; the counts are recorded
in profiles/spc.md."""
from test_raygen_build import _metadata

KERNELS = (
    "depthcloud_bounds_init_kernel", "depthcloud_bounds_kernel", "depthcloud_bounds_final_kernel",
    "depthcloud_points_kernelILb1ENS0_10BytePixels", "depthcloud_points_kernelILb0ENS0_10BytePixels",
    "depthcloud_points_kernelILb0ENS0_9SumPixels",
    "spc_mark_kernelINS0_11CloudSource", "spc_mark_kernelINS0_11DepthSourceINS0_10BytePixels",
    "spc_accumulate_kernelINS0_11CloudSource", "spc_accumulate_kernelINS0_11DepthSourceINS0_10BytePixels",
    "spc_accumulate_kernelINS0_11DepthSourceINS0_9SumPixels",
    "spc_popcount_kernel", "spc_resolve_kernel", "spc_first_hit_kernel",
)


def test_spc_kernels_are_listed_and_use_no_scratch():
    meta = _metadata()
    every = [name for name in meta if "depthcloud_" in name or "spc_" in name]
    assert len(every) == len(KERNELS), every          # no kernel escapes the list
    for want in KERNELS:
        hits = [v for name, v in meta.items() if want in name]
        assert len(hits) == 1, f"{want}: {len(hits)} kernels in the code objects"
        private, lds, vgprs = hits[0]
        assert private == 0, f"{want}: {private} bytes of private segment ({vgprs} vgprs)"
        assert lds <= 16, f"{want}: {lds} bytes of LDS (the compaction's four-entry prefix is the only use)"
