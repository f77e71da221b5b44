"""Build check on the loss-scaled optimizer code objects (no GPU): the multi-tensor kernels of shacira_amd/csrc/adam.hip that
this file names -- loss-scaled Adam and the four RMSprop forms (momentum x scaled) -- are streaming kernels: everything in
registers (no private segment), no LDS, and at most 64 VGPRs, the 8 waves per SIMD an HBM-bound loop wants. The method of
tests/test_shade_build.py: the code objects' notes only."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shacira_amd", "lib", "libshacira_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("adam_multi_scaled_kernel", "rmsprop_multi_kernelILb0ELb0E", "rmsprop_multi_kernelILb0ELb1E",
           "rmsprop_multi_kernelILb1ELb0E", "rmsprop_multi_kernelILb1ELb1E")


def _metadata():
    """{kernel name: (private bytes, LDS bytes, vgprs)} of the gfx950 code objects."""
    if not os.path.exists(LIB):
        pytest.skip("libshacira_hip.so not built")
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    tmp = tempfile.mkdtemp(prefix="shacira_co_")
    try:
        shutil.copy(LIB, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = {}
        for co in glob.glob(os.path.join(tmp, "lib.so.*gfx950*")):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            # one kernel's fields are sorted by key: its LDS size stands before its .name, the rest behind it
            names = list(re.finditer(r"\.name:\s+(_Z\S+)", notes))
            for i, m in enumerate(names):
                before = notes[names[i - 1].end() if i else 0:m.start()]
                after = notes[m.end():names[i + 1].start() if i + 1 < len(names) else len(notes)]
                lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", before)
                priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", after)
                vgpr = re.search(r"\.vgpr_count:\s+(\d+)", after)
                if lds and priv and vgpr:
                    out[m.group(1)] = (int(priv.group(1)), int(lds[-1]), int(vgpr.group(1)))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_scaled_optimizer_kernels_use_no_scratch_no_lds_and_at_most_64_vgprs():
    meta = _metadata()
    every = [name for name in meta if re.search(r"adam_multi_scaled_|rmsprop_", name)]
    assert len(every) == len(KERNELS), every          # no loss-scaled or RMSprop kernel escapes the list
    for want in KERNELS:
        hits = [v for name, v in meta.items() if want in name]
        assert len(hits) == 1, f"{want}: {len(hits)} kernels in the code objects"
        private, lds, vgprs = hits[0]
        assert private == 0, f"{want}: {private} bytes of private segment ({vgprs} vgprs)"
        assert lds == 0, f"{want}: {lds} bytes of LDS"
        assert vgprs <= 64, f"{want}: {vgprs} vgprs: below 8 waves per SIMD"
