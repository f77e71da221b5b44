"""The C-ABI library loads and exports every symbol include/shacira_hip.h declares; argument validation returns the
documented codes WITHOUT touching a GPU (validation precedes any HIP call). No compute here."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from shacira_amd import _lib

HEADER = os.path.join(ROOT, "include", "shacira_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"SHACIRA_API[^;(]*?\b(shacira_\w+)\s*\(", text)))


def test_header_and_binding_list_the_same_symbols():
    syms = declared_symbols()
    assert len(syms) >= 20
    assert sorted(_lib.SIGNATURES.keys()) == syms


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "build with `make -C shacira_amd/csrc` (or __graft_entry__.build())"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(handle, name), name
    assert _lib.lib().shacira_abi_version() == 11


def test_argument_validation_codes():
    L = _lib.lib()
    res = (ctypes.c_int32 * 2)(16, 32)
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first or N == 0
    fwd = L.shacira_hashgrid_forward
    assert fwd(4, 0, 2, 2, 8, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EINVAL     # dim
    assert fwd(2, 0, 0, 2, 8, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EINVAL     # num_lods
    assert fwd(2, 0, 33, 2, 8, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EINVAL    # > SHACIRA_MAX_LODS
    assert fwd(2, 0, 2, 3, 8, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EODD       # odd feature dim
    assert fwd(2, 0, 2, 2, 31, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EINVAL    # bitwidth
    assert fwd(2, 0, 2, 2, 8, res, one, 10, one, one, 7, one, None, 0, None) == _lib.EDTYPE     # dtype
    assert fwd(2, -1, 2, 2, 8, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EINVAL    # negative N
    assert fwd(2, 0, 2, 2, 8, res, one, 10, one, one, 0, one, None, 0, None) == 0               # N == 0: nothing to do
    assert fwd(2, 5, 2, 2, 8, res, None, 10, one, one, 0, one, None, 0, None) == _lib.EINVAL    # null pointer
    assert fwd(2, 5, 2, 2, 8, res, one, 10, one, one, 0, one, None, 0, None) == _lib.EWORKSPACE # workspace missing
    assert L.shacira_hashgrid_forward_workspace_bytes(2, 5, 2, 2, 8, res, 10, 0) >= 5 * 2 * 2 * 4
    assert L.shacira_latent_decode_forward(0, 5, 2, one, one, one, None, None, 0.0, one, None) == _lib.EDTYPE
    assert L.shacira_latent_decode_forward(0, 2, 2, one, one, one, None, None, 0.0, one, None) == 0
    assert L.shacira_entropy_bits_forward(0, 2, 5, one, None, one, one, one, 1 << 20, None) == _lib.EINVAL
    assert L.shacira_entropy_bits_forward(0, 2, 2, one, None, one, one, one, 16, None) == _lib.EWORKSPACE
    assert L.shacira_hashgrid_backward_workspace_bytes(3, 1000, 2, 2, 8, res, 100, 1) >= 100 * 2 * 4   # fp16: fp32 image
    assert L.shacira_hashgrid_backward_workspace_bytes(3, 0, 2, 2, 8, res, 100, 0) == 0
    assert b"multiple of 2" in L.shacira_strerror(_lib.EODD)
    assert L.shacira_set_option(b"nope", 1) == _lib.EINVAL
    # pruned in ABI 7 (round 3): the lost code paths' switches are gone, and forward variants 1, 2, 4, 5, 7 are refused
    for name in (b"bwd_rows", b"bwd_groups", b"bwd_direct_side", b"bwd_fuse"):
        assert L.shacira_set_option(name, 1) == _lib.EINVAL
    for v in (1, 2, 4, 5, 7, 10):
        assert L.shacira_set_option(b"fwd_variant", v) == _lib.EINVAL
    assert L.shacira_set_option(b"bin_acc_kib", 96) == _lib.EINVAL
    for v in (0, 3, 6, 8, 9, -1):
        assert L.shacira_set_option(b"fwd_variant", v) == 0 and L.shacira_get_option(b"fwd_variant") == v
    with pytest.raises(Exception, match="multiple of 2"):
        _lib.check(_lib.EODD)
    with pytest.raises(RuntimeError):
        _lib.check(_lib.EINVAL, "x")


def test_latent_mlp_entry_points_validate_their_arguments():
    """shacira_latent_mlp_*: shape limits and NULL operands are refused before anything is launched (no GPU needed)."""
    import ctypes
    lib = _lib.lib()
    arr = lambda *w: (ctypes.c_int32 * len(w))(*w)
    assert lib.shacira_latent_mlp_supported(2, arr(2, 8, 2)) == 1
    assert lib.shacira_latent_mlp_supported(4, arr(1, 16, 16, 16, 4)) == 1
    assert lib.shacira_latent_mlp_supported(5, arr(1, 2, 2, 2, 2, 2)) == 0          # too deep
    assert lib.shacira_latent_mlp_supported(1, arr(2, 17)) == 0                      # too wide
    assert lib.shacira_latent_mlp_supported(1, arr(0, 2)) == 0
    assert lib.shacira_latent_mlp_backward_workspace_bytes(2, arr(2, 8, 2)) == 512 * (2 * 8 + 8 + 8 * 2 + 2) * 8
    einval = -1
    rc = lib.shacira_latent_mlp_forward(10, 5, arr(1, 2, 2, 2, 2, 2), None, None, 1.0, 0, None, None, 0, 0, 0.0, None, None)
    assert rc != 0
    rc = lib.shacira_latent_mlp_forward(10, 1, arr(2, 2), None, None, 1.0, 0, None, None, 0, 0, 0.0, None, None)
    assert rc != 0                                                                   # NULL div / params
    rc = lib.shacira_latent_mlp_forward(10, 1, arr(2, 2), None, None, 1.0, 0, None, None, 9, 0, 0.0, None, None)
    assert rc != 0                                                                   # unknown activation


def test_backward_workspace_is_sized_by_the_selected_path():
    """A table whose levels all fit LDS images (the Kodak tables of configs B / C, kodak.yaml) stages no transposed gradients
    and writes no items: its backward workspace is control words only, whatever the batch (round 3 asked 1.21 GB for config C).
    The NeRF table's workspace is the staged gradients + the item slots its levels can emit."""
    from conftest import CONFIGS, geo, table_layout
    L = _lib.lib()

    def query(dim, res, bw, n, F=2, dtype=_lib.F32):
        _, _, T = table_layout(res, bw, dim)
        arr = (ctypes.c_int32 * len(res))(*res)
        return L.shacira_hashgrid_backward_workspace_bytes(dim, n, len(res), F, bw, arr, T, dtype)

    dim, res, bw = CONFIGS["B"]
    assert query(dim, res, bw, 393_216) < (1 << 20)                 # config B
    assert query(dim, res, bw, 24 * 393_216) < (1 << 20)            # config C: 9.4 M samples
    assert query(2, geo(16, 512, 24), 11, 393_216) < (1 << 20)      # kodak.yaml's 24 levels
    dim, res, bw = CONFIGS["D"]
    n = 1 << 20
    s1 = query(dim, res, bw, n)
    staged = n * 16 * 2 * 4                                         # gT [L][N][F] fp32
    # round 5: runs are reserved in whole 64-byte pieces = multiples of 4 item units: at most 3 pad units per (1 024-sample
    # tile, bucket): 1 024 tiles x 733 buckets
    slots = n * (5 * 2 + 11 * 4) * 16                               # 5 compact levels (2 slots), 11 hashed (4 pair items)
    pads = 1024 * 733 * 3 * 16
    assert staged + slots <= s1 <= staged + slots + pads + (32 << 20), s1  # S1: 1.10 GB (round 4: 1.07)
    _lib.set_option("bwd_item12", 1)                                # the optional 12-byte stream: 16 units per 192 bytes
    try:
        s1 = query(dim, res, bw, n)
    finally:
        _lib.set_option("bwd_item12", -1)
    slots, pads = n * (5 * 2 + 11 * 4) * 12, 1024 * 733 * 15 * 12
    assert staged + slots <= s1 <= staged + slots + pads + (48 << 20), s1  # 0.98 GB
    # round 6: a PLANNED call (the batch's plan at hand) accumulates the five dense levels block by block on chip: they write no
    # items, the eleven hashed levels 12-byte units. 0.84 GB (plain: 1.10)
    arr = (ctypes.c_int32 * len(res))(*res)
    _, _, T = table_layout(res, bw, dim)
    planned = L.shacira_hashgrid_backward_planned_workspace_bytes(dim, n, len(res), 2, bw, arr, T, _lib.F32)
    slots, pads = n * 11 * 4 * 12, 1024 * 704 * 15 * 12
    assert staged + slots <= planned <= staged + slots + pads + (32 << 20), planned
    assert planned <= 0.85e9 and planned < 0.77 * query(dim, res, bw, n)
    # shapes without a plan / outside the brick pass's rule: the plain size
    assert L.shacira_hashgrid_backward_planned_workspace_bytes(dim, 65536, len(res), 2, bw, arr, T, _lib.F32) == query(dim, res, bw, 65536)
    assert L.shacira_hashgrid_backward_planned_workspace_bytes(dim, n, len(res), 2, bw, arr, T, _lib.F16) == query(dim, res, bw, n, dtype=_lib.F16)


def test_backward_workspace_bytes_match_the_recorded_counts(golden):
    """Every per-call decision of the binned backward (image size, sub-batch size, item format -- its tentative and final
    order included --, one-image-compact rule, brick levels) shows in the two workspace queries, which are host code. Their
    answers over tables x batch sizes x dtypes x option sets must equal, byte for byte, what tests/golden/
    make_bwd_workspace_golden.py recorded before the call resolver was gathered into one function."""
    g = golden("bwd_workspace_bytes.json")
    L = _lib.lib()
    assert len(g["rows"]) == len(g["tables"]) * 9 * 2 * len(g["option_sets"]) and len(g["option_sets"]) == 13
    arrays = {name: (ctypes.c_int32 * len(res))(*res) for name, (_, res, _, _) in g["tables"].items()}
    from conftest import table_layout
    rows_T = {name: table_layout(res, bw, dim)[2] for name, (dim, res, bw, _) in g["tables"].items()}
    bad = []
    for k, opts in enumerate(g["option_sets"]):
        saved = {name: _lib.get_option(name) for name in opts}
        try:
            for name, value in opts.items():
                _lib.set_option(name, value)
            for tname, n, dtype, kk, plain, planned in g["rows"]:
                if kk != k:
                    continue
                dim, res, bw, F = g["tables"][tname]
                args = (dim, n, len(res), F, bw, arrays[tname], rows_T[tname], dtype)
                got = (L.shacira_hashgrid_backward_workspace_bytes(*args),
                       L.shacira_hashgrid_backward_planned_workspace_bytes(*args))
                if got != (plain, planned):
                    bad.append((tname, n, dtype, opts, (plain, planned), got))
        finally:
            for name, value in saved.items():
                _lib.set_option(name, value)
    assert not bad, (len(bad), bad[:8])


def _entry_golden():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_hashgrid_entry_golden as mk
    return mk


def test_hashgrid_size_queries_match_the_recorded_counts(golden):
    """The forward workspace, plan and coordinate-gradient workspace queries over tables x batch sizes x fp32 / fp16 / fp64 x
    the options the plan rule reads equal, byte for byte, what tests/golden/make_hashgrid_entry_golden.py recorded before the
    entry points' shape resolver was gathered into one function (the backward queries: the test above)."""
    mk = _entry_golden()
    g = golden("hashgrid_entry_codes.json")
    assert g["option_sets"] == mk.OPTION_SETS and len(g["option_sets"]) == 7
    assert len(g["sizes"]) == len(g["tables"]) * 9 * 3 * 7 and set(g["tables"]) == {"A", "B", "Bp", "D", "lego", "tiny"}
    assert any(r[5] > 0 for r in g["sizes"]) and any(r[4] > 0 and r[5] == 0 for r in g["sizes"])
    got = mk.query_sizes(g["tables"], sorted({r[1] for r in g["sizes"]}), g["option_sets"])
    bad = [(a, b) for a, b in zip(sorted(g["sizes"]), sorted(got)) if a != b]
    assert len(got) == len(g["sizes"]) and not bad, (len(bad), bad[:8])


def test_hashgrid_entry_codes_match_the_recorded_codes(golden):
    """Every single fault and every pair of faults the eight launching hash-grid entries can carry returns the code recorded
    from the library as it stood before the shape resolver (tests/golden/make_hashgrid_entry_golden.py): which check fires, and
    which fires FIRST. Every case is refused before dispatch (the addresses are made up), so nothing here touches a GPU -- and
    where one is present the test does not run at all: a wrongly accepted call would launch on those addresses."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up addresses: replayed only where a wrongly accepted call cannot launch")
    mk = _entry_golden()
    g = golden("hashgrid_entry_codes.json")
    assert g["batches"] == mk.BATCHES and sorted(g["codes"]) == sorted(mk.ENTRIES) and len(mk.ENTRIES) == 8
    bad, total = [], 0
    for entry, per in g["codes"].items():
        for bname, rec in per.items():
            names = list(mk.faults(entry, g["batches"][bname]))
            assert names == rec["faults"], (entry, bname)
            want = {(i, None): c for i, c in enumerate(rec["single"])}
            want.update({(i, j): c for i, j, c in rec["pairs"]})
            cases = mk.cases(entry, g["batches"][bname])
            assert sorted(want, key=str) == sorted(((i, j) for i, j, _ in cases), key=str), (entry, bname)
            for i, j, args in cases:
                code = want[(i, j)]
                assert code < 0 or (code == 0 and entry in mk.ZERO_BATCH_RETURNS_0 and "n0" in (names[i], j is not None and names[j]))
                got = mk.call(entry, args)
                total += 1
                if got != code:
                    bad.append((entry, bname, names[i], None if j is None else names[j], code, got))
    assert total > 3000 and not bad, (len(bad), bad[:8])


def test_cached_size_queries_equal_the_c_queries_and_follow_the_options():
    """hip_ops' cached size queries answer what the C queries answer, and the cache is keyed by the options epoch: a shape
    that has a plan has none once `tiled` is 0, and has it again once the option is restored."""
    import torch
    from conftest import CONFIGS, geo, table_layout
    from shacira_amd import hip_ops
    L = _lib.lib()
    tables = {"B": CONFIGS["B"] + (2,), "D": CONFIGS["D"] + (2,), "lego": (3, geo(16, 512, 24), 19, 4)}
    some_plan = None
    for dim, res, bw, F in tables.values():
        arr = (ctypes.c_int32 * len(res))(*res)
        _, _, T = table_layout(res, bw, dim)
        for n in (4096, 1 << 18, 1 << 20):
            c = (dim, n, len(res), F, bw, arr, T, _lib.F32)
            py = (dim, n, T, torch.float32, res, bw, F)
            assert hip_ops.hashgrid_plan_bytes(*py) == L.shacira_hashgrid_plan_bytes(*c)
            assert hip_ops.hashgrid_backward_workspace_bytes(*py) == L.shacira_hashgrid_backward_workspace_bytes(*c)
            assert hip_ops.hashgrid_backward_workspace_bytes(*py, planned=True) == \
                L.shacira_hashgrid_backward_planned_workspace_bytes(*c)
            if L.shacira_hashgrid_plan_bytes(*c) > 0:
                some_plan = py
    before = hip_ops.hashgrid_plan_bytes(*some_plan)
    assert before > 0
    saved = _lib.get_option("tiled")
    _lib.set_option("tiled", 0)
    try:
        assert hip_ops.hashgrid_plan_bytes(*some_plan) == 0
    finally:
        _lib.set_option("tiled", saved)
    assert hip_ops.hashgrid_plan_bytes(*some_plan) == before
