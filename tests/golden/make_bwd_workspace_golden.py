#!/usr/bin/env python3
"""Generate tests/golden/bwd_workspace_bytes.json: what the two backward workspace queries of the BUILT library answer.

Run:  python tests/golden/make_bwd_workspace_golden.py        (needs a built shacira_amd/lib; no GPU: the queries are host code)

The queries (shacira_hashgrid_backward_workspace_bytes, shacira_hashgrid_backward_planned_workspace_bytes) are pure functions of
the shape and the options, and every per-call decision of the binned backward shows in them: image size, sub-batch size, item
format, one-image-compact rule, brick levels. The file records them for tables x batch sizes x dtypes x option sets, so that a
change to the host code that resolves a call has to leave every byte count as it was (tests/test_abi.py). Recorded once, from
the library as it stood before the call resolver was gathered into one function; regenerate only for a change that is MEANT to
move a count, and say so.

Layout: {"tables": {name: [dim, resolutions, bitwidth, F]}, "option_sets": [{option: value}], "rows": [[table, n, dtype,
option set index, plain bytes, planned bytes]]}."""
import ctypes
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))              # tests/ (conftest)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from conftest import CONFIGS, geo, table_layout
from shacira_amd import _lib

TABLES = {name: list(CONFIGS[name]) + [2] for name in ("A", "B", "Bp", "D")}
TABLES["lego"] = [3, geo(16, 512, 24), 19, 4]
TABLES["tiny"] = [3, [4, 8, 16], 12, 2]
NS = [1, 2047, 4096, 65536, (1 << 17) - 1, 1 << 17, (1 << 18) + 13, 1 << 20, (1 << 22) + 5]
OPTION_SETS = [
    {},
    {"bwd_item12": 0}, {"bwd_item12": 1},
    {"bwd_brick": 0}, {"bwd_brick": 1},
    {"bin_acc_kib": 64}, {"bin_acc_kib": 128},
    {"bwd_run_pad": 0},
    {"bwd_compact": 0},
    {"bin_batch_mib": 64},
    {"bwd_brick_fork": 0},
    {"bwd_brick_span": 1},
    {"bwd_brick_lo": 1, "bwd_brick_hi": 3},
]


def query_all(tables, ns, option_sets):
    """[[table, n, dtype, option set index, plain, planned]] from the loaded library; every option is restored."""
    L = _lib.lib()
    rows = []
    for k, opts in enumerate(option_sets):
        saved = {name: _lib.get_option(name) for name in opts}
        try:
            for name, value in opts.items():
                _lib.set_option(name, value)
            for tname, (dim, res, bw, F) in tables.items():
                arr = (ctypes.c_int32 * len(res))(*res)
                _, _, T = table_layout(res, bw, dim)
                for n in ns:
                    for dtype in (_lib.F32, _lib.F16):
                        args = (dim, n, len(res), F, bw, arr, T, dtype)
                        rows.append([tname, n, dtype, k, int(L.shacira_hashgrid_backward_workspace_bytes(*args)),
                                     int(L.shacira_hashgrid_backward_planned_workspace_bytes(*args))])
        finally:
            for name, value in saved.items():
                _lib.set_option(name, value)
    return rows


def main():
    tables = {name: [dim, [int(r) for r in res], bw, F] for name, (dim, res, bw, F) in TABLES.items()}
    out = {"tables": tables, "option_sets": OPTION_SETS, "rows": query_all(tables, NS, OPTION_SETS)}
    path = os.path.join(HERE, "bwd_workspace_bytes.json")
    with open(path, "w") as fh:
        fh.write('{"tables": %s,\n "option_sets": %s,\n "rows": [\n' % (json.dumps(out["tables"]), json.dumps(out["option_sets"])))
        fh.write(",\n".join(json.dumps(r) for r in out["rows"]))
        fh.write("\n]}\n")
    print(path, os.path.getsize(path), "bytes,", len(out["rows"]), "rows")


if __name__ == "__main__":
    main()
