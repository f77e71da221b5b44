#!/usr/bin/env python3
"""Generate tests/golden/hashgrid_entry_codes.json: what the hash-grid entry points of the BUILT library answer on the host.

Run:  python tests/golden/make_hashgrid_entry_golden.py     (needs a built shacira_amd/lib and a machine WITHOUT a GPU)

Two halves, both host code (validation and sizing precede every HIP call):

 * "sizes": shacira_hashgrid_forward_workspace_bytes, _plan_bytes, _coords_backward_workspace_bytes and
   _coords_backward2_workspace_bytes over the tables and batch sizes of make_bwd_workspace_golden.py x fp32 / fp16 / fp64 x the
   options the plan rule and the forward workspace read (tiled, fwd_variant). The two backward queries are in
   bwd_workspace_bytes.json.
 * "codes": the return code of the eight launching entries (forward, forward_planned, backward, backward_planned,
   backward_levels, coords_backward, coords_backward2, debug_corners) for every single fault an entry can report and every pair
   of faults it can carry at once -- the pairs pin the ORDER of validation. A fault is a set of argument overrides on a base call
   (table D of conftest.CONFIGS, made-up non-NULL addresses, exactly sufficient buffers); two faults that override the same
   argument cannot be carried at once, and the two orders of a pair are the same call, recorded once. Two batches: 2^18 samples
   (the forward sorts them: a plan exists) and 4096 (it does not: a plan buffer is ignored).

Every recorded case must be REFUSED BEFORE DISPATCH: the addresses are made up. The base call is never made; a case is made only
with a fault applied; the recorder refuses to run where a GPU is present and refuses to write a file in which a launching entry
returned a positive code (a HIP error: something was dispatched) or zero -- except num_coords == 0 through forward,
forward_planned and coords_backward, which return 0 before dispatch. tests/test_abi.py builds the same cases from this module
and skips the launching half where a GPU is present.

Recorded once, from the library as it stood before the entry points' shape resolver (resolve_grid in csrc/api.hip) was gathered
into one function; regenerate only for a change that is MEANT to move a code or a size, and say so.

Layout: {"tables": {name: [dim, resolutions, bitwidth, F]}, "option_sets": [{option: value}], "sizes": [[table, n, dtype,
option set index, forward workspace, plan, coords_backward workspace, coords_backward2 workspace]], "batches": {name: n},
"codes": {entry: {batch: {"faults": [name], "single": [code per fault], "pairs": [[i, j, code]]}}}}."""
import ctypes
import itertools
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))              # tests/ (conftest)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from conftest import CONFIGS, table_layout
from make_bwd_workspace_golden import NS, TABLES
from shacira_amd import _lib

OPTION_SETS = [{}, {"tiled": 0}, {"tiled": 1}, {"fwd_variant": 0}, {"fwd_variant": 3}, {"fwd_variant": 8}, {"fwd_variant": 9}]
DTYPES = (_lib.F32, _lib.F16, _lib.F64)
SIZE_QUERIES = ("shacira_hashgrid_forward_workspace_bytes", "shacira_hashgrid_plan_bytes",
                "shacira_hashgrid_coords_backward_workspace_bytes", "shacira_hashgrid_coords_backward2_workspace_bytes")
BATCHES = {"sorts": 1 << 18, "plain": 4096}


class options:
    """Set the given options for a block; every one is restored."""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        self.saved = {name: _lib.get_option(name) for name in self.opts}
        for name, value in self.opts.items():
            _lib.set_option(name, value)

    def __exit__(self, *exc):
        for name, value in self.saved.items():
            _lib.set_option(name, value)


def query_sizes(tables, ns, option_sets):
    L = _lib.lib()
    rows = []
    for k, opts in enumerate(option_sets):
        with options(opts):
            for tname, (dim, res, bw, F) in tables.items():
                arr = (ctypes.c_int32 * len(res))(*res)
                _, _, T = table_layout(res, bw, dim)
                for n, dtype in itertools.product(ns, DTYPES):
                    args = (dim, n, len(res), F, bw, arr, T, dtype)
                    rows.append([tname, n, dtype, k] + [int(getattr(L, q)(*args)) for q in SIZE_QUERIES])
    return rows


# ---- the launching entries ------------------------------------------------------------------------------------------------
ONE = 16          # a made-up address: never dereferenced, every case is refused first
ALIGNED = 64      # ... of a 16-byte aligned grad_output (what the planned backward's size query assumes)
HEAD = ("dim", "n", "L", "F", "bw", "res", "first", "T")
ENTRIES = {       # argument names in the order of the C signature
    "forward": HEAD + ("coords", "codebook", "dtype", "feats", "ws", "wsb", "stream"),
    "forward_planned": HEAD + ("coords", "codebook", "dtype", "feats", "plan", "planb", "flags", "ws", "wsb", "stream"),
    "backward": HEAD + ("coords", "go", "dtype", "gcb", "ws", "wsb", "stream"),
    "backward_planned": HEAD + ("coords", "go", "dtype", "gcb", "plan", "planb", "ws", "wsb", "stream"),
    "backward_levels": HEAD + ("coords", "go", "dtype", "gcb", "lb", "le", "flags", "ws", "wsb", "stream"),
    "coords_backward": HEAD + ("coords", "codebook", "go", "dtype", "gc", "plan", "planb", "ws", "wsb", "stream"),
    "coords_backward2": HEAD + ("coords", "codebook", "go", "ggc", "dtype", "ggo", "gcb", "gc", "plan", "planb", "ws", "wsb",
                                "stream"),
    "debug_corners": ("dim", "n", "L", "bw", "res", "coords", "rows", "w", "stream"),
}
POINTERS = {      # the pointers an entry requires (each NULL in turn)
    "forward": ("first", "coords", "codebook", "feats"),
    "forward_planned": ("first", "coords", "codebook", "feats"),
    "backward": ("first", "coords", "go", "gcb"),
    "backward_planned": ("first", "coords", "go", "gcb"),
    "backward_levels": ("first", "coords", "go", "gcb"),
    "coords_backward": ("first", "coords", "codebook", "go", "gc"),
    "coords_backward2": ("first", "coords", "codebook", "go", "ggc"),    # (all three outputs asked: both tables are read)
    "debug_corners": ("coords",),
}
ZERO_BATCH_RETURNS_0 = ("forward", "forward_planned", "coords_backward")
_arrays = {}      # resolutions arrays stay alive while ctypes holds their address


def _table():
    dim, res, bw = CONFIGS["D"]
    return dim, [int(r) for r in res], bw, table_layout(res, bw, dim)[2]


def _res(values):
    key = tuple(values)
    if key not in _arrays:
        _arrays[key] = (ctypes.c_int32 * len(key))(*key)
    return _arrays[key]


def base_call(entry, n):
    """The complete, valid call of `entry` on table D with exactly sufficient buffers -- NEVER made: see cases()."""
    L = _lib.lib()
    dim, res, bw, T = _table()
    shape = (dim, n, len(res), 2, bw, _res(res), T)
    fwd, plan, bwd, bwd_planned = (int(getattr(L, "shacira_hashgrid_" + q)(*shape, _lib.F32)) for q in (
        "forward_workspace_bytes", "plan_bytes", "backward_workspace_bytes", "backward_planned_workspace_bytes"))
    b = dict(dim=dim, n=n, L=len(res), F=2, bw=bw, res=_res(res), T=T, dtype=_lib.F32, stream=None, lb=0, le=len(res), flags=0)
    b.update({name: ONE for name in ("first", "coords", "codebook", "feats", "go", "gcb", "gc", "ggc", "ggo", "rows", "w",
                                     "plan", "ws")})
    b["planb"] = plan                    # (0 at the batch that does not sort: the buffer is ignored)
    b["wsb"] = {"forward": fwd, "forward_planned": fwd - plan, "backward": bwd, "backward_levels": bwd,
                "backward_planned": bwd_planned}.get(entry, 0)
    if entry == "backward_planned":
        b["go"] = ALIGNED
    return b


def faults(entry, n):
    """{name: argument overrides} of every fault `entry` can report at batch size `n`, in a fixed order."""
    L = _lib.lib()
    names = ENTRIES[entry]
    b = base_call(entry, n)
    dim, res, bw, T = _table()
    f = {"dim4": {"dim": 4}, "lods0": {"L": 0}, "lods33": {"L": 33}}
    if "F" in names:
        f.update({"F0": {"F": 0}, "F3": {"F": 3}})
    f.update({"bw0": {"bw": 0}, "bw31": {"bw": 31}, "res_null": {"res": None}, "res_zero": {"res": _res(res[:3] + [0] + res[4:])}})
    if "T" in names:
        f["rows_neg"] = {"T": -1}
    if "dtype" in names:
        f["dtype7"] = {"dtype": 7}
    if entry == "coords_backward2":
        f["f64"] = {"dtype": _lib.F64}
    f["n_neg"] = {"n": -1}
    if entry in ZERO_BATCH_RETURNS_0:
        f["n0"] = {"n": 0}
    for p in POINTERS[entry]:
        f[p + "_null"] = {p: None}
    if entry == "debug_corners":
        f["outputs_null"] = {"rows": None, "w": None}
    if entry == "coords_backward2":
        f["no_output"] = {"ggo": None, "gcb": None, "gc": None}
        need16 = int(L.shacira_hashgrid_coords_backward2_workspace_bytes(dim, n, len(res), 2, bw, _res(res), T, _lib.F16))
        assert need16 > 0
        f["f16_ws_null"] = {"dtype": _lib.F16, "ws": None, "wsb": 0}
        f["f16_ws_short"] = {"dtype": _lib.F16, "wsb": need16 - 1}
    if b["wsb"] > 0:       # (forward_planned: the caller's plan is used at "sorts" -- the query less plan_bytes -- and ignored
        f["ws_null"] = {"ws": None}                # at "plain" -- the whole query: both forms of its workspace check)
        f["ws_short"] = {"wsb": b["wsb"] - 1}
    if "plan" in names and b["planb"] > 0:
        f["plan_short"] = {"planb": b["planb"] - 1}
    if entry == "forward_planned":
        f["flags2"] = {"flags": 2}
        f["ready_no_plan"] = {"plan": None, "planb": 0, "flags": _lib.PLAN_READY, "wsb": b["wsb"] + b["planb"]}
    if entry == "backward_levels":
        f.update({"lb_neg": {"lb": -1}, "le_over": {"le": len(res) + 1}, "empty_range": {"lb": 3, "le": 3},
                  "partial_f64": {"lb": 0, "le": 3, "dtype": _lib.F64}, "partial_dtype7": {"lb": 0, "le": 3, "dtype": 7},
                  "f16_stage_all": {"dtype": _lib.F16, "flags": _lib.BWD_STAGE_ALL_LEVELS},
                  "f16_reuse_staged": {"dtype": _lib.F16, "flags": _lib.BWD_REUSE_STAGED}})
    return f


def cases(entry, n):
    """[(i, j or None, argument tuple)] over faults(entry, n): every single fault, every pair with disjoint overrides."""
    b, f = base_call(entry, n), list(faults(entry, n).values())
    out = [(i, None, dict(b, **f[i])) for i in range(len(f))]
    out += [(i, j, dict(b, **f[i], **f[j])) for i, j in itertools.combinations(range(len(f)), 2) if not set(f[i]) & set(f[j])]
    return [(i, j, tuple(args[name] for name in ENTRIES[entry])) for i, j, args in out]


def call(entry, args):
    return int(getattr(_lib.lib(), "shacira_hashgrid_" + entry)(*args))


def record_codes():
    import torch
    if torch.cuda.is_available():
        raise SystemExit("a GPU is present: the launching entries are recorded on made-up addresses, on a machine without one")
    out = {}
    for entry, (bname, n) in itertools.product(ENTRIES, BATCHES.items()):
        names = list(faults(entry, n))
        rec = out.setdefault(entry, {})[bname] = {"faults": names, "single": [None] * len(names), "pairs": []}
        for i, j, args in cases(entry, n):
            code = call(entry, args)
            zero_ok = entry in ZERO_BATCH_RETURNS_0 and "n0" in (names[i], None if j is None else names[j])
            if code > 0 or (code == 0 and not zero_ok):
                raise SystemExit(f"{entry} {bname} {names[i]} {None if j is None else names[j]}: code {code} -- not refused "
                                 f"before dispatch; nothing written")
            if j is None:
                rec["single"][i] = code
            else:
                rec["pairs"].append([i, j, code])
    return out


def main():
    tables = {name: [dim, [int(r) for r in res], bw, F] for name, (dim, res, bw, F) in TABLES.items()}
    codes = record_codes()
    sizes = query_sizes(tables, NS, OPTION_SETS)
    path = os.path.join(HERE, "hashgrid_entry_codes.json")
    with open(path, "w") as fh:
        fh.write('{"tables": %s,\n "option_sets": %s,\n "sizes": [\n' % (json.dumps(tables), json.dumps(OPTION_SETS)))
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in sizes))
        fh.write('\n],\n "batches": %s,\n "codes": {\n' % json.dumps(BATCHES))
        fh.write(",\n".join('%s: {%s}' % (json.dumps(entry), ",\n  ".join(
            "%s: %s" % (json.dumps(bname), json.dumps(rec, separators=(",", ":"))) for bname, rec in per.items()))
            for entry, per in codes.items()))
        fh.write("\n}}\n")
    json.load(open(path))
    print(path, os.path.getsize(path), "bytes,", len(sizes), "size rows,",
          sum(len(r["single"]) + len(r["pairs"]) for per in codes.values() for r in per.values()), "codes")


if __name__ == "__main__":
    main()
