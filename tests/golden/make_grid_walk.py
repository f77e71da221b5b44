#!/usr/bin/env python3
"""Record tests/golden/grid_walk.npz: what the dense-grid ray walk computes on an MI355X, input by input, so that a later
change of the walk (shacira_amd/csrc/grid_walk.h) is held to these bits and not only to itself.

Run:  python tests/golden/make_grid_walk.py --commit HASH [--out FILE]        (needs the GPU)

Only ``render.raytrace_dense``, the ``shacira_raytrace_dense_count`` entry point and ``hip_ops.spc_first_hit`` are called, so the
script runs on any commit that has them; ``SHACIRA_HIP_LIB`` selects the build of the library that is recorded, ``--commit``
names the commit of that build. The inputs come from the seeded generators of tests/test_gpu_render_edges.py (dense trace) and
tests/test_gpu_spc.py (first hit); occupancies are stored as packed bits (tests/spc_ref.py, ``occupancy_bits``).

  dense.<N>.<level>.{origins, dirs, bits, counts, ridx, pidx, depth}
  hit.<level>.<kind>.{bits, colors}     hit.<level>.<kind>.<N>.{origins, dirs, depth, hit, pidx[, rgb]}

The first hit is recorded without colours and, where the set has cells, with them; depth, hit and pidx of the two calls are
required to be equal here and stored once."""
import argparse
import ctypes
import os
import subprocess
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import spc_ref as S
import test_gpu_render_edges as E
import test_gpu_spc as P
from shacira_amd import _lib, hip_ops, render

DENSE = [(1, 0, 300), (1, 8, 300), (255, 1, 300), (256, 3, 300), (257, 8, 303), (600, 3, 300)]      # N, level, seed
HIT_LEVELS, HIT_KINDS, HIT_N = (1, 2, 5), ("empty", "dense", "first", "last", "random"), (1, 63, 64, 65, 257)


def record_dense(out, dev):
    for N, level, seed in DENSE:
        o, d = E._trace_rays(N, level, seed)
        occ = E._trace_occupancy(level)
        od, dd, occ_d = o.to(dev), d.to(dev), occ.to(dev)
        ridx, pidx, depth = render.raytrace_dense(od, dd, occ_d, level)
        counts = torch.full((N,), -1, dtype=torch.int32, device=dev)
        occ8 = occ_d.to(torch.uint8).contiguous()
        assert _lib.lib().shacira_raytrace_dense_count(N, od.data_ptr(), dd.data_ptr(), occ8.data_ptr(), level, counts.data_ptr(),
                                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
        torch.cuda.synchronize()
        assert int(counts.sum()) == ridx.shape[0] > 0
        key = f"dense.{N}.{level}."
        out[key + "origins"], out[key + "dirs"] = o.numpy(), d.numpy()
        out[key + "bits"] = S.occupancy_bits(occ.numpy())
        out[key + "counts"], out[key + "ridx"] = counts.cpu().numpy(), ridx.cpu().numpy()
        out[key + "pidx"], out[key + "depth"] = pidx.cpu().numpy(), depth.cpu().numpy()
        print(key, "nuggets", ridx.shape[0], flush=True)


def record_first_hit(out, dev):
    from shacira_amd.wisp.ops.spc.structured import pack_occupancy
    for level in HIT_LEVELS:
        for kind in HIT_KINDS:
            rng = np.random.default_rng(level * 10 + len(kind))
            occ = P.occupancy(kind, level, rng)
            words = pack_occupancy(torch.from_numpy(occ).to(dev))
            rank_h, cells = S.rank_ref(words.cpu().numpy().view(np.uint32))
            rank = torch.from_numpy(rank_h).to(dev)
            colors = torch.from_numpy(rng.integers(0, 256, (cells, 4), dtype=np.uint8))
            key = f"hit.{level}.{kind}."
            out[key + "bits"], out[key + "colors"] = S.occupancy_bits(occ), colors.numpy()
            hits = 0
            for N in HIT_N:
                o_h, d_h = P.rays_for(occ, level, N, rng)
                assert o_h.shape == (N, 3)
                o, d = torch.from_numpy(o_h).to(dev), torch.from_numpy(d_h).to(dev)
                depth, hit, pidx, rgb = hip_ops.spc_first_hit(o, d, level, words)
                assert rgb is None
                out[f"{key}{N}.origins"], out[f"{key}{N}.dirs"] = o_h, d_h
                out[f"{key}{N}.depth"], out[f"{key}{N}.hit"] = depth.cpu().numpy(), hit.cpu().numpy()
                out[f"{key}{N}.pidx"] = pidx.cpu().numpy()
                if cells:
                    depth2, hit2, pidx2, rgb = hip_ops.spc_first_hit(o, d, level, words, rank, colors.to(dev))
                    assert torch.equal(depth2.view(torch.int32), depth.view(torch.int32))
                    assert torch.equal(hit2, hit) and torch.equal(pidx2, pidx)
                    out[f"{key}{N}.rgb"] = rgb.cpu().numpy()
                hits += int(hit.sum())
            print(key, "cells", cells, "hits", hits, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the recorded library was built from (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "grid_walk.npz"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("make_grid_walk.py records on the GPU; there is none here")
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    dev = torch.device("cuda:0")
    out = {"commit": np.array(commit), "device": np.array(torch.cuda.get_device_properties(dev).gcnArchName)}
    record_dense(out, dev)
    record_first_hit(out, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes, recorded at", commit)


if __name__ == "__main__":
    main()
