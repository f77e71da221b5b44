#!/usr/bin/env python3
"""Generate tests/golden/positional_embedder.npz by RUNNING the reference's PositionalEmbedder on the CPU (dev container only).

Run:  python tests/golden/make_posenc_golden.py        (needs /root/reference)

The reference's wisp/models/embedders/positional_embedder.py is imported from its file with ``wisp.core.WispModule`` shimmed by
a plain nn.Module (as make_golden.py shims the packages that pull kaolin / CUDA). Recorded per case: the constructor arguments, the
coordinates, the bands and the output. Nothing of the reference is copied: outputs are plain arrays."""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch

CASES = {      # name: (input_dim, num_freq, include_input, log_sampling)
    "d2_f4_in": (2, 4, True, True),
    "d2_f4_noin": (2, 4, False, True),
    "d3_f10": (3, 10, True, True),
    "d3_f5_lin": (3, 5, True, False),
}


def _reference_module():
    core = types.ModuleType("wisp.core")

    class WispModule(torch.nn.Module):
        pass

    core.WispModule = WispModule
    wisp = types.ModuleType("wisp")
    wisp.__path__ = []
    wisp.core = core
    sys.modules["wisp"], sys.modules["wisp.core"] = wisp, core
    spec = importlib.util.spec_from_file_location("reference_positional_embedder",
                                                  f"{REF}/wisp/models/embedders/positional_embedder.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = _reference_module()
    rng = np.random.default_rng(20240)
    out = {}
    for name, (d, F, include_input, log_sampling) in CASES.items():
        coords = rng.uniform(-1, 1, (33, d)).astype(np.float32)
        coords[0] = 1.0
        coords[1] = -1.0
        coords[2] = 0.0
        emb = ref.PositionalEmbedder(F, F - 1, log_sampling=log_sampling, include_input=include_input, input_dim=d)
        with torch.no_grad():
            y = emb(torch.from_numpy(coords))
        assert y.shape[1] == emb.out_dim
        out[f"{name}.args"] = np.array([d, F, int(include_input), int(log_sampling)], np.int64)
        out[f"{name}.coords"] = coords
        out[f"{name}.bands"] = emb.bands.detach().numpy().astype(np.float32)
        out[f"{name}.out"] = y.numpy().astype(np.float32)
    path = os.path.join(HERE, "positional_embedder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
