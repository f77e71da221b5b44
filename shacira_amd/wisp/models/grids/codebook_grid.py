"""``CodebookOctreeGrid``: an ``OctreeGrid`` whose corners store logits over a small per-level dictionary of feature vectors
(reference wisp/models/grids/codebook_grid.py, the VQAD grid).

``dictionary`` is a ``ParameterList`` of [2^bitwidth, F] and ``features`` holds the logits [C_l + 1, 2^bitwidth], both drawn
as in the reference (dictionaries first, then logits, ``zeros`` then ``+= randn * std``).

The reference evaluates the softmax and its straight-through estimator for every (sample, corner) pair
(codebook_grid.py:285-293). The keys depend on the corner only, so this module decodes ONCE PER CORNER ROW in torch and
hands the decoded [C_l + 1, F] tables to the same fused lookup as ``OctreeGrid``:
  training: ``keys = y_hard - y_soft.detach() + y_soft``, ``table = keys @ dictionary``;
  eval:     ``table = dictionary[argmax(logits)]``.
That is the same function of the parameters with the same gradients, and the softmax work drops from 8 x samples rows to
C_l rows. ``bake()`` and ``size(use_torchac=True)`` are not implemented.
"""
from typing import Any, Dict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .octree_grid import OctreeGrid


class CodebookOctreeGrid(OctreeGrid):
    def __init__(self, accelstruct, feature_dim: int, base_lod: int, num_lods: int = 1, interpolation_type: str = "linear",
                 multiscale_type: str = "cat", feature_std: float = 0.0, feature_bias: float = 0.0,
                 codebook_bitwidth: int = 8):
        self.bitwidth = codebook_bitwidth
        super().__init__(accelstruct=accelstruct, feature_dim=feature_dim, base_lod=base_lod, num_lods=num_lods,
                         interpolation_type=interpolation_type, multiscale_type=multiscale_type, feature_std=feature_std,
                         feature_bias=feature_bias)

    def _new_row_value(self) -> float:
        return 0.0

    def _draw_tables(self, rows):
        self.dictionary_size = 2 ** self.bitwidth
        self.dictionary = nn.ParameterList([])
        for _ in rows:
            fts = torch.zeros(self.dictionary_size, self.feature_dim)
            fts += torch.randn_like(fts) * self.feature_std
            self.dictionary.append(nn.Parameter(fts))
        self.features = nn.ParameterList([])
        for n in rows:
            fts = torch.zeros(n, self.dictionary_size)
            fts += torch.randn_like(fts) * self.feature_std
            self.features.append(nn.Parameter(fts))

    def decode_table(self, lod_idx: int) -> torch.Tensor:
        """The [C_l + 1, F] feature table of level ``active_lods[lod_idx]``, decoded once per corner row."""
        logits, dictionary = self.features[lod_idx], self.dictionary[lod_idx]
        if not self.training:
            return dictionary[torch.max(logits, dim=-1)[1]]
        y_soft = F.softmax(logits, dim=-1)
        index = y_soft.max(-1, keepdim=True)[1]
        y_hard = torch.zeros_like(logits, memory_format=torch.legacy_contiguous_format).scatter_(-1, index, 1.0)
        keys = y_hard - y_soft.detach() + y_soft
        return keys @ dictionary

    def _tables(self, num_feats):
        return [self.decode_table(i) for i in range(num_feats)]

    def bake(self):
        raise NotImplementedError("CodebookOctreeGrid.bake is not implemented")

    def size(self, use_torchac=False, use_prob_model=False):
        """(0.0, bits): the dictionaries at their dtype's width plus the entropy of each level's argmax indices."""
        if use_torchac:
            raise NotImplementedError("the torchac coder is not vendored: size(use_torchac=True) is not available")
        dict_size = sum([d.numel() * torch.finfo(d.dtype).bits for d in self.dictionary])
        index_bits = 0
        for dim in range(len(self.features)):
            weight = torch.argmax(self.features[dim], dim=-1)
            _, counts = torch.unique(weight, return_counts=True)
            probs = counts / torch.sum(counts)
            information_bits = torch.clamp(-1.0 * torch.log(probs + 1e-10) / np.log(2.0), 0, 1000)
            index_bits += torch.sum(information_bits * counts).item()
        return 0.0, index_bits + dict_size

    def name(self) -> str:
        return "Codebook Grid"

    def public_properties(self) -> Dict[str, Any]:
        return {**super().public_properties(), "Bitwidth": self.bitwidth}
