"""``NeuralImage``: 2-D coordinates -> grid features (+ embedded position) -> colour decoder (reference
wisp/models/nefs/image.py:19-177): the same constructor options and defaults, parameter names (``grid.*``,
``decoder_color.layers.N.*``, ``decoder_color.lout.*``, ``pos_embedder.bands`` -- the optimiser groups and the model file go by
them) and channels. The grid lookup runs through the HIP operators. With a positional embedder the decoder's input row
``[features | coords | sin | cos]`` is written by one HIP kernel (``fused_embedder``, an addition) instead of the seven torch
ops of ``cat([features, embedder(coords)])``; the decoder takes the fused MLP kernel when its shape is one of its
instantiations (32 features + the 16-wide encoding of ``pos_multires=4`` is: 48 -> 16 -> 16 -> 3).
"""
import torch
import torch.nn as nn

from ..activations import get_activation_class
from ..decoders.basic_decoders import BasicDecoder
from ..embedders import PositionalEmbedder, get_positional_embedder


class NeuralImage(nn.Module):
    def __init__(self, grid=None, pos_embedder="none", pos_multires=10, position_input=False, activation_type="relu",
                 final_activation="none", layer_type="none", hidden_dim=128, num_layers=1, *, fused_embedder=True):
        super().__init__()
        if layer_type not in ("none", "linear"):
            raise NotImplementedError("plain linear layers (the reference's image configs)")
        self.grid = grid
        self.fused_embedder = fused_embedder
        self.pos_embedder, self.pos_embed_dim = self.init_embedder(pos_embedder, pos_multires, include_input=position_input)
        self.activation_type = activation_type
        self.final_activation = get_activation_class(final_activation)
        self.layer_type = layer_type
        self.hidden_dim, self.num_layers = hidden_dim, num_layers
        self.decoder_color = self.init_decoders(activation_type, layer_type, num_layers, hidden_dim)

    def init_embedder(self, embedder_type, frequencies=None, include_input=False):
        if embedder_type == "none" and not include_input:
            return None, 0
        if embedder_type == "identity" or (embedder_type == "none" and include_input):
            return nn.Identity(), 2                                   # the position is always 2-D
        if embedder_type == "positional":
            return get_positional_embedder(frequencies=frequencies, input_dim=2, include_input=include_input,
                                           fused=self.fused_embedder)
        raise NotImplementedError(f"Unsupported embedder type for NeuralImage: {embedder_type}")

    def init_decoders(self, activation_type, layer_type, num_layers, hidden_dim):
        return BasicDecoder(self.color_net_input_dim(), 3, get_activation_class(activation_type), True, nn.Linear,
                            num_layers + 1, hidden_dim, [])

    def effective_feature_dim(self):
        if self.grid.multiscale_type == "cat":
            return self.grid.feature_dim * self.grid.num_lods
        return self.grid.feature_dim

    def color_net_input_dim(self):
        return self.effective_feature_dim() + self.pos_embed_dim

    def get_supported_channels(self):
        return {"rgb"}

    def forward(self, channels=None, **kwargs):
        """Dict of the requested channels (a single channel name returns its tensor, like the reference's BaseNeuralField)."""
        out = self.rgb(**kwargs)
        if isinstance(channels, str):
            return out[channels]
        return out if channels is None else {c: out[c] for c in channels}

    def rgb(self, coords, lod_idx=None):
        """coords [batch, 2] -> {"rgb": [batch, 3]} at ``lod_idx`` (the finest active level by default)."""
        if lod_idx is None:
            lod_idx = len(self.grid.active_lods) - 1
        batch = coords.shape[0]
        feats = self.grid.interpolate(coords, lod_idx).reshape(batch, self.effective_feature_dim())
        if isinstance(self.pos_embedder, PositionalEmbedder):
            feats = self.pos_embedder.rows(feats, coords)
        elif self.pos_embedder is not None:
            feats = torch.cat([feats, self.pos_embedder(coords).view(batch, self.pos_embed_dim)], dim=-1)
        return dict(rgb=self.final_activation(self.decoder_color(feats)))

    def public_properties(self):
        return {"Grid": self.grid, "Pos. Embedding": self.pos_embedder, "Decoder (color)": self.decoder_color,
                "Final Activation": self.final_activation}
