"""``NeuralSDF``: [embedded position,] grid features -> decoder -> signed distance (reference
wisp/models/nefs/neural_sdf.py): same constructor options, parameter names (``grid.*``, ``decoder.*``), channel and output
shapes. The positions come FIRST in the decoder's input, as in the reference's ``sdf`` (``NeuralRadianceField`` puts them
last). The grid lookup runs through the HIP operators; the decoder uses the fused MLP kernel when its shape is one of its
instantiations and torch Linear layers otherwise.
"""
import inspect

import torch
import torch.nn as nn

from ..decoders.basic_decoders import BasicDecoder
from ..embedders import get_positional_embedder


class NeuralSDF(nn.Module):
    def __init__(self, grid=None, pos_embedder="none", pos_multires=10, position_input=True, activation_type="relu",
                 layer_type="none", hidden_dim=128, num_layers=1):
        super().__init__()
        if activation_type != "relu" or layer_type not in ("none", "linear"):
            raise NotImplementedError("relu activations and plain linear layers (the reference's SDF configs)")
        self.grid = grid
        self.pos_multires, self.position_input = pos_multires, position_input
        self.pos_embedder, self.pos_embed_dim = self.init_embedder(pos_embedder, pos_multires, position_input)
        self.activation_type, self.layer_type = activation_type, layer_type
        self.hidden_dim, self.num_layers = hidden_dim, num_layers
        self.decoder = self.init_decoder(activation_type, layer_type, num_layers, hidden_dim)
        self._forward_functions = {"sdf": self.sdf}

    def init_embedder(self, embedder_type, frequencies=None, position_input=True):
        if embedder_type == "none" and not position_input:
            return None, 0
        if embedder_type == "identity" or (embedder_type == "none" and position_input):
            return nn.Identity(), 3
        if embedder_type == "positional":
            return get_positional_embedder(frequencies=frequencies, include_input=position_input)
        raise NotImplementedError(f"Unsupported embedder type for NeuralSDF: {embedder_type}")

    def init_decoder(self, activation_type, layer_type, num_layers, hidden_dim):
        return BasicDecoder(self.decoder_input_dim(), 1, torch.relu, True, nn.Linear, num_layers, hidden_dim, [])

    def effective_feature_dim(self):
        if self.grid.multiscale_type == "cat":
            return self.grid.feature_dim * self.grid.num_lods
        return self.grid.feature_dim

    def decoder_input_dim(self):
        input_dim = self.effective_feature_dim()
        if self.position_input:
            input_dim += self.pos_embed_dim
        return input_dim

    def get_supported_channels(self):
        return set(self._forward_functions)

    @staticmethod
    def _accepted(fn, kwargs):
        """The keyword arguments ``fn`` takes (a tracer passes every field the same set, e.g. ``pidx``)."""
        names = inspect.signature(fn).parameters
        return {k: v for k, v in kwargs.items() if k in names}

    def get_forward_function(self, channel):
        """coords -> the channel's tensor; keyword arguments the function does not take are dropped."""
        if channel not in self._forward_functions:
            raise Exception(f"Channel {channel} is not supported in {self.__class__.__name__}")
        fn = self._forward_functions[channel]
        return lambda *args, **kwargs: fn(*args, **self._accepted(fn, kwargs))[channel]

    def forward(self, channels=None, **kwargs):
        """Dict of the requested channels (a single channel name returns its tensor, like the reference's BaseNeuralField).
        Keyword arguments the forward function does not take (``pidx``) are dropped."""
        requested = {channels} if isinstance(channels, str) else set(self._forward_functions if channels is None else channels)
        unsupported = requested - self.get_supported_channels()
        if unsupported:
            raise Exception(f"Channels {unsupported} are not supported in {self.__class__.__name__}")
        out = self.sdf(**self._accepted(self.sdf, kwargs))
        if isinstance(channels, str):
            return out[channels]
        return out if channels is None else {c: out[c] for c in channels}

    def sdf(self, coords, lod_idx=None):
        """coords [batch, 3] or [batch, num_samples, 3] -> dict(sdf=[batch, 1] or [batch, num_samples, 1])."""
        shape = coords.shape
        if shape[0] == 0:
            return dict(sdf=torch.zeros_like(coords)[..., 0:1])
        if lod_idx is None:
            lod_idx = self.grid.num_lods - 1
        if len(shape) == 2:
            coords = coords[:, None]
        num_samples = coords.shape[1]
        feats = self.grid.interpolate(coords, lod_idx)
        if self.pos_embedder is not None:
            embedded = self.pos_embedder(coords.reshape(-1, 3)).view(-1, num_samples, self.pos_embed_dim)
            feats = torch.cat([embedded, feats], dim=-1)
        sdf = self.decoder(feats)
        if len(shape) == 2:
            sdf = sdf[:, 0]
        return dict(sdf=sdf)

    def public_properties(self):
        return {"Grid": self.grid, "Pos. Embedding": self.pos_embedder, "Decoder (sdf)": self.decoder}
