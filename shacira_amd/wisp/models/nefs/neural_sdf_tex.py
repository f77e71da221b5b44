"""``NeuralSDFTex``: [embedded position,] grid features -> decoder -> (rgb, signed distance) (reference
wisp/models/nefs/neural_sdf_tex.py): ``NeuralSDF`` with a four-channel decoder, one forward function serving both channels.
As in the reference the position is a decoder input only with the ``'positional'`` embedder."""
import torch
import torch.nn as nn

from ..decoders.basic_decoders import BasicDecoder
from ..embedders import get_positional_embedder
from .neural_sdf import NeuralSDF


class NeuralSDFTex(NeuralSDF):
    def __init__(self, grid=None, embedder_type="none", pos_multires=10, activation_type="relu", layer_type="none",
                 hidden_dim=128, num_layers=1):
        self.embedder_type = embedder_type
        super().__init__(grid=grid, pos_embedder=embedder_type, pos_multires=pos_multires,
                         position_input=embedder_type != "none", activation_type=activation_type, layer_type=layer_type,
                         hidden_dim=hidden_dim, num_layers=num_layers)
        self._forward_functions = {"rgb": self.rgbsdf, "sdf": self.rgbsdf}

    def init_embedder(self, embedder_type, frequencies=None, position_input=True):
        if embedder_type == "none":
            return None, 0
        if embedder_type == "positional":
            return get_positional_embedder(frequencies=frequencies)
        raise NotImplementedError(f"Unsupported embedder type for NeuralSDFTex: {embedder_type}")

    def decoder_input_dim(self):
        return self.effective_feature_dim() + (self.pos_embed_dim if self.pos_embedder is not None else 0)

    def init_decoder(self, activation_type, layer_type, num_layers, hidden_dim):
        return BasicDecoder(self.decoder_input_dim(), 4, torch.relu, True, nn.Linear, num_layers, hidden_dim, [])

    def forward(self, channels=None, **kwargs):
        requested = {channels} if isinstance(channels, str) else set(self._forward_functions if channels is None else channels)
        unsupported = requested - self.get_supported_channels()
        if unsupported:
            raise Exception(f"Channels {unsupported} are not supported in {self.__class__.__name__}")
        out = self.rgbsdf(**self._accepted(self.rgbsdf, kwargs))
        if isinstance(channels, str):
            return out[channels]
        return out if channels is None else {c: out[c] for c in channels}

    def rgbsdf(self, coords, lod_idx=None):
        """coords [batch, 3] or [batch, num_samples, 3] -> dict(rgb=[..., 3] in (0, 1), sdf=[..., 1])."""
        shape = coords.shape
        if shape[0] == 0:
            return dict(rgb=torch.zeros_like(coords), sdf=torch.zeros_like(coords)[..., 0:1])
        if lod_idx is None:
            lod_idx = self.grid.num_lods - 1
        if len(shape) == 2:
            coords = coords[:, None]
        num_samples = coords.shape[1]
        feats = self.grid.interpolate(coords, lod_idx)
        if self.pos_embedder is not None:
            embedded = self.pos_embedder(coords.reshape(-1, 3)).view(-1, num_samples, self.pos_embed_dim)
            feats = torch.cat([embedded, feats], dim=-1)
        rgbsdf = self.decoder(feats)
        if len(shape) == 2:
            rgbsdf = rgbsdf[:, 0]
        return dict(rgb=torch.sigmoid(rgbsdf[..., :3]), sdf=rgbsdf[..., 3:])

    def public_properties(self):
        return {"Grid": self.grid, "Pos. Embedding": self.pos_embedder, "Decoder (rgbsdf)": self.decoder}
