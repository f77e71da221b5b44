"""Activation functions by name (reference wisp/models/activations/basic_activations.py:12-109, restated): what
``activation_type`` / ``final_activation`` of the neural fields select."""
import torch
import torch.nn as nn


class FullSort(nn.Module):
    """Sort along the feature dimension (Anil et al. 2019, arXiv:1811.05381)."""

    def forward(self, x):
        return torch.sort(x, dim=-1)[0]


class MinMax(nn.Module):
    """Sort every pair of neighbouring features of x [batch, 2n]: (min, max) (arXiv:1811.05381)."""

    def forward(self, x):
        n, m = x.shape
        x = x.reshape(n, m // 2, 2)
        return torch.cat([x.min(-1, keepdim=True)[0], x.max(-1, keepdim=True)[0]], dim=-1).reshape(n, m)


class Identity(nn.Module):
    def forward(self, x):
        return x


class Clamp(nn.Module):
    def __init__(self, min=None, max=None):
        super().__init__()
        self.min, self.max = min, max

    def forward(self, x):
        return torch.clamp(x, min=self.min, max=self.max)


class SineScaled(nn.Module):
    """sin(w0 * x)."""

    def __init__(self, w0=1.0):
        super().__init__()
        self.w0 = w0

    def forward(self, x):
        return torch.sin(self.w0 * x)


def get_activation_class(activation_type):
    """The activation named ``activation_type``: 'none' / 'identity', 'relu', 'sin', 'sinescaled' (w0 = 30), 'sigmoid',
    'fullsort', 'minmax'. The reference's ``assert False and "..."`` on an unknown name is an AssertionError here too."""
    if activation_type in ("none", "identity"):
        return Identity()
    if activation_type == "fullsort":
        return FullSort()
    if activation_type == "minmax":
        return MinMax()
    if activation_type == "relu":
        return torch.relu
    if activation_type == "sin":
        return torch.sin
    if activation_type == "sinescaled":
        return SineScaled(30.0)
    if activation_type == "sigmoid":
        return torch.sigmoid
    raise AssertionError(f"activation type does not exist: {activation_type}")


__all__ = ["FullSort", "MinMax", "Identity", "Clamp", "SineScaled", "get_activation_class"]
