"""``Pipeline``: a neural field and the tracer that renders it (reference wisp/models/pipeline.py)."""
import torch.nn as nn


class Pipeline(nn.Module):
    """Holds ``nef`` (the field: coordinates -> signals) and ``tracer`` (the forward map that calls the field in its outer loop
    and returns a ``RenderBuffer``). A tracer that is not an ``nn.Module`` is kept as a plain attribute."""

    def __init__(self, nef, tracer=None):
        super().__init__()
        self.nef = nef
        self.tracer = tracer

    def forward(self, *args, **kwargs):
        """Through the tracer when there is one, else the field itself."""
        if self.tracer is not None:
            return self.tracer(self.nef, *args, **kwargs)
        return self.nef(*args, **kwargs)
