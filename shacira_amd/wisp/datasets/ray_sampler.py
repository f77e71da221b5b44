"""``SampleRays``: the reference's transform (wisp/datasets/transforms/ray_sampler.py) over one view's dict."""
import torch


class SampleRays:
    """Keeps ``num_samples`` random pixels of a view: ``rays``, ``rgb`` and ``masks`` (when present) indexed by one draw of
    ``torch.randint`` on the tensors' device (with replacement, as the reference draws)."""

    def __init__(self, num_samples):
        self.num_samples = num_samples

    def __call__(self, inputs):
        device = inputs["rays"].origins.device
        idx = torch.randint(0, inputs["rays"].origins.shape[0], [self.num_samples], device=device)
        out = dict(inputs)
        out["rays"] = inputs["rays"][idx]
        for key in ("rgb", "masks"):
            if key in inputs and inputs[key] is not None:
                out[key] = inputs[key][idx]
        return out
