"""Batches as the reference's ``wisp.datasets.batch`` defines them: dictionaries whose entries also read as attributes. Which
fields a batch carries depends on its dataset; an optional channel that is absent is present with the value None."""


class Batch(dict):
    """One batch sampled from a dataset: ``batch["coords"]`` and ``batch.coords`` are the same entry."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for k, v in dict(*args, **kwargs).items():
            self[k] = v

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value

    @property
    def fields(self):
        """The names of the fields the batch holds (some values may be None)."""
        return list(self.keys())


class SDFBatch(Batch):
    """Coordinates [B, 3] and their signed distances [B, 1], optionally the colour of the nearest surface point (``rgb``) and
    the surface normal (``normals``); None when the dataset does not carry them."""

    def __init__(self, coords, sdf, rgb=None, normals=None, *args, **kwargs):
        super().__init__(coords=coords, sdf=sdf, rgb=rgb, normals=normals)

    def coord_values(self):
        """The supervision channels of the coordinates that are present."""
        out = dict(sdf=self["sdf"])
        if self["rgb"] is not None:
            out["rgb"] = self["rgb"]
        if self["normals"] is not None:
            out["normals"] = self["normals"]
        return out
