"""Intersection over union of the inside sets of two signed-distance samplings (reference wisp/ops/sdf/metrics.py)."""
import torch


def compute_sdf_iou(pred: torch.Tensor, gts: torch.Tensor) -> float:
    """IoU in percent, 0 to 100, of {pred < 0} against {gts < 0}. When neither is negative anywhere the union is empty: the
    two agree everywhere and 100.0 is returned (the reference divides by zero there)."""
    inside_pred, inside_gts = pred < 0, gts < 0
    union = int((inside_pred | inside_gts).sum().item())
    if union == 0:
        return 100.0
    return 100.0 * int((inside_pred & inside_gts).sum().item()) / union


def compute_sparse_sdf_iou(nef, coords: torch.Tensor, gts: torch.Tensor, lod_idx=0) -> float:
    """The narrowband IoU of a sparse field: ``nef`` predicts where ``coords`` [N, 3] fall into cells of its grid, elsewhere the
    prediction counts as the truth ``gts`` [N, 1]. The reference queries the grid and the field with ``gts`` where it means
    ``coords``; the intent is restated here."""
    if getattr(nef, "grid", None) is None:
        raise Exception(f"{nef.__class__.__name__} is incompatible with this function.")
    pidx = nef.grid.query(coords).pidx        # the occupied cells of the grid's structure, at its finest level
    mask = pidx > -1
    pred = gts.clone()
    if bool(mask.any()):
        pred[mask] = nef(coords=coords[mask], pidx=pidx[mask], lod_idx=lod_idx, channels="sdf").to(pred.dtype)
    return compute_sdf_iou(pred, gts)
