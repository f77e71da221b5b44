"""Mirror of the reference's ``wisp/ops/grid.py`` (:69-196): the autograd wrappers and functional API of the
hash-grid operator, bound to the MI355X C-ABI instead of ``wisp._C``.

Kept from the reference, because callers depend on it:
  * ``HashGridInterpolate`` / ``HashGridInterpolate2D``: ``forward(ctx, coords, resolutions, codebook_bitwidth,
    lod_idx, codebook, codebook_sizes, codebook_first_idx)`` and a 7-tuple ``backward`` (grid.py:111, :176);
  * odd feature dims raise ``Exception("The codebook feature dimension needs to be a multiple of 2.")`` (grid.py:75);
  * ``lod_idx`` and ``codebook_sizes`` are accepted and ignored by the operator (grid.py:79 TODO);
  * autocast: float inputs are cast to fp16 when autocast is active (``custom_fwd(cast_inputs=torch.half)``, grid.py:73).

Not kept: ``hashgrid_naive`` (deprecated in the reference, needs kaolin, not numerically equivalent).
The reference saves the (decoded) codebook for backward although only its shape and dtype are used; we save those.

Added: the coordinate gradient. The reference's backward returns None for the coordinates (grid.py:111, its kernel's
branch is dead code); here slot 0 of ``backward`` carries dL/dcoords (fp32, ``hip_ops.hashgrid_coords_backward``) when the
coordinates require a gradient -- computed on the coordinates the forward used (under autocast the fp16-rounded ones). Only
then is the codebook saved as well, and the batch's plan is requested when either the codebook or the coordinates need a
gradient.

Added, opt-in: second order. By default a backward with ``create_graph=True`` that needs the coordinate gradient raises, as
before. Inside ``with second_order():`` (or after the plain call ``second_order(True)``) ``hashgrid`` / ``hashgrid2d`` -- and
through them ``HashGrid`` and ``LatentGrid`` -- route coordinates that require a gradient through ``HashGridInterpolateSO`` /
``HashGridInterpolate2DSO``: the same forward, and a backward whose coordinate gradient is itself differentiable
(``HashGridCoordsBackward``, backed by ``hip_ops.hashgrid_coords_backward2``) with respect to ``grad_output``, the codebook
and the coordinates -- what a loss on d(features)/d(coords) needs (eikonal, normal consistency, gradient matching). The switch
is read when ``hashgrid`` / ``hashgrid2d`` is called. Not covered: the double backward of the codebook gradient (differentiating
it raises), third order (raises), fp64 tables, the triplane and octree operators, and the fused MLP Functions of this package
(they are differentiable once: an eikonal term through a decoder needs a decoder made of torch layers).
"""
import torch

from ... import hip_ops


def _check_feature_dim(codebook):
    if codebook[0].shape[-1] % 2 == 1:
        raise Exception("The codebook feature dimension needs to be a multiple of 2.")


def _forward(ctx, dim, coords, resolutions, codebook_bitwidth, codebook, codebook_first_idx):
    _check_feature_dim(codebook)
    op = hip_ops.hashgrid_interpolate_cuda if dim == 3 else hip_ops.hashgrid_interpolate2d_cuda
    # the batch's plan (its samples sorted by spatial block: what the forward of a large batch computes first) is kept with
    # the coordinates the reference saves (grid.py:86), so that the backward does not have to rediscover the batch's layout
    plan = None
    need_coords = ctx.needs_input_grad[0]
    if coords.is_cuda and (ctx.needs_input_grad[4] or need_coords):   # (codebook is forward()'s fifth argument)
        plan = hip_ops.hashgrid_plan_buffer(dim, coords, codebook, resolutions, codebook_bitwidth)
    extra = {} if plan is None else {"plan": plan}   # (the operator's own signature when there is none: hashgrid_interpolate.h)
    feats_out = op(coords.float().contiguous(), codebook.contiguous(), codebook_first_idx, resolutions,
                   codebook_bitwidth, **extra).contiguous()
    if need_coords:   # the coordinate gradient reads the table's values; a caller that does not ask saves nothing more
        ctx.save_for_backward(coords, codebook_first_idx, codebook)
    else:
        ctx.save_for_backward(coords, codebook_first_idx)
    ctx.plan = plan
    ctx.resolutions = resolutions
    ctx.codebook_bitwidth = codebook_bitwidth
    ctx.feature_dim = codebook.shape[-1]
    ctx.table_rows = codebook.shape[0]
    ctx.table_dtype = codebook.dtype
    return feats_out


def _backward(ctx, dim, grad_output):
    if ctx.needs_input_grad[0] and torch.is_grad_enabled():
        raise RuntimeError("shacira_amd: the hash-grid operator has no second derivative: backward with "
                           "create_graph=True is not supported when the coordinates require a gradient (opt in with "
                           "shacira_amd.wisp.ops.grid.second_order())")
    return _backward_calls(ctx, dim, grad_output)


def _backward_calls(ctx, dim, grad_output):
    need_coords = ctx.needs_input_grad[0]
    if need_coords:
        coords, codebook_first_idx, codebook = ctx.saved_tensors
    else:
        coords, codebook_first_idx = ctx.saved_tensors
    grad_codebook = grad_coords = None
    if ctx.needs_input_grad[4]:
        grad_codebook = hip_ops.hashgrid_backward(dim, coords.float().contiguous(), grad_output.contiguous(),
                                                  ctx.table_rows, ctx.table_dtype, codebook_first_idx, ctx.resolutions,
                                                  ctx.codebook_bitwidth, ctx.feature_dim,
                                                  **({} if ctx.plan is None else {"plan": ctx.plan}))
    if need_coords:
        grad_coords = hip_ops.hashgrid_coords_backward(dim, coords.float().contiguous(), grad_output, codebook,
                                                       codebook_first_idx, ctx.resolutions, ctx.codebook_bitwidth,
                                                       plan=ctx.plan)
    return (grad_coords, None, None, None, grad_codebook, None, None)


class HashGridInterpolate(torch.autograd.Function):
    """3-D operator (reference grid.py:69-111)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.half)
    def forward(ctx, coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes, codebook_first_idx):
        return _forward(ctx, 3, coords, resolutions, codebook_bitwidth, codebook, codebook_first_idx)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        return _backward(ctx, 3, grad_output)


class HashGridInterpolate2D(torch.autograd.Function):
    """2-D operator (reference grid.py:135-176)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.half)
    def forward(ctx, coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes, codebook_first_idx):
        return _forward(ctx, 2, coords, resolutions, codebook_bitwidth, codebook, codebook_first_idx)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        return _backward(ctx, 2, grad_output)


# ---- second order (opt-in) -------------------------------------------------------------------------------------------------
_second_order = False


class second_order:
    """Switch for twice differentiable coordinate gradients, off by default. ``with second_order(): ...`` turns it on for the
    block and restores the previous state; the plain call ``second_order(True)`` / ``second_order(False)`` sets it. Read when
    ``hashgrid`` / ``hashgrid2d`` is called (module docstring)."""

    def __init__(self, enabled=True):
        global _second_order
        self.prev = _second_order
        _second_order = bool(enabled)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _second_order
        _second_order = self.prev
        return False


def second_order_enabled():
    return _second_order


class _RoundToHalf(torch.autograd.Function):
    """The fp16 rounding autocast applies to the coordinates, as fp32 values with a straight-through (identity, fp32)
    gradient: the first-order path's convention (``custom_fwd(cast_inputs=torch.half)`` + an fp32 coordinate gradient)."""

    @staticmethod
    def forward(ctx, coords):
        return coords.half().float()

    @staticmethod
    def backward(ctx, grad):
        return grad


class HashGridCoordsBackward(torch.autograd.Function):
    """``hip_ops.hashgrid_coords_backward`` as a differentiable node: its backward is ``hip_ops.hashgrid_coords_backward2``,
    asked only for what needs a gradient. Differentiable once (third order raises)."""

    @staticmethod
    def forward(ctx, coords, grad_output, codebook, codebook_first_idx, dim, resolutions, codebook_bitwidth, plan):
        ctx.save_for_backward(coords, grad_output, codebook, codebook_first_idx)
        ctx.dim, ctx.resolutions, ctx.codebook_bitwidth, ctx.plan = dim, resolutions, codebook_bitwidth, plan
        return hip_ops.hashgrid_coords_backward(dim, coords.float().contiguous(), grad_output, codebook, codebook_first_idx,
                                                resolutions, codebook_bitwidth, plan=plan)

    @staticmethod
    def backward(ctx, grad_grad_coords):
        coords, grad_output, codebook, codebook_first_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        with torch.no_grad():
            ggo, gcb, gc = hip_ops.hashgrid_coords_backward2(ctx.dim, coords.float().contiguous(), grad_output,
                                                             grad_grad_coords, codebook, codebook_first_idx,
                                                             ctx.resolutions, ctx.codebook_bitwidth,
                                                             want=(need[1], need[2], need[0]), plan=ctx.plan)
            if ggo is not None and ggo.dtype != grad_output.dtype:
                ggo = ggo.to(grad_output.dtype)
        grads = [gc, ggo, gcb]
        if torch.is_grad_enabled():       # create_graph=True once more: results that refuse a third differentiation
            live = [i for i, t in enumerate(grads) if t is not None]
            for i, t in zip(live, _NoThirdOrder.apply(grad_grad_coords, coords, grad_output, codebook,
                                                      *[grads[i] for i in live])):
                grads[i] = t
        return (*grads, None, None, None, None, None)


class _NoThirdOrder(torch.autograd.Function):
    """Passes the second-order results through; differentiating them raises."""

    @staticmethod
    def forward(ctx, grad_grad_coords, coords, grad_output, codebook, *results):
        return tuple(r.view_as(r) for r in results)

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("shacira_amd: third-order derivatives of the hash-grid operator are not implemented "
                           "(second_order() covers one more differentiation of the coordinate gradient)")


class _HashGridCodebookGrad(torch.autograd.Function):
    """The codebook gradient inside a ``create_graph=True`` backward: today's ``hip_ops.hashgrid_backward`` call, as a node
    that refuses to be differentiated again."""

    @staticmethod
    def forward(ctx, grad_output, coords, codebook_first_idx, dim, fctx):
        return hip_ops.hashgrid_backward(dim, coords.float().contiguous(), grad_output.contiguous(), fctx.table_rows,
                                         fctx.table_dtype, codebook_first_idx, fctx.resolutions, fctx.codebook_bitwidth,
                                         fctx.feature_dim, **({} if fctx.plan is None else {"plan": fctx.plan}))

    @staticmethod
    def backward(ctx, grad):
        raise RuntimeError("shacira_amd: the double backward of the hash-grid codebook gradient is not implemented: "
                           "second_order() makes the coordinate gradient differentiable, not the codebook gradient")


def _backward_second_order(ctx, dim, grad_output):
    if not torch.is_grad_enabled():       # create_graph=False: exactly the first-order calls
        return _backward_calls(ctx, dim, grad_output)
    coords, codebook_first_idx, codebook = ctx.saved_tensors
    grad_codebook = grad_coords = None
    if ctx.needs_input_grad[4]:
        grad_codebook = _HashGridCodebookGrad.apply(grad_output, coords, codebook_first_idx, dim, ctx)
    if ctx.needs_input_grad[0]:
        grad_coords = HashGridCoordsBackward.apply(coords, grad_output, codebook, codebook_first_idx, dim, ctx.resolutions,
                                                   ctx.codebook_bitwidth, ctx.plan)
    return (grad_coords, None, None, None, grad_codebook, None, None)


class HashGridInterpolateSO(torch.autograd.Function):
    """3-D operator with a twice differentiable coordinate gradient (``second_order``). No autocast handling of its own:
    ``hashgrid`` applies autocast's casts outside, where autograd sees them."""

    @staticmethod
    def forward(ctx, coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes, codebook_first_idx):
        return _forward(ctx, 3, coords, resolutions, codebook_bitwidth, codebook, codebook_first_idx)

    @staticmethod
    def backward(ctx, grad_output):
        return _backward_second_order(ctx, 3, grad_output)


class HashGridInterpolate2DSO(torch.autograd.Function):
    """2-D operator with a twice differentiable coordinate gradient (``second_order``)."""

    @staticmethod
    def forward(ctx, coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes, codebook_first_idx):
        return _forward(ctx, 2, coords, resolutions, codebook_bitwidth, codebook, codebook_first_idx)

    @staticmethod
    def backward(ctx, grad_output):
        return _backward_second_order(ctx, 2, grad_output)


def _apply(first_order, second, coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes,
           codebook_first_idx):
    if not (_second_order and coords.requires_grad and torch.is_grad_enabled()):
        return first_order.apply(coords.contiguous(), resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes,
                                 codebook_first_idx)
    if codebook.dtype == torch.float64:
        raise RuntimeError("shacira_amd: second_order() supports fp32 and fp16 tables, not torch.float64")
    if coords.is_cuda and torch.is_autocast_enabled("cuda"):
        # what custom_fwd(cast_inputs=torch.half) does to the first-order path's inputs, as differentiable steps
        if coords.dtype == torch.float32:
            coords = _RoundToHalf.apply(coords)
        if codebook.is_cuda and codebook.dtype == torch.float32:
            codebook = codebook.half()
    with torch.autocast("cuda", enabled=False):
        return second.apply(coords.contiguous(), resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes,
                            codebook_first_idx)


def hashgrid(coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes, codebook_first_idx):
    """3-D hash-grid query + trilinear interpolation: coords [N,3] -> features [N, F*L] (reference grid.py:113-131)."""
    batch, _ = coords.shape
    feats = _apply(HashGridInterpolate, HashGridInterpolateSO, coords, resolutions, codebook_bitwidth, lod_idx, codebook,
                   codebook_sizes, codebook_first_idx)
    return feats.reshape(batch, codebook.shape[1] * len(resolutions))


def hashgrid2d(coords, resolutions, codebook_bitwidth, lod_idx, codebook, codebook_sizes, codebook_first_idx):
    """2-D hash-grid query + bilinear interpolation: coords [N,2] -> features [N, F*L] (reference grid.py:178-196)."""
    batch, _ = coords.shape
    feats = _apply(HashGridInterpolate2D, HashGridInterpolate2DSO, coords, resolutions, codebook_bitwidth, lod_idx,
                   codebook, codebook_sizes, codebook_first_idx)
    return feats.reshape(batch, codebook.shape[1] * len(resolutions))
