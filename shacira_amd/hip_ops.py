"""Tensor-level wrappers over the C-ABI: PyTorch supplies device memory and the stream, nothing else.

These functions have the signatures of the reference's pybind11 operators
(``wisp._C.ops.hashgrid_interpolate[2d]_cuda`` / ``..._backward_cuda``, wisp/csrc/bindings.cpp:24-28 and
wisp/csrc/ops/hashgrid_interpolate.h:18-50) so ``wisp/ops/grid.py``-style callers read the same.
Inputs must live on a HIP device; there is no CPU path (RuntimeError otherwise).
"""
import collections
import ctypes
import functools
import threading
import weakref

import numpy as np
import torch

from . import _lib

_DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.float64: _lib.F64}


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ptr_array(tensors):     # per-plane / per-level pointers, copied into the kernel arguments by the library
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


@functools.lru_cache(maxsize=64)
def _res_array(resolutions):
    return (ctypes.c_int32 * len(resolutions))(*resolutions)


_warned = set()


def warn_unfused(what, why):
    """One warning per (what, why): a GPU tensor is about to take the torch-op chain instead of a fused HIP kernel."""
    key = (what, why)
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(f"shacira_amd: {what} runs as torch ops, not as the fused HIP kernel ({why})", RuntimeWarning,
                      stacklevel=3)


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("shacira_amd: operands must be on the MI355X (HIP) device; there is no CPU fallback")


def _check_coords(dim, coords):
    # the reference reads coords as a flat [N, dim] array without looking at its shape (a [N, 2] tensor handed to the
    # 3-D op is read past its end): a wrong shape is refused here instead of faulting on the device
    if coords.dim() != 2 or coords.shape[1] != dim or not coords.is_contiguous():
        raise RuntimeError(f"shacira_amd: coords must be a contiguous [N, {dim}] tensor for the {dim}-D operator, got "
                           f"{tuple(coords.shape)}")


def _check_float_coords(dim, coords, *others):
    _need_gpu(coords, *others)
    if coords.dtype != torch.float32:
        raise RuntimeError("expected scalar type Float for coords")  # data_ptr<float>() in the reference
    _check_coords(dim, coords)      # [N, dim], contiguous: the kernels read dim floats per sample


def _check_grad_output(grad_output, N, K):
    """``grad_output`` as the contiguous fp32 [N, K] tensor on the device that the triplane / octree backward reads."""
    if grad_output.dtype != torch.float32:
        grad_output = grad_output.float()
    grad_output = grad_output.contiguous()
    _need_gpu(grad_output)
    if tuple(grad_output.shape) != (N, K):
        raise RuntimeError(f"grad_output must be [{N}, {K}], got {tuple(grad_output.shape)}")
    return grad_output


# ---- scratch memory: one grow-only buffer per (device, stream, host thread) -----------------------------------------------
# The operators' workspaces (up to ~1 GB for a 2^20-sample backward) were a fresh torch.empty per call. Work one thread puts
# on one stream is ordered, so its calls can share one buffer that only grows. Per host THREAD, because an operator is several
# launches and ctypes drops the GIL: two threads on the same stream could interleave their launch sequences (the autograd
# engine's backward thread therefore gets a buffer of its own). Exceptions: while the stream is being captured into a HIP
# graph the buffer comes from the graph's own pool (a cached buffer could be replaced -- freed -- by a later, larger eager
# call while the graph still replays into it), and a caller-supplied workspace wins.
_tls = threading.local()     # per-thread: a thread's buffers are dropped with the thread (no entries of dead threads linger)


class _Scratch:
    """One thread's buffers: {(device, stream): [buffer, calls in a row that asked for less than a quarter of it]}."""
    __slots__ = ("buffers", "__weakref__")

    def __init__(self):
        self.buffers = {}


# every live thread's _Scratch (weak: a finished thread's entry goes with its thread-local storage), so that
# release_workspaces() can reach the gigabyte the autograd engine's backward thread holds (round-4 advisor finding)
_all_scratch = weakref.WeakSet()
_all_scratch_lock = threading.Lock()
_SHRINK_AFTER = 64           # calls in a row far below the buffer's size before it is given back


def _workspace(device, nbytes):
    if nbytes <= 0:
        return None
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((nbytes,), dtype=torch.uint8, device=device)
    scratch = getattr(_tls, "scratch", None)
    if scratch is None:
        scratch = _tls.scratch = _Scratch()
        with _all_scratch_lock:
            _all_scratch.add(scratch)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    entry = scratch.buffers.get(key)
    if entry is not None and entry[0].numel() >= nbytes:
        # retained memory is bounded in time, too: a buffer grown by one large call (1.1 GB for a 2^20-sample backward) is
        # given back once _SHRINK_AFTER calls in a row needed less than a quarter of it
        if nbytes * 4 < entry[0].numel():
            entry[1] += 1
            if entry[1] < _SHRINK_AFTER:
                return entry[0]
        else:
            entry[1] = 0
            return entry[0]
    scratch.buffers.pop(key, None)       # release the old buffer before the new one is allocated
    entry = None
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    scratch.buffers[key] = [buf, 0]
    return buf


def release_workspaces(all_threads=True):
    """Drop the cached scratch buffers (they go back to torch's caching allocator): the calling thread's, and -- by default
    -- every other thread's too (the autograd engine's backward thread keeps its own ~1 GB after a large backward). Call it
    between steps, not while another thread is inside an operator of this library. Returns the number of bytes released."""
    freed = 0
    with _all_scratch_lock:
        targets = list(_all_scratch) if all_threads else [getattr(_tls, "scratch", None)]
    for sc in targets:
        if sc is None:
            continue
        for key in list(sc.buffers):
            entry = sc.buffers.pop(key, None)
            if entry is not None:
                freed += entry[0].numel()
    return freed


def retained_workspace_bytes():
    """Bytes currently held in scratch buffers over all threads (what release_workspaces() would give back)."""
    with _all_scratch_lock:
        return sum(e[0].numel() for sc in list(_all_scratch) for e in list(sc.buffers.values()))


# workspace sizes are pure functions of the shape and the library's tunables: one C call per new shape, not per call
@functools.lru_cache(maxsize=4096)   # (NeRF steps change N every step: 256 entries thrashed)
def _grid_bytes(shape, query, epoch):
    return int(getattr(_lib.lib(), "shacira_hashgrid_" + query)(*shape.head(), shape.T, shape.dt))


class _GridShape(collections.namedtuple("_GridShape", "dim N L F bw res T dt")):
    """What every hash-grid entry point of the C ABI begins with, in that order, built once per operator call (``res``: a tuple)."""
    __slots__ = ()

    def head(self):
        """The leading C arguments, up to the resolutions array (``codebook_first_idx`` or ``table_rows`` come next)."""
        return (*self[:5], _res_array(self.res))

    def bytes(self, query):
        """``shacira_hashgrid_<query>`` of this shape (a size query), cached per shape and options epoch."""
        return _grid_bytes(self, query, _lib.options_epoch)


def _grid_shape(dim, N, resolution, codebook_bitwidth, T, F, dt):
    res = tuple(map(int, resolution))
    # (tuple.__new__, not _GridShape(...): one Python-level call less, on a path whose host cost shows in small batches)
    return tuple.__new__(_GridShape, (dim, N, len(res), F, int(codebook_bitwidth), res, T, dt))


def hashgrid_plan_bytes(dim, num_coords, table_rows, table_dtype, resolution, codebook_bitwidth, feature_dim):
    """Size of the plan buffer the forward of this shape fills (0: it sorts nothing -- pass ``plan=None``)."""
    return _grid_shape(dim, int(num_coords), resolution, codebook_bitwidth, int(table_rows), int(feature_dim),
                       _DTYPES[table_dtype]).bytes("plan_bytes")


def hashgrid_backward_workspace_bytes(dim, num_coords, table_rows, table_dtype, resolution, codebook_bitwidth, feature_dim,
                                      planned=False):
    """Scratch bytes of the backward of this shape; ``planned=True``: of a whole call that brings the batch's plan."""
    return _grid_shape(dim, int(num_coords), resolution, codebook_bitwidth, int(table_rows), int(feature_dim),
                       _DTYPES[table_dtype]).bytes("backward_planned_workspace_bytes" if planned
                                                   else "backward_workspace_bytes")


def hashgrid_plan_buffer(dim, coords, codebook, resolution, codebook_bitwidth):
    """A plan buffer for this batch and table (uint8 tensor), or None when the forward of this shape builds no plan. Pass it
    to the forward (``plan=``), keep it with the coordinates, pass it to the backward of the same batch."""
    n = hashgrid_plan_bytes(dim, coords.shape[0], codebook.shape[0], codebook.dtype, resolution, codebook_bitwidth,
                            codebook.shape[1])
    return torch.empty((n,), dtype=torch.uint8, device=codebook.device) if n > 0 else None


class _on_device:
    """`with torch.cuda.device(d)` only when d is not already current (the context manager costs ~4 us a call)."""
    __slots__ = ("ctx",)

    def __init__(self, device):
        self.ctx = None if torch.cuda.current_device() == device.index else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


def _dtype_code(t):
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise RuntimeError(f"shacira_amd: unsupported table dtype {t.dtype} (fp32, fp16 and fp64 are implemented)")


def _hashgrid_forward(dim, coords, codebook, codebook_first_idx, resolution, codebook_bitwidth, plan=None, plan_ready=False):
    _check_float_coords(dim, coords, codebook, codebook_first_idx)
    sh = _grid_shape(dim, coords.shape[0], resolution, codebook_bitwidth, codebook.shape[0], codebook.shape[1],
                     _dtype_code(codebook))
    feats = torch.empty((sh.N, sh.F * sh.L), dtype=codebook.dtype, device=codebook.device)
    L = _lib.lib()
    with _on_device(codebook.device):
        nbytes = sh.bytes("forward_workspace_bytes")
        if plan is not None:   # the workspace query includes a plan region for calls that bring none (shacira_hip.h)
            nbytes -= sh.bytes("plan_bytes")
        ws = _workspace(codebook.device, nbytes)
        if plan is None:
            rc = L.shacira_hashgrid_forward(*sh.head(), _ptr(codebook_first_idx), sh.T, _ptr(coords), _ptr(codebook),
                                            sh.dt, _ptr(feats), _ptr(ws), nbytes, _stream(codebook))
        else:
            _need_gpu(plan)
            rc = L.shacira_hashgrid_forward_planned(*sh.head(), _ptr(codebook_first_idx), sh.T, _ptr(coords),
                                                    _ptr(codebook), sh.dt, _ptr(feats), _ptr(plan), plan.numel(),
                                                    _lib.PLAN_READY if plan_ready else 0, _ptr(ws), nbytes,
                                                    _stream(codebook))
    _lib.check(rc, "hashgrid_interpolate")
    return feats


def hashgrid_backward(dim, coords, grad_output, table_rows, table_dtype, codebook_first_idx, resolution,
                      codebook_bitwidth, feature_dim, levels=None, out=None, workspace=None, flags=0, plan=None):
    """grad_codebook [table_rows, feature_dim] of ``table_dtype`` (the codebook's values are not needed).

    ``plan``: the buffer the forward of the SAME coordinate batch filled (``hashgrid_plan_buffer``); whole calls only.

    ``levels=(begin, end)`` computes (and overwrites) only the rows of those levels inside ``out`` (an existing
    gradient buffer) -- used to overlap the all-reduce of finished rows with the remaining levels. A series of such
    calls can share ``workspace`` (see ``backward_workspace``) with ``flags`` BWD_STAGE_ALL_LEVELS on the first and
    BWD_REUSE_STAGED on the following ones, so the gradients are transposed once."""
    _need_gpu(coords, grad_output, codebook_first_idx)
    _check_coords(dim, coords)
    if table_dtype not in _DTYPES:
        raise RuntimeError(f"shacira_amd: unsupported table dtype {table_dtype} (fp32, fp16 and fp64 are implemented)")
    sh = _grid_shape(dim, coords.shape[0], resolution, codebook_bitwidth, int(table_rows), int(feature_dim),
                     _DTYPES[table_dtype])
    whole = (0, sh.L)
    if grad_output.dtype != table_dtype:
        grad_output = grad_output.to(table_dtype)
    device = grad_output.device
    if out is not None:
        if tuple(out.shape) != (sh.T, sh.F) or out.dtype != table_dtype or not out.is_contiguous():
            raise RuntimeError("out must be a contiguous [table_rows, feature_dim] tensor of the table dtype")
        grad_codebook = out
    else:
        if levels is not None and tuple(levels) != whole:
            raise RuntimeError("a level range needs an existing `out` buffer (other rows are left untouched)")
        grad_codebook = torch.empty((sh.T, sh.F), dtype=table_dtype, device=device)
    lb, le = whole if levels is None else (int(levels[0]), int(levels[1]))
    L = _lib.lib()
    with _on_device(device):
        planned = plan is not None and (lb, le) == whole and not flags
        # (a planned call whose coarse levels go through the brick pass writes fewer, smaller items: its own query -- valid for
        # 16-byte aligned gradients, which every freshly allocated tensor is)
        nbytes = sh.bytes("backward_planned_workspace_bytes" if planned and grad_output.data_ptr() % 16 == 0
                          else "backward_workspace_bytes")
        if workspace is not None:
            if workspace.numel() * workspace.element_size() < nbytes:
                raise RuntimeError("workspace too small")
            ws = workspace
        elif levels is not None and tuple(levels) != whole:
            # a level-range call WITHOUT a shared workspace stages nothing for later calls: scratch of its own
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None
        else:
            ws = _workspace(device, nbytes)
        if planned:
            _need_gpu(plan)
            rc = L.shacira_hashgrid_backward_planned(*sh.head(), _ptr(codebook_first_idx), sh.T, _ptr(coords),
                                                     _ptr(grad_output), sh.dt, _ptr(grad_codebook), _ptr(plan),
                                                     plan.numel(), _ptr(ws), nbytes, _stream(grad_output))
        else:
            rc = L.shacira_hashgrid_backward_levels(*sh.head(), _ptr(codebook_first_idx), sh.T, _ptr(coords),
                                                    _ptr(grad_output), sh.dt, _ptr(grad_codebook), lb, le, int(flags),
                                                    _ptr(ws), nbytes, _stream(grad_output))
    _lib.check(rc, "hashgrid_interpolate_backward")
    return grad_codebook


def _table_operands(sh, codebook, grad_output):
    """The coordinate gradients' table and ``grad_output`` [N, L*F]: contiguous, the latter in the table's dtype."""
    if grad_output.dtype != codebook.dtype:
        grad_output = grad_output.to(codebook.dtype)
    grad_output = grad_output.contiguous()
    if tuple(grad_output.shape) != (sh.N, sh.L * sh.F):
        raise RuntimeError(f"grad_output must be [{sh.N}, {sh.L * sh.F}], got {tuple(grad_output.shape)}")
    return codebook.contiguous(), grad_output


def hashgrid_coords_backward(dim, coords, grad_output, codebook, codebook_first_idx, resolution, codebook_bitwidth,
                             plan=None):
    """Gradient of the features with respect to the coordinates: fp32 [N, dim] (include/shacira_hip.h,
    shacira_hashgrid_coords_backward). ``codebook`` is the table the forward read; ``grad_output`` [N, L*F] is taken in
    the table's dtype; ``plan``: the buffer the forward of the SAME coordinate batch filled, or None."""
    _check_float_coords(dim, coords, grad_output, codebook, codebook_first_idx)
    sh = _grid_shape(dim, coords.shape[0], resolution, codebook_bitwidth, codebook.shape[0], codebook.shape[1],
                     _dtype_code(codebook))
    codebook, grad_output = _table_operands(sh, codebook, grad_output)
    grad_coords = torch.empty((sh.N, dim), dtype=torch.float32, device=coords.device)
    with _on_device(coords.device):
        nbytes = sh.bytes("coords_backward_workspace_bytes")
        ws = _workspace(coords.device, nbytes)
        if plan is not None:
            _need_gpu(plan)
        rc = _lib.lib().shacira_hashgrid_coords_backward(*sh.head(), _ptr(codebook_first_idx), sh.T, _ptr(coords),
                                                         _ptr(codebook), _ptr(grad_output), sh.dt, _ptr(grad_coords),
                                                         _ptr(plan), 0 if plan is None else plan.numel(), _ptr(ws), nbytes,
                                                         _stream(coords))
    _lib.check(rc, "hashgrid_coords_backward")
    return grad_coords


def hashgrid_coords_backward2(dim, coords, grad_output, grad_grad_coords, codebook, codebook_first_idx, resolution,
                              codebook_bitwidth, want=(True, True, True), plan=None):
    """Backward of ``hashgrid_coords_backward`` for ``grad_grad_coords`` = dL/dgrad_coords (fp32 [N, dim]): the tuple
    (grad_grad_output [N, L*F] in the table's dtype, grad_codebook [T, F] in the table's dtype, grad_coords fp32 [N, dim]),
    ``None`` where ``want`` is false (include/shacira_hip.h, shacira_hashgrid_coords_backward2). fp32 and fp16 tables."""
    _check_float_coords(dim, coords, grad_output, grad_grad_coords, codebook, codebook_first_idx)
    want = tuple(bool(w) for w in want)
    if len(want) != 3:
        raise RuntimeError("want must have three entries: (grad_grad_output, grad_codebook, grad_coords)")
    if not any(want):
        return None, None, None
    if codebook.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"shacira_amd: the second-order hash-grid gradients are implemented for fp32 and fp16 tables, "
                           f"not {codebook.dtype}")
    sh = _grid_shape(dim, coords.shape[0], resolution, codebook_bitwidth, codebook.shape[0], codebook.shape[1],
                     _dtype_code(codebook))
    N, T, device = sh.N, sh.T, coords.device
    codebook, grad_output = _table_operands(sh, codebook, grad_output)
    v = grad_grad_coords
    if v.dtype != torch.float32:
        v = v.float()
    v = v.contiguous()
    if tuple(v.shape) != (N, dim):
        raise RuntimeError(f"grad_grad_coords must be [{N}, {dim}], got {tuple(v.shape)}")
    ggo = torch.empty((N, sh.L * sh.F), dtype=codebook.dtype, device=device) if want[0] else None
    gcb = torch.empty((T, sh.F), dtype=codebook.dtype, device=device) if want[1] else None
    gc = torch.empty((N, dim), dtype=torch.float32, device=device) if want[2] else None
    if N == 0 and (not want[1] or T == 0):     # nothing to compute, no table to zero
        return ggo, gcb, gc
    with _on_device(device):
        nbytes = sh.bytes("coords_backward2_workspace_bytes") if want[1] else 0
        ws = _workspace(device, nbytes)
        if plan is not None:
            _need_gpu(plan)
        rc = _lib.lib().shacira_hashgrid_coords_backward2(*sh.head(), _ptr(codebook_first_idx), T, _ptr(coords),
                                                          _ptr(codebook), _ptr(grad_output), _ptr(v), sh.dt, _ptr(ggo),
                                                          _ptr(gcb), _ptr(gc), _ptr(plan),
                                                          0 if plan is None else plan.numel(), _ptr(ws), nbytes,
                                                          _stream(coords))
    _lib.check(rc, "hashgrid_coords_backward2")
    return ggo, gcb, gc


def hashgrid_debug_corners(dim, coords, resolution, codebook_bitwidth):
    """Test hook: (rows int32 [N, L, 2^dim], weights fp32 [N, L, 2^dim]) exactly as the kernels compute them."""
    _check_float_coords(dim, coords)
    res = tuple(int(r) for r in resolution)
    N = coords.shape[0]
    rows = torch.empty((N, len(res), 1 << dim), dtype=torch.int32, device=coords.device)
    w = torch.empty((N, len(res), 1 << dim), dtype=torch.float32, device=coords.device)
    with _on_device(coords.device):
        rc = _lib.lib().shacira_hashgrid_debug_corners(dim, N, len(res), int(codebook_bitwidth), _res_array(res),
                                                       _ptr(coords), _ptr(rows), _ptr(w), _stream(coords))
    _lib.check(rc, "hashgrid_debug_corners")
    return rows, w


def backward_workspace(dim, num_coords, table_rows, table_dtype, resolution, codebook_bitwidth, feature_dim, device,
                       planned=False):
    """Scratch buffer a caller can share between several ``hashgrid_backward(..., levels=...)`` calls; ``planned=True``: the
    (smaller) buffer of whole calls that bring the batch's plan."""
    n = hashgrid_backward_workspace_bytes(dim, num_coords, table_rows, table_dtype, resolution, codebook_bitwidth,
                                          feature_dim, planned)
    return torch.empty((max(n, 1),), dtype=torch.uint8, device=device)


def hashgrid_interpolate_cuda(coords, codebook, codebook_first_idx, resolution, codebook_bitwidth, plan=None,
                              plan_ready=False):
    """hashgrid_interpolate.h:18-23 -> feats [N, L*F] (3-D coords). ``plan``: see ``hashgrid_plan_buffer``."""
    return _hashgrid_forward(3, coords, codebook, codebook_first_idx, resolution, codebook_bitwidth, plan, plan_ready)


def hashgrid_interpolate2d_cuda(coords, codebook, codebook_first_idx, resolution, codebook_bitwidth, plan=None,
                                plan_ready=False):
    """hashgrid_interpolate.h:35-40 -> feats [N, L*F] (2-D coords)."""
    return _hashgrid_forward(2, coords, codebook, codebook_first_idx, resolution, codebook_bitwidth, plan, plan_ready)


def hashgrid_interpolate_backward_cuda(coords, grad_output, codebook, codebook_first_idx, resolution,
                                       codebook_bitwidth, feature_dim, require_grad_coords):
    """hashgrid_interpolate.h:25-33 -> grad_codebook [T, F]."""
    return hashgrid_backward(3, coords, grad_output, codebook.shape[0], codebook.dtype, codebook_first_idx, resolution,
                             codebook_bitwidth, feature_dim)


def hashgrid_interpolate2d_backward_cuda(coords, grad_output, codebook, codebook_first_idx, resolution,
                                         codebook_bitwidth, feature_dim, require_grad_coords):
    """hashgrid_interpolate.h:42-50 -> grad_codebook [T, F]."""
    return hashgrid_backward(2, coords, grad_output, codebook.shape[0], codebook.dtype, codebook_first_idx, resolution,
                             codebook_bitwidth, feature_dim)


# ------------------------------------------------------------------------------------------------ latent path
def latent_decode_supported(latent_dim, feature_dim):
    return latent_dim in (1, 2, 3, 4, 8) and feature_dim in (1, 2, 4, 8) and not (latent_dim == 8 and feature_dim == 1)


def _latent_workspace(device):
    """fp64 block partials of the table reductions: a fresh buffer per call (the caching allocator makes that cheap).
    A buffer cached per stream would be shared by two host threads working on that stream -- A.kernel, B.kernel,
    A.finish reduces B's partials -- and could be captured into a graph pool and then reused eagerly."""
    n = _lib.lib().shacira_entropy_bits_workspace_bytes(0, 1)
    return torch.empty((n,), dtype=torch.uint8, device=device)


def _check_device_scalar(t, device):
    if t.device != device or t.dtype != torch.float32 or t.numel() != 1:
        raise RuntimeError("a device-side temperature must be one fp32 value on the table's device")


def _offsets_array(offsets):
    return (ctypes.c_int64 * len(offsets))(*[int(o) for o in offsets])


def _decode_entry(name, latent, F, offsets, sga):
    """-> (the C entry point ``shacira_<name>``, its arguments ahead of ``div``). ``offsets`` (host ints, [L+1]) selects the
    per-level ABI; ``sga`` is None (plain ABI) or (uniforms, temperature, diff_sampling). Without ``offsets`` the temperature
    may be one fp32 value in device memory (graph-captured steps anneal it between replays): the ``_tdev`` entry point."""
    T, ld = latent.shape
    args = (T, ld, F, _ptr(latent))
    if offsets is not None:
        args = (len(offsets) - 1, _offsets_array(offsets)) + args
    if sga is not None:
        uniforms, temperature, diff_sampling = sga
        if offsets is None and torch.is_tensor(temperature):
            _check_device_scalar(temperature, latent.device)
            name, temperature = name + "_tdev", _ptr(temperature)
        else:
            temperature = float(temperature)
        args += (_ptr(uniforms), temperature, int(bool(diff_sampling)))
    return getattr(_lib.lib(), "shacira_" + name), args


def _decode_forward(name, latent, offsets, sga, div, matrix, colscale, shift, clamp_weights):
    uniforms = sga[0] if sga is not None else None
    _need_gpu(latent, uniforms, div, matrix, colscale, shift)
    T, ld = latent.shape
    F = matrix.shape[-1]
    if offsets is None and sga is not None and (tuple(uniforms.shape) != (T, ld, 2) or uniforms.dtype != torch.float32
                                                or not uniforms.is_contiguous()):
        raise RuntimeError("uniforms must be a contiguous fp32 [rows, latent_dim, 2] tensor")
    out = torch.empty((T, F), dtype=torch.float32, device=latent.device)
    with _on_device(latent.device):
        fn, args = _decode_entry(name, latent, F, offsets, sga)
        rc = fn(*args, _ptr(div), _ptr(matrix), _ptr(colscale), _ptr(shift), float(clamp_weights), _ptr(out),
                _stream(latent))
    _lib.check(rc, name)
    return out


def _decode_backward(name, latent, offsets, sga, div, matrix, colscale, shift, clamp_weights, grad_decoded, need_colscale):
    """-> grad_latent [T, ld], grad_matrix [ld, F], grad_colscale [F] or None, grad_shift [F]; per level ([L, ...]) with
    ``offsets``."""
    _need_gpu(latent, sga[0] if sga is not None else None, grad_decoded)
    ld, F = latent.shape[1], matrix.shape[-1]
    lead = () if offsets is None else (len(offsets) - 1,)
    dev = latent.device
    g_lat = torch.empty_like(latent)
    g_mat = torch.empty(lead + (ld, F), dtype=torch.float32, device=dev)
    g_cs = torch.empty(lead + (F,), dtype=torch.float32, device=dev) if need_colscale else None
    g_sh = torch.empty(lead + (F,), dtype=torch.float32, device=dev)
    with _on_device(dev):
        ws = _latent_workspace(dev)
        fn, args = _decode_entry(name, latent, F, offsets, sga)
        rc = fn(*args, _ptr(div), _ptr(matrix), _ptr(colscale), _ptr(shift), float(clamp_weights), _ptr(grad_decoded),
                _ptr(g_lat), _ptr(g_mat), _ptr(g_cs), _ptr(g_sh), _ptr(ws), ws.numel(), _stream(latent))
    _lib.check(rc, name)
    return g_lat, g_mat, g_cs, g_sh


def latent_decode_forward(latent, div, matrix, colscale, shift, clamp_weights):
    return _decode_forward("latent_decode_forward", latent, None, None, div, matrix, colscale, shift, clamp_weights)


def latent_decode_backward(latent, div, matrix, colscale, shift, clamp_weights, grad_decoded, need_colscale):
    return _decode_backward("latent_decode_backward", latent, None, None, div, matrix, colscale, shift, clamp_weights,
                            grad_decoded, need_colscale)


def latent_decode_sga_forward(latent, uniforms, temperature, diff_sampling, div, matrix, colscale, shift, clamp_weights):
    """SGA sample (reference basic_latent_decoder.py:183-191) + decode in one kernel; ``uniforms`` [T, ld, 2]."""
    return _decode_forward("latent_decode_sga_forward", latent, None, (uniforms, temperature, diff_sampling), div, matrix,
                           colscale, shift, clamp_weights)


def latent_decode_sga_backward(latent, uniforms, temperature, diff_sampling, div, matrix, colscale, shift, clamp_weights,
                               grad_decoded, need_colscale):
    return _decode_backward("latent_decode_sga_backward", latent, None, (uniforms, temperature, diff_sampling), div, matrix,
                            colscale, shift, clamp_weights, grad_decoded, need_colscale)


def latent_decode_levels_forward(latent, offsets, uniforms, temperature, diff_sampling, div, matrix, colscale, shift,
                                 clamp_weights):
    """Per-level decoders in one launch: ``offsets`` (host ints, [L+1]) bound the levels' rows; ``div`` [L, ld],
    ``matrix`` [L, ld, F], ``colscale`` / ``shift`` [L, F] or None; ``uniforms`` [T, ld, 2] selects the SGA path."""
    return _decode_forward("latent_decode_levels_forward", latent, offsets, (uniforms, temperature, diff_sampling), div,
                           matrix, colscale, shift, clamp_weights)


def latent_decode_levels_backward(latent, offsets, uniforms, temperature, diff_sampling, div, matrix, colscale, shift,
                                  clamp_weights, grad_decoded):
    return _decode_backward("latent_decode_levels_backward", latent, offsets, (uniforms, temperature, diff_sampling), div,
                            matrix, colscale, shift, clamp_weights, grad_decoded, colscale is not None)


LATENT_ACTIVATIONS = {"none": 0, "sigmoid": 1, "tanh": 2, "relu": 3, "sine": 4}   # SHACIRA_ACT_*


def _widths_array(widths):
    return (ctypes.c_int32 * len(widths))(*[int(w) for w in widths])


def latent_mlp_supported(widths):
    """Hidden-layer latent decoder (shacira_latent_mlp_*): ``widths`` = (latent_dim, hidden..., feature_dim)."""
    return len(widths) >= 2 and bool(_lib.lib().shacira_latent_mlp_supported(len(widths) - 1, _widths_array(widths)))


def _check_mlp_operands(latent, uniforms, div, params, widths):
    _need_gpu(latent, uniforms, div, params)
    # the kernels read latent as float[rows * ld] and div as float[ld]: anything else would read garbage or out of bounds
    if latent.dim() != 2 or latent.dtype != torch.float32 or not latent.is_contiguous():
        raise RuntimeError("latent must be a contiguous fp32 [rows, latent_dim] tensor")
    if div.dtype != torch.float32 or not div.is_contiguous():
        raise RuntimeError("div must be a contiguous fp32 vector of latent_dim elements")
    T, ld = latent.shape
    if ld != widths[0] or div.numel() != ld:
        raise RuntimeError("latent / div do not match widths[0]")
    want = sum(a * b + b for a, b in zip(widths[:-1], widths[1:]))
    if params.numel() != want or params.dtype != torch.float32 or not params.is_contiguous():
        raise RuntimeError(f"params must be a contiguous fp32 vector of {want} elements (W_k then b_k per layer)")
    if uniforms is not None and (tuple(uniforms.shape) != (T, ld, 2) or uniforms.dtype != torch.float32
                                 or not uniforms.is_contiguous()):
        raise RuntimeError("uniforms must be a contiguous fp32 [rows, latent_dim, 2] tensor")
    return T


def latent_mlp_forward(latent, uniforms, temperature, diff_sampling, div, params, widths, activation, final_activation,
                       clamp_weights):
    """decoded [T, widths[-1]] = clamp(final_act(MLP(q(latent) / div))): one kernel (reference basic_latent_decoder.py:182-198
    with hidden layers). ``params``: per layer the effective matrix [in, out] row-major, then the shift [out]."""
    T = _check_mlp_operands(latent, uniforms, div, params, widths)
    out = torch.empty((T, widths[-1]), dtype=torch.float32, device=latent.device)
    with _on_device(latent.device):
        rc = _lib.lib().shacira_latent_mlp_forward(
            T, len(widths) - 1, _widths_array(widths), _ptr(latent), _ptr(uniforms), float(temperature),
            int(bool(diff_sampling)), _ptr(div), _ptr(params), LATENT_ACTIVATIONS[activation],
            LATENT_ACTIVATIONS[final_activation], float(clamp_weights), _ptr(out), _stream(latent))
    _lib.check(rc, "latent_mlp_forward")
    return out


def latent_mlp_backward(latent, uniforms, temperature, diff_sampling, div, params, widths, activation, final_activation,
                        clamp_weights, grad_decoded):
    """-> (grad_latent [T, ld], grad_params packed like ``params``)."""
    T = _check_mlp_operands(latent, uniforms, div, params, widths)
    _need_gpu(grad_decoded)
    if tuple(grad_decoded.shape) != (T, widths[-1]) or grad_decoded.dtype != torch.float32 or not grad_decoded.is_contiguous():
        raise RuntimeError("grad_decoded must be a contiguous fp32 [rows, feature_dim] tensor")
    dev = latent.device
    g_lat = torch.empty_like(latent)
    g_par = torch.empty_like(params)
    wa = _widths_array(widths)
    with _on_device(dev):
        n = _lib.lib().shacira_latent_mlp_backward_workspace_bytes(len(widths) - 1, wa)
        ws = torch.empty((n,), dtype=torch.uint8, device=dev)
        rc = _lib.lib().shacira_latent_mlp_backward(
            T, len(widths) - 1, wa, _ptr(latent), _ptr(uniforms), float(temperature), int(bool(diff_sampling)), _ptr(div),
            _ptr(params), LATENT_ACTIVATIONS[activation], LATENT_ACTIVATIONS[final_activation], float(clamp_weights),
            _ptr(grad_decoded), _ptr(g_lat), _ptr(g_par), _ptr(ws), ws.numel(), _stream(latent))
    _lib.check(rc, "latent_mlp_backward")
    return g_lat, g_par


def latent_multi_supported(latent_dim, feature_dim, num_decoders):
    return bool(_lib.lib().shacira_latent_multi_supported(int(latent_dim), int(feature_dim), int(num_decoders)))


def latent_multi_decode_forward(latent, alpha, uniforms, temperature, straight_through, diff_sampling, div, scale, dft,
                                shift, clamp_weights):
    """MultiLatentDecoder in one kernel: alpha [K, T], scale [K, S, F], dft [ld, F] or None, shift [K, F] or None."""
    _need_gpu(latent, alpha, uniforms, div, scale, dft, shift)
    T, ld = latent.shape
    K, F = scale.shape[0], scale.shape[-1]
    out = torch.empty((T, F), dtype=torch.float32, device=latent.device)
    with _on_device(latent.device):
        rc = _lib.lib().shacira_latent_multi_decode_forward(
            T, ld, F, K, _ptr(latent), _ptr(alpha), _ptr(uniforms), float(temperature), int(bool(straight_through)),
            int(bool(diff_sampling)), _ptr(div), _ptr(scale), _ptr(dft), _ptr(shift), float(clamp_weights), _ptr(out),
            _stream(latent))
    _lib.check(rc, "latent_multi_decode_forward")
    return out


def latent_multi_decode_backward(latent, alpha, uniforms, temperature, straight_through, diff_sampling, div, scale, dft,
                                 shift, clamp_weights, grad_decoded):
    _need_gpu(latent, alpha, grad_decoded)
    T, ld = latent.shape
    K, F = scale.shape[0], scale.shape[-1]
    dev = latent.device
    g_lat = torch.empty_like(latent)
    g_alpha = torch.empty_like(alpha)
    g_scale = torch.empty_like(scale)
    g_shift = torch.empty((K, F), dtype=torch.float32, device=dev) if shift is not None else None
    with _on_device(dev):
        ws = _latent_workspace(dev)
        rc = _lib.lib().shacira_latent_multi_decode_backward(
            T, ld, F, K, _ptr(latent), _ptr(alpha), _ptr(uniforms), float(temperature), int(bool(straight_through)),
            int(bool(diff_sampling)), _ptr(div), _ptr(scale), _ptr(dft), _ptr(shift), float(clamp_weights),
            _ptr(grad_decoded), _ptr(g_lat), _ptr(g_alpha), _ptr(g_scale), _ptr(g_shift), _ptr(ws), ws.numel(),
            _stream(latent))
    _lib.check(rc, "latent_multi_decode_backward")
    return g_lat, g_alpha, g_scale, g_shift


def entropy_supported(latent_dim):
    return latent_dim in (1, 2, 3, 4, 8)


def entropy_bits_forward(latent, noise, params, num_layers):
    _need_gpu(latent, noise, params)
    T, ld = latent.shape
    dev = latent.device
    total = torch.empty((), dtype=torch.float32, device=dev)
    with _on_device(dev):
        ws = _latent_workspace(dev)
        rc = _lib.lib().shacira_entropy_bits_forward(T, ld, int(num_layers), _ptr(latent), _ptr(noise), _ptr(params),
                                                     _ptr(total), _ptr(ws), ws.numel(), _stream(latent))
    _lib.check(rc, "entropy_bits_forward")
    return total


def entropy_bits_backward(latent, noise, params, num_layers, grad_total, need_latent=True):
    _need_gpu(latent, noise, params, grad_total)
    T, ld = latent.shape
    dev = latent.device
    g_lat = torch.empty_like(latent) if need_latent else None
    g_par = torch.empty((4, 3, ld), dtype=torch.float32, device=dev)
    with _on_device(dev):
        ws = _latent_workspace(dev)
        rc = _lib.lib().shacira_entropy_bits_backward(T, ld, int(num_layers), _ptr(latent), _ptr(noise), _ptr(params),
                                                      _ptr(grad_total), _ptr(g_lat), _ptr(g_par), _ptr(ws), ws.numel(),
                                                      _stream(latent))
    _lib.check(rc, "entropy_bits_backward")
    return g_lat, g_par


# ------------------------------------------------------------------------------------------------ decoder MLP (a14)
def mlp_supported(in_dim, hidden_dim, num_hidden, out_dim):
    return bool(_lib.lib().shacira_mlp_supported(int(in_dim), int(hidden_dim), int(num_hidden), int(out_dim)))


def _mlp_rows(x, in_dim):
    """The kernels move rows of 4n floats as 16-byte vectors (the C-ABI refuses a pointer that is not 16-byte aligned then): a
    view that starts elsewhere, as a slice of a flat buffer does, is copied into an allocation of its own."""
    if in_dim % 4 == 0 and x.data_ptr() % 16 != 0:
        return x.clone(memory_format=torch.contiguous_format)
    return x


def mlp_forward(x, params, in_dim, hidden_dim, num_hidden, out_dim):
    _need_gpu(x, params)
    x = _mlp_rows(x, in_dim)
    y = torch.empty((x.shape[0], out_dim), dtype=torch.float32, device=x.device)
    with _on_device(x.device):
        rc = _lib.lib().shacira_mlp_forward(x.shape[0], in_dim, hidden_dim, num_hidden, out_dim, _ptr(x), _ptr(params),
                                            _ptr(y), _stream(x))
    _lib.check(rc, "mlp_forward")
    return y


def mlp_backward(x, params, grad_y, in_dim, hidden_dim, num_hidden, out_dim, need_grad_x=True):
    _need_gpu(x, params, grad_y)
    dev = x.device
    x = _mlp_rows(x, in_dim)
    gx = torch.empty(x.shape, dtype=torch.float32, device=dev) if need_grad_x else None
    gp = torch.empty(params.shape, dtype=torch.float32, device=dev)
    L = _lib.lib()
    with _on_device(dev):
        n = L.shacira_mlp_backward_workspace_bytes(in_dim, hidden_dim, num_hidden, out_dim)
        ws = torch.empty((n,), dtype=torch.uint8, device=dev)
        rc = L.shacira_mlp_backward(x.shape[0], in_dim, hidden_dim, num_hidden, out_dim, _ptr(x), _ptr(params),
                                    _ptr(grad_y), _ptr(gx), _ptr(gp), _ptr(ws), n, _stream(x))
    _lib.check(rc, "mlp_backward")
    return gx, gp


# ---------------------------------------------------------------------------------------------- symbol statistics
def symbols_supported(latent_dim):
    return 1 <= latent_dim <= 16


def latent_symbol_counts(latent):
    """Per-channel histogram of ``round(latent)`` (half to even, as ``torch.round``).

    Returns ``(lo, counts)``: ``lo`` int64 [ld] on the host = smallest symbol per channel, ``counts`` int64
    [ld, nbins] on the device with ``counts[c, k]`` = rows whose rounded value in channel c is ``lo[c] + k``
    (trailing bins of narrower channels are 0). Replaces ``torch.unique(return_counts=True)`` of
    LatentGrid.size (reference latent_grid.py:141-143); one host read-back of 2*ld integers sizes the bins."""
    _need_gpu(latent)
    if latent.dtype != torch.float32 or latent.dim() != 2:
        raise RuntimeError("latent_symbol_counts: expected an fp32 [rows, latent_dim] tensor")
    latent = latent.detach().contiguous()
    rows, ld = latent.shape
    L = _lib.lib()
    with _on_device(latent.device):
        minmax = torch.empty((ld, 2), dtype=torch.int32, device=latent.device)
        _lib.check(L.shacira_latent_symbol_range(rows, ld, _ptr(latent), _ptr(minmax), _stream(latent)),
                   "shacira_latent_symbol_range")
        mm = minmax.cpu()
        if rows == 0:
            return torch.zeros(ld, dtype=torch.int64), torch.zeros((ld, 1), dtype=torch.int64, device=latent.device)
        nbins = int((mm[:, 1].long() - mm[:, 0].long()).max().item()) + 1
        counts = torch.empty((ld, nbins), dtype=torch.int64, device=latent.device)  # kernel writes uint64, < 2^63
        _lib.check(L.shacira_latent_symbol_histogram(rows, ld, _ptr(latent), _ptr(minmax), nbins, _ptr(counts),
                                                     _stream(latent)), "shacira_latent_symbol_histogram")
    return mm[:, 0].long(), counts


def _rans_host_arrays(lo, nbins, payload, words):
    ld = len(nbins)
    return ((ctypes.c_int32 * ld)(*[int(v) for v in lo]), (ctypes.c_int32 * ld)(*[int(v) for v in nbins]),
            (ctypes.c_int64 * ld)(*[int(v) for v in payload]), (ctypes.c_int64 * ld)(*[int(v) for v in words]))


def latent_rans_encode(latent, lo, nbins, cdf, steps):
    """rans64 channel payloads of ``round(latent)`` (include/shacira_hip.h, "Interleaved rANS"), coded on the device.

    ``latent`` fp32 [rows, ld] on the GPU; ``lo`` / ``nbins`` per channel (host); ``cdf`` uint32 numpy [ld, stride] with
    ``cdf[c, :nbins[c] + 1]`` the channel's cumulative frequencies. Returns one ``bytes`` per channel (empty for
    channels with fewer than two bins). The kernels read the fp32 table itself; one read-back of the per-block word
    counts sizes the output, one copy brings the packed payloads to the host."""
    _need_gpu(latent)
    if latent.dtype != torch.float32 or latent.dim() != 2:
        raise RuntimeError("latent_rans_encode: expected an fp32 [rows, latent_dim] tensor")
    latent = latent.detach().contiguous()
    rows, ld = latent.shape
    if rows == 0:
        return [b""] * ld
    steps = int(steps)
    nblocks = -(-rows // (64 * steps))
    dev = latent.device
    cdf = np.ascontiguousarray(cdf, dtype=np.uint32)
    L = _lib.lib()
    with _on_device(dev):
        cdf_dev = torch.from_numpy(cdf.view(np.int32)).to(dev)
        counts = torch.empty((ld, nblocks), dtype=torch.int32, device=dev)
        states = torch.empty((ld, nblocks, 64), dtype=torch.int32, device=dev)
        slots = torch.empty((ld, nblocks, 64 * steps), dtype=torch.int16, device=dev)
        lo_h, nb_h, _, _ = _rans_host_arrays(lo, nbins, [0] * ld, [0] * ld)
        _lib.check(L.shacira_latent_rans_encode(rows, ld, _ptr(latent), lo_h, nb_h, _ptr(cdf_dev), cdf.shape[1], steps,
                                                _ptr(counts), _ptr(states), _ptr(slots), _stream(latent)),
                   "shacira_latent_rans_encode")
        n_b = counts.cpu().numpy().astype(np.int64)                  # the one read-back: sizes the output
        words = n_b.sum(axis=1)
        start = np.cumsum(n_b, axis=1) - n_b
        sizes = [260 * nblocks + 2 * int(words[c]) if nbins[c] >= 2 else 0 for c in range(ld)]
        offsets = np.concatenate([[0], np.cumsum([-(-s // 4) * 4 for s in sizes])])
        out = torch.zeros(max(int(offsets[-1]), 4), dtype=torch.uint8, device=dev)
        start_dev = torch.from_numpy(np.ascontiguousarray(start)).to(dev)
        _, _, off_h, words_h = _rans_host_arrays(lo, nbins, offsets[:ld], words)
        _lib.check(L.shacira_latent_rans_pack(rows, ld, nb_h, steps, _ptr(counts), _ptr(states), _ptr(slots),
                                              _ptr(start_dev), off_h, words_h, _ptr(out), out.numel(), _stream(latent)),
                   "shacira_latent_rans_pack")
        host = out.cpu().numpy()
    return [host[int(offsets[c]):int(offsets[c]) + sizes[c]].tobytes() for c in range(ld)]


def latent_rans_decode(container, rows, ld, lo, nbins, payload_offsets, words, cdf, block_start, steps, device):
    """Decode a version-2 ("rans64") container on ``device``: fp32 [rows, ld] tensor of symbol + lo.

    ``container``: the container's bytes (uploaded as they are); per channel (host) ``lo``, ``nbins``, byte offset of its
    payload and number of 16-bit words; ``cdf`` uint32 numpy [ld, stride]; ``block_start`` int64 numpy [ld, nblocks] =
    exclusive prefix of each channel's per-block word counts. The caller (codec.decompress_latents) has checked the
    header against the container's size. Raises ValueError when the kernel reports an inconsistent stream."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("shacira_amd: latent_rans_decode runs on the MI355X (HIP) device")
    out = torch.empty((rows, ld), dtype=torch.float32, device=device)
    if rows == 0:
        return out
    cdf = np.ascontiguousarray(cdf, dtype=np.uint32)
    L = _lib.lib()
    with _on_device(device):
        data = torch.frombuffer(bytearray(container), dtype=torch.uint8).to(device)
        cdf_dev = torch.from_numpy(cdf.view(np.int32)).to(device)
        start_dev = torch.from_numpy(np.ascontiguousarray(block_start, dtype=np.int64)).to(device)
        error = torch.zeros(1, dtype=torch.int32, device=device)
        lo_h, nb_h, off_h, words_h = _rans_host_arrays(lo, nbins, payload_offsets, words)
        _lib.check(L.shacira_latent_rans_decode(rows, ld, _ptr(data), data.numel(), lo_h, nb_h, off_h, words_h,
                                                _ptr(cdf_dev), cdf.shape[1], _ptr(start_dev), int(steps), _ptr(out),
                                                _ptr(error), _stream(out)), "shacira_latent_rans_decode")
        if int(error.item()) != 0:
            raise ValueError("corrupt rans64 payload: the stream does not return to its initial state")
    return out


# ---- triplanes (include/shacira_hip.h, shacira_triplane_*) -----------------------------------------------------------------
def _triplane_shape(coords, lods, planes):
    _check_float_coords(3, coords, *planes)
    lods = tuple(int(l) for l in lods)
    if len(planes) != 3 * len(lods):
        raise RuntimeError(f"shacira_amd: {len(lods)} LODs need {3 * len(lods)} planes, got {len(planes)}")
    fdim = planes[0].shape[1] if planes[0].dim() == 4 else -1
    for l, lod in enumerate(lods):
        side = (1 << lod) + 1 if lod >= 0 else 0
        for p in planes[3 * l:3 * l + 3]:
            if (p.dtype != torch.float32 or tuple(p.shape) != (1, fdim, side, side) or not p.is_contiguous()
                    or p.device != coords.device):
                raise RuntimeError(f"shacira_amd: LOD {l} planes must be contiguous fp32 [1, {fdim}, {side}, {side}] on "
                                   f"{coords.device}, got {p.dtype} {tuple(p.shape)}")
    return lods, fdim


def triplane_forward(coords, lods, planes, multiscale_sum):
    """Features of the triplanes at ``coords`` [N, 3] fp32: [N, 3F] (``multiscale_sum``) or [N, len(lods) * 3F].

    ``planes``: the 3 * len(lods) NCHW plane parameters [1, F, 2^lod + 1, 2^lod + 1], ordered fmx, fmy, fmz per LOD."""
    lods, fdim = _triplane_shape(coords, lods, planes)
    N = coords.shape[0]
    K = 3 * fdim if multiscale_sum else 3 * fdim * len(lods)
    feats = torch.empty((N, K), dtype=torch.float32, device=coords.device)
    L = _lib.lib()
    la = _res_array(lods)
    with _on_device(coords.device):
        nbytes = int(L.shacira_triplane_forward_workspace_bytes(N, len(lods), la, fdim, int(bool(multiscale_sum))))
        ws = _workspace(coords.device, nbytes)
        rc = L.shacira_triplane_forward(N, len(lods), la, fdim, _ptr(coords), _ptr_array(planes),
                                        int(bool(multiscale_sum)), _ptr(feats), _ptr(ws), nbytes, _stream(coords))
    _lib.check(rc, "triplane_forward")
    return feats


def triplane_backward(coords, lods, feature_dim, grad_output, multiscale_sum, planes=None, need_planes=True,
                      need_coords=False):
    """(plane gradients: one fp32 [1, F, S, S] tensor per plane, or None; coordinate gradient fp32 [N, 3], or None).

    ``planes`` (the forward's planes) are needed, and their values read, only when ``need_coords``. The plane gradients
    come from float atomics: two runs differ in the last bits."""
    lods = tuple(int(l) for l in lods)
    fdim = int(feature_dim)
    if need_coords:
        lods, fdim = _triplane_shape(coords, lods, planes)
    else:
        _check_float_coords(3, coords)
        if min(lods, default=-1) < 0:
            raise RuntimeError("shacira_amd: triplane LODs must be >= 0")
    N = coords.shape[0]
    K = 3 * fdim if multiscale_sum else 3 * fdim * len(lods)
    grad_output = _check_grad_output(grad_output, N, K)
    flags = (_lib.TRIPLANE_GRAD_PLANES if need_planes else 0) | (_lib.TRIPLANE_GRAD_COORDS if need_coords else 0)
    if not flags:
        return None, None
    dev = coords.device
    grads = None
    if need_planes:
        grads = [torch.empty((1, fdim, (1 << lod) + 1, (1 << lod) + 1), dtype=torch.float32, device=dev)
                 for lod in lods for _ in range(3)]
    grad_coords = torch.empty((N, 3), dtype=torch.float32, device=dev) if need_coords else None
    L = _lib.lib()
    la = _res_array(lods)
    with _on_device(dev):
        nbytes = int(L.shacira_triplane_backward_workspace_bytes(N, len(lods), la, fdim, int(bool(multiscale_sum)),
                                                                 flags))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_triplane_backward(N, len(lods), la, fdim, _ptr(coords),
                                         _ptr_array(planes) if need_coords else None, _ptr(grad_output),
                                         int(bool(multiscale_sum)), flags,
                                         _ptr_array(grads) if grads is not None else None, _ptr(grad_coords),
                                         _ptr(ws), nbytes, _stream(coords))
    _lib.check(rc, "triplane_backward")
    return grads, grad_coords


# ---- octree grids (include/shacira_hip.h, shacira_octree_*) ----------------------------------------------------------------
def _octree_shape(coords, levels, tables, fdim=None):
    """``levels``: one ``wisp.ops.octree.OctreeLevelIndex`` per level, on the coordinates' device."""
    _check_float_coords(3, coords)
    if not levels:
        raise RuntimeError("shacira_amd: the octree lookup needs at least one level")
    if tables is not None:
        _need_gpu(*tables)
        if len(tables) != len(levels):
            raise RuntimeError(f"shacira_amd: {len(levels)} levels need {len(levels)} tables, got {len(tables)}")
        fdim = tables[0].shape[1] if tables[0].dim() == 2 else -1
    for l, li in enumerate(levels):
        G = 1 << li.level
        S = G + 1
        want_ci, want_occ = ((S ** 3 + 31) // 32, 2), ((G ** 3 + 31) // 32,)
        for name, t, want in (("corner index", li.corner_index, want_ci), ("occupancy", li.occupancy, want_occ)):
            if (t.dtype != torch.int32 or tuple(t.shape) != want or not t.is_contiguous() or t.device != coords.device):
                raise RuntimeError(f"shacira_amd: level {li.level} {name} must be contiguous int32 {want} on "
                                   f"{coords.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if tables is not None:
            t = tables[l]
            if (t.dtype != torch.float32 or tuple(t.shape) != (li.rows + 1, fdim) or not t.is_contiguous()
                    or t.device != coords.device):
                raise RuntimeError(f"shacira_amd: level {li.level} table must be contiguous fp32 [{li.rows + 1}, {fdim}] on "
                                   f"{coords.device}, got {t.dtype} {tuple(t.shape)}")
    return int(fdim)


def _octree_arrays(levels):
    n = len(levels)
    return (_res_array(tuple(li.level for li in levels)), (ctypes.c_int64 * n)(*[li.rows for li in levels]),
            (ctypes.c_void_p * n)(*[li.corner_index.data_ptr() for li in levels]),
            (ctypes.c_void_p * n)(*[li.occupancy.data_ptr() for li in levels]))


def octree_forward(coords, levels, tables, multiscale_sum):
    """Trilinear octree features at ``coords`` [N, 3] fp32: [N, F] (``multiscale_sum``) or [N, len(levels) * F].

    ``levels``: the ``OctreeLevelIndex`` of each level; ``tables``: its fp32 feature table [C_l + 1, F]."""
    fdim = _octree_shape(coords, levels, tables)
    N = coords.shape[0]
    K = fdim if multiscale_sum else fdim * len(levels)
    feats = torch.empty((N, K), dtype=torch.float32, device=coords.device)
    L = _lib.lib()
    la, rows, ci, occ = _octree_arrays(levels)
    with _on_device(coords.device):
        nbytes = int(L.shacira_octree_forward_workspace_bytes(N, len(levels), la, fdim, int(bool(multiscale_sum))))
        ws = _workspace(coords.device, nbytes)
        rc = L.shacira_octree_forward(N, len(levels), la, fdim, _ptr(coords), _ptr_array(tables), rows, ci, occ,
                                      int(bool(multiscale_sum)), _ptr(feats), _ptr(ws), nbytes, _stream(coords))
    _lib.check(rc, "octree_forward")
    return feats


def octree_backward(coords, levels, feature_dim, grad_output, multiscale_sum, features=None, need_features=True,
                    need_coords=False):
    """(table gradients: one fp32 [C_l + 1, F] tensor per level, or None; coordinate gradient fp32 [N, 3], or None).

    ``features`` (the forward's tables) are needed, and their values read, only when ``need_coords``. The table gradients
    are overwritten (zeroed by the call, the padding row stays zero) and come from float atomics: two runs differ in the
    last bits."""
    fdim = _octree_shape(coords, levels, features if need_coords else None, int(feature_dim))
    N = coords.shape[0]
    K = fdim if multiscale_sum else fdim * len(levels)
    grad_output = _check_grad_output(grad_output, N, K)
    flags = (_lib.OCTREE_GRAD_FEATURES if need_features else 0) | (_lib.OCTREE_GRAD_COORDS if need_coords else 0)
    if not flags:
        return None, None
    dev = coords.device
    grads = None
    if need_features:
        grads = [torch.empty((li.rows + 1, fdim), dtype=torch.float32, device=dev) for li in levels]
    grad_coords = torch.empty((N, 3), dtype=torch.float32, device=dev) if need_coords else None
    L = _lib.lib()
    la, rows, ci, occ = _octree_arrays(levels)
    with _on_device(dev):
        nbytes = int(L.shacira_octree_backward_workspace_bytes(N, len(levels), la, fdim, int(bool(multiscale_sum)), flags))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_octree_backward(N, len(levels), la, fdim, _ptr(coords),
                                       _ptr_array(features) if need_coords else None, rows, ci, occ, _ptr(grad_output),
                                       int(bool(multiscale_sum)), flags,
                                       _ptr_array(grads) if grads is not None else None, _ptr(grad_coords), _ptr(ws),
                                       nbytes, _stream(coords))
    _lib.check(rc, "octree_backward")
    return grads, grad_coords


# ---- mesh to signed distance (include/shacira_hip.h, shacira_mesh_sdf) -------------------------------------------------------
def _mesh_operands(points, triangles):
    """The checked operands of the two mesh calls as contiguous fp32 on the device of ``points``: (points, triangles, N, T,
    device)."""
    _need_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"shacira_amd: points must be [N, 3], got {tuple(points.shape)}")
    if triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3):
        raise RuntimeError(f"shacira_amd: triangles must be [T, 3, 3], got {tuple(triangles.shape)}")
    dev = points.device
    points = points.detach().to(dtype=torch.float32).contiguous()
    triangles = triangles.detach().to(device=dev, dtype=torch.float32).contiguous()
    N, T = points.shape[0], triangles.shape[0]
    return points, triangles, N, T, dev


def mesh_sdf(points, triangles):
    """Signed distance [N] fp32 of ``points`` [N, 3] to the triangles [T, 3, 3] (the vertices a, b, c of each: ``V[F]``),
    negative inside by 13-direction ray stabbing: the reference's ``_C.external.mesh_to_sdf_cuda``. Operands that are not
    contiguous fp32 are copied; ``triangles`` is moved to the device of ``points``. T == 0 gives +inf."""
    points, triangles, N, T, dev = _mesh_operands(points, triangles)
    sdf = torch.empty((N,), dtype=torch.float32, device=dev)
    if N == 0:
        return sdf
    L = _lib.lib()
    with _on_device(dev):
        nbytes = int(L.shacira_mesh_sdf_workspace_bytes(N, T))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_mesh_sdf(N, T, _ptr(points), _ptr(triangles), _ptr(sdf), _ptr(ws), nbytes, _stream(points))
    _lib.check(rc, "mesh_sdf")
    return sdf


def mesh_closest(points, triangles, signed=True):
    """(dist [N] fp32, hit [N, 3] fp32, tidx [N] int32) of ``points`` [N, 3] against the triangles [T, 3, 3]: the distance to
    the nearest non-degenerate triangle (negative inside when ``signed``: the bits of ``mesh_sdf``; otherwise its absolute
    value, and no ray stabbing is executed), the closest point and the triangle it lies on (lowest index among equals, -1 and
    ``hit = points`` when there is none). One pass over the N x T pairs (include/shacira_hip.h, shacira_mesh_closest)."""
    points, triangles, N, T, dev = _mesh_operands(points, triangles)
    dist = torch.empty((N,), dtype=torch.float32, device=dev)
    hit = torch.empty((N, 3), dtype=torch.float32, device=dev)
    tidx = torch.empty((N,), dtype=torch.int32, device=dev)
    if N == 0:
        return dist, hit, tidx
    flags = _lib.MESH_CLOSEST_SIGNED if signed else 0
    L = _lib.lib()
    with _on_device(dev):
        nbytes = int(L.shacira_mesh_closest_workspace_bytes(N, T, flags))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_mesh_closest(N, T, _ptr(points), _ptr(triangles), flags, _ptr(dist), _ptr(hit), _ptr(tidx), _ptr(ws),
                                    nbytes, _stream(points))
    _lib.check(rc, "mesh_closest")
    return dist, hit, tidx


# ---- mesh to occupancy (include/shacira_hip.h, shacira_mesh_voxelize) ---------------------------------------------------------
def mesh_voxelize(triangles, level, margin=0.5, with_grid=True):
    """The triangles [T, 3, 3] (in [-1, 1]^3) rasterised into the occupancy of octree level ``level``: (words int32
    [ceil(G^3 / 32)], grid bool [G, G, G] or None). A cell is set iff a non-degenerate triangle overlaps the closed cube of
    half-extent ``0.5 + margin`` cells around its centre; geometry outside the cube marks nothing. ``words`` has the bit layout
    of ``wisp.ops.octree``'s ``occupancy``, ``grid`` that of ``OctreeAS.occupancy_grid``. Deterministic."""
    _need_gpu(triangles)
    if triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3):
        raise RuntimeError(f"shacira_amd: triangles must be [T, 3, 3], got {tuple(triangles.shape)}")
    level, margin = int(level), float(margin)
    if not 0 <= level <= _lib.OCTREE_MAX_LEVEL:
        raise RuntimeError(f"shacira_amd: level must be in 0..{_lib.OCTREE_MAX_LEVEL}, got {level}")
    if not 0.0 <= margin < float("inf"):
        raise RuntimeError(f"shacira_amd: margin must be finite and >= 0, got {margin}")
    dev = triangles.device
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("shacira_amd: mesh_voxelize synchronises its stream (the host reads a unit count per pass of "
                           "triangles) and cannot be captured into a graph")
    triangles = triangles.detach().to(dtype=torch.float32).contiguous()
    T, G = triangles.shape[0], 1 << level
    words = torch.empty(((G ** 3 + 31) // 32,), dtype=torch.int32, device=dev)
    grid = torch.empty((G, G, G), dtype=torch.uint8, device=dev) if with_grid else None
    L = _lib.lib()
    with _on_device(dev):
        nbytes = int(L.shacira_mesh_voxelize_workspace_bytes(T, level))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_mesh_voxelize(T, _ptr(triangles), level, margin, _ptr(words), _ptr(grid), _ptr(ws), nbytes,
                                     _stream(triangles))
    _lib.check(rc, "mesh_voxelize")
    return words, (grid.view(torch.bool) if with_grid else None)


# ---- mesh point sampling (include/shacira_hip.h, shacira_mesh_sample / shacira_mesh_sample_count) --------------------------------
MESH_SAMPLE_MODES = {"surface": _lib.MESH_SAMPLE_SURFACE, "near": _lib.MESH_SAMPLE_NEAR, "cube": _lib.MESH_SAMPLE_CUBE,
                     "cells": _lib.MESH_SAMPLE_CELLS}
MeshSamples = collections.namedtuple("MeshSamples", ["points", "normals", "face_idx", "source_idx", "block_counts"])


def mesh_face_cdf(triangles):
    """The integer area CDF the sampler searches: an int32 tensor [T] holding uint32 bits, on the device of ``triangles``
    [T, 3, 3]. cdf[t] = min(floor(sum[t] / sum[T - 1] * 2^32), 2^32 - 1), where sum is the running sum, in
    index order and in fp64, of |cross(a - b, b - c)| (the operator order of ``per_face_normals``: the differences in fp32,
    the cross product, its norm and the sum in fp64). Built once per mesh, on the host: the datasets cache it. A mesh without
    area (or with a non-finite one) is refused with SHACIRA_EINVAL."""
    if triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3):
        raise RuntimeError(f"shacira_amd: triangles must be [T, 3, 3], got {tuple(triangles.shape)}")
    tri = triangles.detach().to(dtype=torch.float32).cpu().numpy()
    x, y = (tri[:, 0] - tri[:, 1]).astype(np.float64), (tri[:, 1] - tri[:, 2]).astype(np.float64)
    nx = x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1]
    ny = x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2]
    nz = x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]
    run = np.cumsum(np.sqrt((nx * nx + ny * ny) + nz * nz))
    if run.shape[0] == 0 or not (run[-1] > 0) or not np.isfinite(run[-1]):
        _lib.check(_lib.EINVAL, "mesh_face_cdf (the mesh has no area)")
    cdf = np.minimum(np.floor(run / run[-1] * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)
    return torch.from_numpy(cdf.view(np.int32)).to(triangles.device)


def _u32_operand(t, shape, dev, what, who="mesh_sample"):
    """``t`` as contiguous 32-bit integer words of ``shape`` on ``dev`` (int32 and uint32 tensors carry the same bits)."""
    if t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or t.device != dev or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"shacira_amd: {who} expects {what} as int32 / uint32 {list(shape)} on {dev}, got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device}")
    return t.contiguous()


def mesh_sample(mode, n=None, seed=0, segment=0, index_base=0, triangles=None, cdf=None, sigma=0.0, corners=None,
                samples_per_cell=None, cell_level=None, occupancy=None, occupancy_level=None, words=None, want_normals=False,
                want_face=False, want_source=False, device=None):
    """``MeshSamples`` of one sampling technique, every sample a pure function of (``seed``, ``index_base`` + i, ``segment``):

    mode 'surface'  points uniform on ``triangles`` [T, 3, 3] (faces by area through ``cdf``, ``mesh_face_cdf(triangles)`` when
                    None), their unnormalised face normals and face indices
         'near'     surface points displaced by ``sigma`` times a standard normal per coordinate
         'cube'     uniform in [-1, 1)^3
         'cells'    ``samples_per_cell`` uniform points in every cell of ``corners`` (int16 [C, 3], cells of ``cell_level``);
                    ``n`` is C * samples_per_cell

    ``occupancy`` (the packed int32 words of ``occupancy_level``, ``OctreeAS.packed_occupancy``) keeps only the samples whose
    cell is occupied -- ``OctreeAS.query(...).pidx > -1`` -- in index order: a counting launch, an exact int64 ``cumsum``, one
    read-back of the total, a writing launch (not capturable into a graph; the unfiltered form is one launch and is).
    ``block_counts`` is then the int32 count per 256 indices, else None. ``words`` (int32 / uint32 [n, 8]) replaces the random
    words. ``normals`` / ``face_idx`` (int32) / ``source_idx`` (int64, the index i of every row) are None unless wanted. The
    operands must be on the GPU; without tensor operands ('cube') ``device`` says where."""
    if mode not in MESH_SAMPLE_MODES:
        raise ValueError(f"mesh_sample: unknown mode {mode!r} (expected one of {sorted(MESH_SAMPLE_MODES)})")
    code = MESH_SAMPLE_MODES[mode]
    _need_gpu(triangles, cdf, corners, occupancy, words)
    seed, segment, index_base = int(seed), int(segment), int(index_base)
    if not 0 <= seed < 1 << 64 or not 0 <= segment < 1 << 32 or index_base < 0:
        raise RuntimeError(f"shacira_amd: mesh_sample expects 0 <= seed < 2^64, 0 <= segment < 2^32 and index_base >= 0, got "
                           f"{seed}, {segment}, {index_base}")
    dev = next((t.device for t in (triangles, corners, occupancy, words) if t is not None), None)
    if dev is None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            _need_gpu(torch.empty(0, device=dev))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
    T = C = spc = level = 0
    if code in (_lib.MESH_SAMPLE_SURFACE, _lib.MESH_SAMPLE_NEAR):
        if triangles is None or triangles.dim() != 3 or tuple(triangles.shape[1:]) != (3, 3) or triangles.shape[0] < 1:
            raise RuntimeError(f"shacira_amd: mesh_sample('{mode}') expects triangles [T >= 1, 3, 3], got "
                               f"{None if triangles is None else tuple(triangles.shape)}")
        triangles = triangles.detach().to(device=dev, dtype=torch.float32).contiguous()
        T = triangles.shape[0]
        cdf = mesh_face_cdf(triangles) if cdf is None else _u32_operand(cdf, (T,), dev, "cdf")
    else:
        triangles = cdf = None
    if code == _lib.MESH_SAMPLE_CELLS:
        if corners is None or corners.dim() != 2 or corners.shape[1] < 3 or samples_per_cell is None or cell_level is None:
            raise RuntimeError("shacira_amd: mesh_sample('cells') expects corners [C, 3], samples_per_cell and cell_level")
        corners = corners[:, :3].to(device=dev, dtype=torch.int16).contiguous()
        C, spc, level = corners.shape[0], int(samples_per_cell), int(cell_level)
        if spc < 1 or not 0 <= level <= _lib.OCTREE_MAX_LEVEL:
            raise RuntimeError(f"shacira_amd: mesh_sample('cells') expects samples_per_cell >= 1 and cell_level in "
                               f"0..{_lib.OCTREE_MAX_LEVEL}, got {spc}, {level}")
        if n is None:
            n = C * spc
    else:
        corners = None
    if n is None or int(n) < 0:
        raise RuntimeError(f"shacira_amd: mesh_sample expects n >= 0, got {n}")
    n = int(n)
    if words is not None:
        words = _u32_operand(words, (n, 8), dev, "words")
    olevel = 0
    if occupancy is not None:
        olevel = int(occupancy_level)
        if not 0 <= olevel <= _lib.OCTREE_MAX_LEVEL:
            raise RuntimeError(f"shacira_amd: occupancy_level must be in 0..{_lib.OCTREE_MAX_LEVEL}, got {olevel}")
        occupancy = _u32_operand(occupancy, (((1 << (3 * olevel)) + 31) // 32,), dev, "occupancy")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("shacira_amd: the filtered mesh_sample reads the number of kept samples back between its two "
                               "launches and cannot be captured into a graph")
    L = _lib.lib()
    head = (code, n, index_base, seed, segment, _ptr(words), T, _ptr(triangles), _ptr(cdf), float(sigma), C, _ptr(corners), spc,
            level, _ptr(occupancy), olevel)
    blocks = (n + _lib.MESH_SAMPLE_BLOCK - 1) // _lib.MESH_SAMPLE_BLOCK
    counts = offsets = None
    rows = n
    with _on_device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if occupancy is not None:
            counts = torch.empty((blocks,), dtype=torch.int32, device=dev)
            _lib.check(L.shacira_mesh_sample_count(*head, _ptr(counts), stream), "mesh_sample_count")
            ends = torch.cumsum(counts, dim=0, dtype=torch.int64)          # integers: exact
            rows = int(ends[-1].item()) if blocks else 0
            offsets = ends - counts
        points = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((rows, 3), dtype=torch.float32, device=dev) if want_normals else None
        face = torch.empty((rows,), dtype=torch.int32, device=dev) if want_face else None
        source = torch.empty((rows,), dtype=torch.int64, device=dev) if want_source else None
        if rows > 0:                                                       # nothing kept: the writer is not launched
            _lib.check(L.shacira_mesh_sample(*head, _ptr(offsets), _ptr(points), _ptr(normals), _ptr(face), _ptr(source),
                                             stream), "mesh_sample")
    return MeshSamples(points, normals, face, source, counts)


# ---- structural similarity (include/shacira_hip.h, shacira_ssim_forward / shacira_ssim_backward) -------------------------------
def _ssim_operands(pred, target, channels):
    """The checked operands of the two SSIM calls: (pred, target, H, W, Cin, C) with both images contiguous fp32 [H, W, Cin] on
    the device of ``pred``. Sizes below the 11-pixel window raise ValueError, as skimage does."""
    _need_gpu(pred, target)
    if pred.dim() != 3 or pred.shape != target.shape:
        raise RuntimeError(f"shacira_amd: ssim expects two [H, W, C] images of one shape, got {tuple(pred.shape)} and "
                           f"{tuple(target.shape)}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise RuntimeError("shacira_amd: ssim expects fp32 images")
    H, W, Cin = pred.shape
    C = Cin if channels is None else int(channels)
    if H < _lib.SSIM_WINDOW or W < _lib.SSIM_WINDOW:
        raise ValueError(f"win_size exceeds image extent: the {_lib.SSIM_WINDOW}-pixel window does not fit a {H} x {W} image")
    if not 1 <= C <= Cin:
        raise RuntimeError(f"shacira_amd: ssim over {C} channels of a {Cin}-channel image")
    return pred.detach().contiguous(), target.detach().to(pred.device).contiguous(), H, W, Cin, C


def ssim_forward(pred, target, channels=None, data_range=1.0, with_map=False):
    """(value, map): the SSIM of ``pred`` against ``target`` ([H, W, Cin] fp32 on the device) over their first ``channels``
    channels (all by default) as ONE fp64 on the device, and the per-pixel map fp32 [H, W, channels] (``None`` unless
    ``with_map``). No host read-back: capturable. Deterministic to the bit."""
    pred, target, H, W, Cin, C = _ssim_operands(pred, target, channels)
    dev = pred.device
    value = torch.empty((), dtype=torch.float64, device=dev)
    smap = torch.empty((H, W, C), dtype=torch.float32, device=dev) if with_map else None
    L = _lib.lib()
    with _on_device(dev):
        nbytes = int(L.shacira_ssim_workspace_bytes(H, W, C, 0))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_ssim_forward(H, W, Cin, C, _ptr(pred), _ptr(target), float(data_range), _ptr(value), _ptr(smap),
                                    _ptr(ws), nbytes, _stream(pred))
    _lib.check(rc, "ssim_forward")
    return value, smap


def ssim_backward(pred, target, grad, channels=None, data_range=1.0):
    """d(grad * SSIM)/d(pred): fp32 [H, W, Cin], exactly zero in the channels beyond ``channels``. ``grad`` is a one-element
    tensor on the device (any float dtype) or a number. There is no gradient with respect to ``target``."""
    pred, target, H, W, Cin, C = _ssim_operands(pred, target, channels)
    dev = pred.device
    if torch.is_tensor(grad):
        _need_gpu(grad)
        if grad.numel() != 1:
            raise RuntimeError(f"shacira_amd: ssim_backward expects a scalar grad, got {tuple(grad.shape)}")
        grad = grad.detach().to(dtype=torch.float32).reshape(1).contiguous()
    else:
        grad = torch.full((1,), float(grad), dtype=torch.float32, device=dev)
    grad_pred = torch.empty((H, W, Cin), dtype=torch.float32, device=dev)
    L = _lib.lib()
    with _on_device(dev):
        nbytes = int(L.shacira_ssim_workspace_bytes(H, W, C, 1))
        ws = _workspace(dev, nbytes)
        rc = L.shacira_ssim_backward(H, W, Cin, C, _ptr(pred), _ptr(target), float(data_range), _ptr(grad), _ptr(grad_pred),
                                     _ptr(ws), nbytes, _stream(pred))
    _lib.check(rc, "ssim_backward")
    return grad_pred


# ---- positional-encoding rows (include/shacira_hip.h, shacira_posenc_forward / _backward / _backward2) -------------------------
def _posenc_rows(t, width, what):
    """``t`` as an fp32 [N, width] device operand of the row kernels and its row stride in floats: a tensor whose last stride is
    not 1 (or whose rows overlap) is made contiguous, a row-strided view such as ``x[:, :3]`` is passed as it is."""
    _need_gpu(t)
    if t.dtype != torch.float32:
        raise RuntimeError(f"shacira_amd: posenc expects fp32 {what}, got {t.dtype}")
    if t.dim() != 2 or (width is not None and t.shape[1] != width):
        raise RuntimeError(f"shacira_amd: posenc expects {what} [N, {width if width is not None else 'd'}], got "
                           f"{tuple(t.shape)}")
    t = t.detach()
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))


def _posenc_shape(d, bands, include_input, prefix_width):
    F = bands.numel()
    if not 1 <= d <= _lib.POSENC_MAX_DIM or not 1 <= F <= _lib.POSENC_MAX_BANDS or bands.dim() != 1:
        raise RuntimeError(f"shacira_amd: posenc takes 1..{_lib.POSENC_MAX_DIM} coordinates and 1..{_lib.POSENC_MAX_BANDS} "
                           f"bands, got d = {d}, bands {tuple(bands.shape)}")
    if bands.dtype != torch.float32 or not bands.is_cuda:
        raise RuntimeError("shacira_amd: posenc expects fp32 bands on the device")
    return F, int(prefix_width) + (d if include_input else 0) + 2 * d * F


def posenc_forward(coords, bands, prefix=None, include_input=True, out=None):
    """The row ``[prefix | coords | sin(coords * bands) | cos(coords * bands)]`` fp32 [N, P + E] in one kernel (the layout of the
    reference's PositionalEmbedder behind the ``P`` prefix columns). ``out``: an fp32 [N, P + E] tensor or row-strided view to
    write into (columns of its storage beyond P + E are left alone); a new tensor otherwise."""
    coords, cs = _posenc_rows(coords, None, "coords")
    N, d = coords.shape
    P = 0 if prefix is None else int(prefix.shape[-1])
    bands = bands.detach().contiguous()
    F, width = _posenc_shape(d, bands, include_input, P)
    dev = coords.device
    ps = 0
    if prefix is not None:
        prefix, ps = _posenc_rows(prefix, P, "prefix")
        if prefix.shape[0] != N or prefix.device != dev:
            raise RuntimeError(f"shacira_amd: posenc prefix {tuple(prefix.shape)} on {prefix.device} for coords {(N, d)} on {dev}")
    if bands.device != dev:
        raise RuntimeError("shacira_amd: posenc bands and coords are on different devices")
    if out is None:
        out = torch.empty((N, width), dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (N, width)
          or (width > 1 and out.stride(1) != 1) or (N > 1 and out.stride(0) < width)):
        raise RuntimeError(f"shacira_amd: posenc out must be fp32 [{N}, {width}] on {dev} with unit column stride")
    if N == 0:
        return out
    os_ = out.stride(0) if N > 1 else width
    with _on_device(dev):
        rc = _lib.lib().shacira_posenc_forward(N, d, F, int(bool(include_input)), P, _ptr(coords), cs,
                                               _ptr(prefix) if P > 0 else None, ps, _ptr(bands), _ptr(out), os_,
                                               _stream(coords))
    _lib.check(rc, "posenc_forward")
    return out


def posenc_backward(row, grad_out, bands, d, include_input=True, prefix_width=0):
    """grad_coords fp32 [N, d] of ``posenc_forward`` from its SAVED output ``row`` and ``grad_out`` (both [N, P + E])."""
    bands = bands.detach().contiguous()
    F, width = _posenc_shape(int(d), bands, include_input, prefix_width)
    row, rs = _posenc_rows(row, width, "row")
    grad_out, gs = _posenc_rows(grad_out, width, "grad_out")
    N, dev = row.shape[0], row.device
    if grad_out.shape[0] != N or grad_out.device != dev or bands.device != dev:
        raise RuntimeError("shacira_amd: posenc_backward operands disagree in rows or device")
    grad_coords = torch.empty((N, int(d)), dtype=torch.float32, device=dev)
    if N == 0:
        return grad_coords
    with _on_device(dev):
        rc = _lib.lib().shacira_posenc_backward(N, int(d), F, int(bool(include_input)), int(prefix_width), _ptr(row), rs,
                                                _ptr(grad_out), gs, _ptr(bands), _ptr(grad_coords), _stream(row))
    _lib.check(rc, "posenc_backward")
    return grad_coords


def posenc_backward2(gg, row, grad_out, bands, d, include_input=True, prefix_width=0):
    """(grad_row, grad_grad_out), both fp32 [N, P + E]: the gradients of ``(posenc_backward(row, grad_out) * gg).sum()`` with
    respect to ``row`` and to ``grad_out``."""
    bands = bands.detach().contiguous()
    F, width = _posenc_shape(int(d), bands, include_input, prefix_width)
    row, rs = _posenc_rows(row, width, "row")
    grad_out, gs = _posenc_rows(grad_out, width, "grad_out")
    gg, _ = _posenc_rows(gg, int(d), "gg")
    gg = gg.contiguous()
    N, dev = row.shape[0], row.device
    if grad_out.shape[0] != N or gg.shape[0] != N or grad_out.device != dev or gg.device != dev or bands.device != dev:
        raise RuntimeError("shacira_amd: posenc_backward2 operands disagree in rows or device")
    grad_row = torch.empty((N, width), dtype=torch.float32, device=dev)
    grad_grad = torch.empty((N, width), dtype=torch.float32, device=dev)
    if N == 0:
        return grad_row, grad_grad
    with _on_device(dev):
        rc = _lib.lib().shacira_posenc_backward2(N, int(d), F, int(bool(include_input)), int(prefix_width), _ptr(gg), _ptr(row),
                                                 rs, _ptr(grad_out), gs, _ptr(bands), _ptr(grad_row), _ptr(grad_grad),
                                                 _stream(row))
    _lib.check(rc, "posenc_backward2")
    return grad_row, grad_grad


# ---- ray generation (include/shacira_hip.h, shacira_raygen) ---------------------------------------------------------------------
def image_mip(images, mip, out=None):
    """The mip level ``mip`` (1 .. 4) of uint8 images [V, H, W, C] or of one image [H, W, C] (C 1 .. 4) on the device, as exact
    block sums in one kernel: uint16 [V, H >> mip, W >> mip, C] (or [H >> mip, W >> mip, C]), each the sum of a 2^mip x 2^mip
    block of bytes; the block mean -- OpenCV's INTER_AREA -- is ``sum / 4^mip``. H and W must be multiples of 2^mip. ``out``: a
    contiguous uint16 tensor of that shape to write into (a slice of a larger set, say)."""
    _need_gpu(images)
    if images.dtype != torch.uint8 or images.dim() not in (3, 4):
        raise RuntimeError(f"shacira_amd: image_mip expects uint8 images [V, H, W, C] or [H, W, C], got {images.dtype} "
                           f"{tuple(images.shape)}")
    single = images.dim() == 3
    if single:
        images = images.unsqueeze(0)
    images = images.contiguous()
    V, H, W, C = (int(s) for s in images.shape)
    mip = int(mip)
    if not 1 <= mip <= _lib.IMAGE_MIP_MAX:
        raise RuntimeError(f"shacira_amd: image_mip takes mip 1..{_lib.IMAGE_MIP_MAX}, got {mip}")
    if H % (1 << mip) or W % (1 << mip):
        raise RuntimeError(f"shacira_amd: image_mip needs H and W divisible by {1 << mip} at mip {mip}, got {H} x {W}")
    shape = (V, H >> mip, W >> mip, C)
    if out is None:
        sums = torch.empty(shape, dtype=torch.uint16, device=images.device)
    else:
        sums = out.unsqueeze(0) if single and out.dim() == 3 else out
        if sums.dtype != torch.uint16 or tuple(sums.shape) != shape or sums.device != images.device or not sums.is_contiguous():
            raise RuntimeError(f"shacira_amd: image_mip out must be contiguous uint16 {list(shape)} on {images.device}")
    if sums.numel() > 0:
        with _on_device(images.device):
            rc = _lib.lib().shacira_image_mip(_ptr(images), V, H, W, C, mip, _ptr(sums), _stream(images))
        _lib.check(rc, "image_mip")
    return sums[0] if single else sums


def raygen(records, width, height, view_idx=None, pixel_idx=None, jitter=None, images=None, bg_color="white", num_rays=None,
           mip=0):
    """(origins, dirs, rgb, mask) of (view, pixel) pairs in one kernel: fp32 [n, 3] each and bool [n, 1]; ``rgb`` and ``mask``
    are None without ``images``. ``records``: fp32 [V, RAYGEN_RECORD_FLOATS] camera records; ``view_idx`` / ``pixel_idx``: int32
    [n] (pixel = y * W + x), or both None for the whole-view form -- ray i is pixel i mod (H W) of view i div (H W), for the first
    ``num_rays`` rays (default: all V H W); ``jitter``: fp32 [n, 2] or None; ``images``: uint8 [V, H, W, 3 or 4] or None.
    With ``mip`` > 0 ``images`` are the uint16 block sums of that mip level (``image_mip``), ``width`` and ``height`` the
    level's, and a colour is sum / (255 * 4^mip). An index out of range gives a NaN row and mask 0. Not differentiable."""
    _need_gpu(records, view_idx, pixel_idx, jitter, images)
    dev = records.device
    mip = int(mip or 0)
    if not 0 <= mip <= _lib.IMAGE_MIP_MAX:
        raise RuntimeError(f"shacira_amd: raygen takes mip 0..{_lib.IMAGE_MIP_MAX}, got {mip}")
    pixel_dtype = torch.uint16 if mip > 0 else torch.uint8
    K = _lib.RAYGEN_RECORD_FLOATS
    if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != K or not records.is_contiguous():
        raise RuntimeError(f"shacira_amd: raygen expects contiguous fp32 records [V, {K}], got {records.dtype} "
                           f"{tuple(records.shape)}")
    V, W, H = records.shape[0], int(width), int(height)
    if bg_color not in ("white", "black"):
        raise RuntimeError(f"shacira_amd: raygen bg_color must be 'white' or 'black', got {bg_color!r}")
    if (view_idx is None) != (pixel_idx is None):
        raise RuntimeError("shacira_amd: raygen takes view_idx and pixel_idx together, or neither")
    if view_idx is None:
        n = V * H * W if num_rays is None else int(num_rays)
    else:
        for name, t in (("view_idx", view_idx), ("pixel_idx", pixel_idx)):
            if t.dtype != torch.int32 or t.dim() != 1 or t.device != dev:
                raise RuntimeError(f"shacira_amd: raygen expects int32 [n] {name} on {dev}, got {t.dtype} {tuple(t.shape)} "
                                   f"on {t.device}")
        n = view_idx.shape[0]
        if pixel_idx.shape[0] != n or (num_rays is not None and int(num_rays) != n):
            raise RuntimeError("shacira_amd: raygen view_idx, pixel_idx and num_rays disagree")
        view_idx, pixel_idx = view_idx.contiguous(), pixel_idx.contiguous()
    if jitter is not None:
        if jitter.dtype != torch.float32 or tuple(jitter.shape) != (n, 2) or jitter.device != dev:
            raise RuntimeError(f"shacira_amd: raygen expects fp32 jitter [{n}, 2] on {dev}")
        jitter = jitter.detach().contiguous()
    channels = 4
    if images is not None:
        if images.dtype != pixel_dtype or images.dim() != 4 or tuple(images.shape[:3]) != (V, H, W) or images.device != dev:
            what = f"uint16 sums (mip {mip})" if mip > 0 else "uint8 images"
            raise RuntimeError(f"shacira_amd: raygen expects {what} [{V}, {H}, {W}, C] on {dev}, got {images.dtype} "
                               f"{tuple(images.shape)} on {images.device}")
        images = images.contiguous()
        channels = images.shape[3]
    origins = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rgb = mask = None
    if images is not None:
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        mask = torch.empty((n, 1), dtype=torch.bool, device=dev)
    bg = _lib.RAYGEN_BG_BLACK if bg_color == "black" else _lib.RAYGEN_BG_WHITE
    with _on_device(dev):
        if mip > 0:
            rc = _lib.lib().shacira_raygen_sums(_ptr(records), V, W, H, _ptr(view_idx), _ptr(pixel_idx), _ptr(jitter), n,
                                                _ptr(images), channels, mip, bg, _ptr(origins), _ptr(dirs), _ptr(rgb),
                                                _ptr(mask), _stream(records))
        else:
            rc = _lib.lib().shacira_raygen(_ptr(records), V, W, H, _ptr(view_idx), _ptr(pixel_idx), _ptr(jitter), n,
                                           _ptr(images), channels, bg, _ptr(origins), _ptr(dirs), _ptr(rgb), _ptr(mask),
                                           _stream(records))
    _lib.check(rc, "raygen")
    return origins, dirs, rgb, mask


# ---- structured point clouds (include/shacira_hip.h, shacira_depth_* / shacira_spc_*) ------------------------------------------
def _depth_operands(records, depth, images=None, bg_color="white", mip=0):
    """The checked operands the depth entries share: (records, depth, images, head) with ``head`` the leading C arguments
    (cams, V, W, H, depth). ``depth``: fp32 [V, H, W]; ``images``: uint8 [V, H, W, 3 or 4], or the uint16 sums of ``mip``."""
    _need_gpu(records, depth, images)
    dev = records.device
    K = _lib.RAYGEN_RECORD_FLOATS
    if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != K or not records.is_contiguous():
        raise RuntimeError(f"shacira_amd: expected contiguous fp32 records [V, {K}], got {records.dtype} {tuple(records.shape)}")
    V = records.shape[0]
    if depth.dtype != torch.float32 or depth.dim() != 3 or depth.shape[0] != V or depth.device != dev:
        raise RuntimeError(f"shacira_amd: expected fp32 depth [{V}, H, W] on {dev}, got {depth.dtype} {tuple(depth.shape)} on "
                           f"{depth.device}")
    depth = depth.detach().contiguous()
    H, W = int(depth.shape[1]), int(depth.shape[2])
    mip = int(mip or 0)
    if images is not None:
        if not 0 <= mip <= _lib.IMAGE_MIP_MAX:
            raise RuntimeError(f"shacira_amd: mip must be in 0..{_lib.IMAGE_MIP_MAX}, got {mip}")
        want = torch.uint16 if mip > 0 else torch.uint8
        if (images.dtype != want or images.dim() != 4 or tuple(images.shape[:3]) != (V, H, W) or images.shape[3] not in (3, 4)
                or images.device != dev):
            raise RuntimeError(f"shacira_amd: expected {want} images [{V}, {H}, {W}, 3 or 4] on {dev}, got {images.dtype} "
                               f"{tuple(images.shape)} on {images.device}")
        images = images.contiguous()
        if bg_color not in ("white", "black"):
            raise RuntimeError(f"shacira_amd: bg_color must be 'white' or 'black', got {bg_color!r}")
    return records, depth, images, (_ptr(records), V, W, H, _ptr(depth))


def _image_tail(images, bg_color, mip):
    return (_ptr(images), int(images.shape[3]), int(mip or 0),
            _lib.RAYGEN_BG_BLACK if bg_color == "black" else _lib.RAYGEN_BG_WHITE)


def depth_bounds(records, depth):
    """(bounds, count) on the device, no read-back: fp32 [6] = the per-axis minimum then maximum of the points of all pixels of
    ``depth`` (fp32 [V, H, W]) that are finite, and int64 [1], their number. +inf / -inf / 0 without one. Deterministic."""
    records, depth, _, head = _depth_operands(records, depth)
    dev = records.device
    bounds = torch.empty((6,), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    if depth.numel() == 0:
        bounds[:3], bounds[3:] = float("inf"), float("-inf")
        count.zero_()
        return bounds, count
    with _on_device(dev):
        _lib.check(_lib.lib().shacira_depth_bounds(*head, _ptr(bounds), _ptr(count), _stream(records)), "depth_bounds")
    return bounds, count


def depth_points(records, depth, images=None, bg_color="white", mip=0):
    """(points fp32 [M, 3], colors uint8 [M, 3] or None): the points of the finite pixels of ``depth`` in (view, pixel) order and,
    with ``images``, their composited colours as bytes. A counting launch, an exact int64 ``cumsum``, one read-back of M, a
    writing launch (not capturable). Two calls return the same bits."""
    records, depth, images, head = _depth_operands(records, depth, images, bg_color, mip)
    dev = records.device
    n = depth.numel()
    blocks = (n + _lib.DEPTH_POINTS_BLOCK - 1) // _lib.DEPTH_POINTS_BLOCK
    L = _lib.lib()
    rows = 0
    with _on_device(dev):
        stream = _stream(records)
        if blocks:
            counts = torch.empty((blocks,), dtype=torch.int32, device=dev)
            _lib.check(L.shacira_depth_points_count(*head, _ptr(counts), stream), "depth_points_count")
            ends = torch.cumsum(counts, dim=0, dtype=torch.int64)          # integers: exact
            rows = int(ends[-1].item())
            offsets = ends - counts
        points = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((rows, 3), dtype=torch.uint8, device=dev) if images is not None else None
        if rows > 0:
            tail = _image_tail(images, bg_color, mip) if images is not None else (None, 3, 0, 0)
            _lib.check(L.shacira_depth_points_emit(*head, *tail, _ptr(offsets), _ptr(points), _ptr(colors), stream),
                       "depth_points_emit")
    return points, colors


def _spc_level(level):
    level = int(level)
    if not 1 <= level <= _lib.OCTREE_MAX_LEVEL:
        raise RuntimeError(f"shacira_amd: an SPC level must be in 1..{_lib.OCTREE_MAX_LEVEL}, got {level}")
    return level


def spc_num_words(level):
    return max(1, (1 << (3 * int(level))) // 32)


def _spc_rank(words, level, stream):
    """(rank int32, num_cells): the exclusive prefix of the words' popcounts and its total (one read-back: the colours' size)."""
    pop = torch.empty_like(words)
    _lib.check(_lib.lib().shacira_spc_rank(level, _ptr(words), _ptr(pop), stream), "spc_rank")
    ends = torch.cumsum(pop, dim=0, dtype=torch.int32)                      # at most 2^30 cells: exact in int32
    return ends - pop, int(ends[-1].item())


def _spc_build(dev, level, mark, accumulate):
    words = torch.zeros((spc_num_words(level),), dtype=torch.int32, device=dev)
    with _on_device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        mark(words, stream)
        rank, cells = _spc_rank(words, level, stream)
        colors = None
        if accumulate is not None:
            colors = torch.empty((cells, 4), dtype=torch.uint8, device=dev)
            if cells > 0:
                sums = torch.zeros((cells, 4), dtype=torch.int64, device=dev)       # the kernel's uint64: the same bits
                accumulate(words, rank, cells, sums, stream)
                _lib.check(_lib.lib().shacira_spc_resolve(cells, _ptr(sums), _ptr(colors), stream), "spc_resolve")
    return words, rank, colors, cells


def spc_from_points(points, colors_u8, level):
    """(words, rank, colors, num_cells) of the SPC of ``level`` holding ``points`` (fp32 [N, 3]; points that are not finite are
    dropped, the others clamped into [-1, 1]^3's cells) with the rounded mean of ``colors_u8`` (uint8 [N, 3], or None: no
    colours) per cell: mark, popcount + scan, accumulate, resolve -- no sort. Deterministic to the bit."""
    _need_gpu(points, colors_u8)
    level = _spc_level(level)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"shacira_amd: spc_from_points expects fp32 points [N, 3], got {points.dtype} {tuple(points.shape)}")
    points = points.detach().contiguous()
    N, dev = points.shape[0], points.device
    if colors_u8 is not None:
        if colors_u8.dtype != torch.uint8 or tuple(colors_u8.shape) != (N, 3) or colors_u8.device != dev:
            raise RuntimeError(f"shacira_amd: spc_from_points expects uint8 colours [{N}, 3] on {dev}")
        colors_u8 = colors_u8.contiguous()
    L = _lib.lib()

    def mark(words, stream):
        _lib.check(L.shacira_spc_mark_points(N, _ptr(points), level, _ptr(words), stream), "spc_mark_points")

    def accumulate(words, rank, cells, sums, stream):
        _lib.check(L.shacira_spc_accumulate_points(N, _ptr(points), _ptr(colors_u8), level, _ptr(words), _ptr(rank), cells,
                                                   _ptr(sums), stream), "spc_accumulate_points")
    return _spc_build(dev, level, mark, accumulate if colors_u8 is not None else None)


def spc_from_depth(records, depth, images, level, bg_color="white", mip=0):
    """``spc_from_points`` of the cloud ``depth_points`` would make, without making it: the marking and the accumulating kernel
    derive each point and colour from (view, pixel). The same bits as the two-step path."""
    level = _spc_level(level)
    records, depth, images, head = _depth_operands(records, depth, images, bg_color, mip)
    L = _lib.lib()

    def mark(words, stream):
        _lib.check(L.shacira_spc_mark_depth(*head, level, _ptr(words), stream), "spc_mark_depth")

    def accumulate(words, rank, cells, sums, stream):
        _lib.check(L.shacira_spc_accumulate_depth(*head, *_image_tail(images, bg_color, mip), level, _ptr(words), _ptr(rank),
                                                  cells, _ptr(sums), stream), "spc_accumulate_depth")
    return _spc_build(records.device, level, mark, accumulate if images is not None else None)


def spc_first_hit(origins, dirs, level, words, rank=None, colors=None):
    """(depth fp32 [N], hit bool [N], pidx int32 [N], rgb fp32 [N, 3] or None) of the first occupied cell of ``level`` along every
    ray, in ONE launch: the first nugget of ``render.raytrace_dense`` on the same set (same ``pidx``, entry depth bit for bit).
    A miss -- and any ray with a component that is not finite -- gives 0 / False / -1 / 0. ``words``: the packed occupancy;
    ``rank`` and ``colors`` (uint8 [cells, 4]) give ``rgb`` = byte / 255, None without them."""
    _need_gpu(origins, dirs, words, rank, colors)
    level = _spc_level(level)
    dev = origins.device
    origins = _rows(origins.detach().contiguous(), "origins", dev=dev)
    dirs = _rows(dirs.detach().contiguous(), "dirs", dev=dev, n=origins.shape[0])
    N = origins.shape[0]
    want_rgb = colors is not None
    words = _u32_operand(words, (spc_num_words(level),), dev, "words", "spc_first_hit")
    if (rank is None) != (colors is None):
        raise RuntimeError("shacira_amd: spc_first_hit takes rank and colors together, or neither")
    if colors is not None:
        rank = _u32_operand(rank, (spc_num_words(level),), dev, "rank", "spc_first_hit")
        if colors.dtype != torch.uint8 or colors.dim() != 2 or colors.shape[1] != 4 or colors.device != dev:
            raise RuntimeError(f"shacira_amd: spc_first_hit expects uint8 colors [cells, 4] on {dev}")
        colors = colors.contiguous()
        if colors.shape[0] == 0:            # an empty SPC: nothing can be hit, nothing is looked up
            rank = colors = None
    depth = torch.empty((N,), dtype=torch.float32, device=dev)
    hit = torch.empty((N,), dtype=torch.bool, device=dev)
    pidx = torch.empty((N,), dtype=torch.int32, device=dev)
    rgb = torch.zeros((N, 3), dtype=torch.float32, device=dev) if want_rgb else None
    if N > 0:
        with _on_device(dev):
            rc = _lib.lib().shacira_spc_first_hit(N, _ptr(origins), _ptr(dirs), level, _ptr(words), _ptr(rank), _ptr(colors),
                                                  _ptr(depth), _ptr(hit), _ptr(pidx), _ptr(rgb), _stream(origins))
        _lib.check(rc, "spc_first_hit")
    return depth, hit, pidx, rgb


# ---- pixel batches and the pixel loss (include/shacira_hip.h, shacira_pixel_batch / shacira_pixel_loss_*) -----------------------
def _pixel_operands(image, pixel_idx, start, n, what):
    """The checked operands the pixel calls share: (image, H, W, pixel_idx, idx_bits, start, n)."""
    _need_gpu(image, pixel_idx)
    dev = image.device
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or not image.is_contiguous():
        raise RuntimeError(f"shacira_amd: {what} expects a contiguous uint8 image [H, W, 3], got {image.dtype} "
                           f"{tuple(image.shape)}")
    H, W = int(image.shape[0]), int(image.shape[1])
    if H < 1 or W < 1:
        raise RuntimeError(f"shacira_amd: {what} expects an image of at least one pixel, got {H} x {W}")
    if pixel_idx is None:
        start = int(start)
        n = H * W - start if n is None else int(n)
        if start < 0 or n < 0 or start + n > H * W:
            raise RuntimeError(f"shacira_amd: {what}: pixels {start} .. {start + n} are not inside a {H} x {W} image")
        return image, H, W, None, 64, start, n
    if pixel_idx.dtype not in (torch.int32, torch.int64) or pixel_idx.device != dev:
        raise RuntimeError(f"shacira_amd: {what} expects int32 or int64 pixel_idx on {dev}, got {pixel_idx.dtype} on "
                           f"{pixel_idx.device}")
    if pixel_idx.dim() == 2 and pixel_idx.shape[1] == 1:       # the [n, 1] indices the 'eval' and 'wreplace' batches carry
        pixel_idx = pixel_idx.reshape(-1)
    if pixel_idx.dim() != 1 or (n is not None and int(n) != pixel_idx.shape[0]):
        raise RuntimeError(f"shacira_amd: {what} expects pixel_idx [n] or [n, 1], got {tuple(pixel_idx.shape)}"
                           + (f" for n = {n}" if n is not None else ""))
    pixel_idx = pixel_idx.contiguous()
    return image, H, W, pixel_idx, 32 if pixel_idx.dtype == torch.int32 else 64, 0, pixel_idx.shape[0]


def pixel_batch(image, pixel_idx=None, start=0, n=None, want_coords=True, want_rgb=True):
    """(coords, rgb) of pixels of ``image`` (uint8 [H, W, 3] on the device) in one kernel: fp32 [n, 2] in [-1, 1) with the ROW
    first and fp32 [n, 3] = byte / 255; the one not wanted is None. ``pixel_idx``: int32 or int64 [n] (or [n, 1]), pixel =
    y * W + x; None: the range form, pixels ``start .. start + n`` (default: to the end of the image). An index out of range
    gives NaN rows. Not differentiable."""
    image, H, W, pixel_idx, bits, start, n = _pixel_operands(image, pixel_idx, start, n, "pixel_batch")
    if not (want_coords or want_rgb):
        raise RuntimeError("shacira_amd: pixel_batch makes coords, rgb or both")
    dev = image.device
    coords = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_coords else None
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_rgb else None
    if n == 0:
        return coords, rgb
    with _on_device(dev):
        rc = _lib.lib().shacira_pixel_batch(_ptr(image), H, W, _ptr(pixel_idx), bits, start, n, _ptr(coords), _ptr(rgb),
                                            _stream(image))
    _lib.check(rc, "pixel_batch")
    return coords, rgb


def _pixel_pred(pred, n, dev):
    """``pred`` as the fp32 [n, 3+] device operand of the loss kernels and its row stride in floats (a row-strided view such as
    ``x[:, :3]`` goes through as it is)."""
    _need_gpu(pred)
    if pred.dtype != torch.float32 or pred.dim() != 2 or pred.shape[0] != n or pred.shape[1] < 3 or pred.device != dev:
        raise RuntimeError(f"shacira_amd: pixel_loss expects fp32 pred [{n}, 3+] on {dev}, got {pred.dtype} "
                           f"{tuple(pred.shape)} on {pred.device}")
    pred = pred.detach()
    if pred.stride(1) != 1 or (n > 1 and pred.stride(0) < pred.shape[1]):
        pred = pred.contiguous()
    return pred, (pred.stride(0) if n > 1 else max(int(pred.shape[1]), 3))


@functools.lru_cache(maxsize=256)
def _pixel_loss_ws_bytes(n):
    return int(_lib.lib().shacira_pixel_loss_workspace_bytes(n))


class _PixelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, image, pixel_idx, start, out_image):
        image, H, W, pixel_idx, bits, start, n = _pixel_operands(image, pixel_idx, start,
                                                                 pred.shape[0] if pred.dim() == 2 else None, "pixel_loss")
        dev = image.device
        p, ps = _pixel_pred(pred, n, dev)
        if out_image is not None and (out_image.dtype != torch.uint8 or tuple(out_image.shape) != (H, W, 3)
                                      or out_image.device != dev or not out_image.is_contiguous()):
            raise RuntimeError(f"shacira_amd: pixel_loss out_image must be contiguous uint8 [{H}, {W}, 3] on {dev}")
        # the finish kernel overwrites all three: zeros only where nothing is enqueued
        stats = (torch.empty if n > 0 else torch.zeros)(3, dtype=torch.float64, device=dev)
        if n > 0:
            L = _lib.lib()
            with _on_device(dev):
                nbytes = _pixel_loss_ws_bytes(n)
                ws = _workspace(dev, nbytes)
                rc = L.shacira_pixel_loss_forward(_ptr(p), ps, _ptr(image), H, W, _ptr(pixel_idx), bits, start, n,
                                                  _ptr(out_image), _ptr(stats), _ptr(ws), nbytes, _stream(image))
            _lib.check(rc, "pixel_loss_forward")
        ctx.save_for_backward(p, image, pixel_idx)
        ctx.geom = (ps, H, W, bits, start, n, tuple(pred.shape))
        ctx.mark_non_differentiable(stats)
        return stats[0].to(torch.float32), stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sq, _grad_stats):
        p, image, pixel_idx = ctx.saved_tensors
        ps, H, W, bits, start, n, shape = ctx.geom
        dev = image.device
        # columns beyond the third are not read: their gradient is zero
        grad = (torch.zeros if shape[1] > 3 else torch.empty)(shape, dtype=torch.float32, device=dev)
        if n == 0:
            return grad, None, None, None, None
        g = grad_sq.detach().to(dtype=torch.float32).reshape(1).contiguous()
        rows = grad if shape[1] == 3 else torch.empty((n, 3), dtype=torch.float32, device=dev)
        with _on_device(dev):
            rc = _lib.lib().shacira_pixel_loss_backward(_ptr(p), ps, _ptr(image), H, W, _ptr(pixel_idx), bits, start, n, _ptr(g),
                                                        _ptr(rows), _stream(image))
        _lib.check(rc, "pixel_loss_backward")
        if rows is not grad:
            grad[:, :3] = rows
        return grad, None, None, None, None


def pixel_loss(pred, image, pixel_idx=None, start=0, out_image=None):
    """(sq_sum, stats) of predictions ``pred`` (fp32 [n, 3+], the first three columns) against pixels of ``image`` (uint8
    [H, W, 3]) in one pass over the image's bytes: ``sq_sum`` fp32 0-dim = sum (pred - byte / 255)^2, differentiable in ``pred``
    (once: double backward raises); ``stats`` fp64 [3] = that sum in fp64, the exact sum of squared 8-bit level differences
    (``metrics.clamped_mse`` times the element count) and the number of pixels that counted; not differentiable. ``pixel_idx``:
    int32 or int64 [n] or [n, 1]; None: pixels ``start .. start + n``. ``out_image``: uint8 [H, W, 3] that receives the
    predictions' levels at the pixels' places (duplicate indices race there, not in ``stats``). Indices out of range are skipped
    and get a zero gradient. Nothing is read back: capturable, and deterministic to the bit."""
    if pixel_idx is not None:
        pixel_idx = pixel_idx.detach()
    return _PixelLoss.apply(pred, image, pixel_idx, int(start), out_image)


# ---- view shading (include/shacira_hip.h, shacira_shade_view / shacira_shadow_* / shacira_sdf_slice_colors) ---------------------
SHADE_MODES = {"rb": _lib.SHADE_RB, "normal": _lib.SHADE_NORMAL, "matcap": _lib.SHADE_MATCAP}


def _rows(t, what, width=3, dtype=torch.float32, dev=None, n=None):
    """A dense [n, width] (or [n] for width None) operand of the shading calls, checked: dtype, device, contiguity, shape."""
    shape_ok = t.dim() == 1 if width is None else (t.dim() == 2 and t.shape[1] == width)
    if t.dtype != dtype or not shape_ok or not t.is_contiguous() or (dev is not None and t.device != dev) or \
            (n is not None and t.shape[0] != n):
        want = f"[{'n' if n is None else n}{'' if width is None else ', ' + str(width)}]"
        raise RuntimeError(f"shacira_amd: {what} must be a contiguous {dtype} {want} tensor"
                           f"{'' if dev is None else ' on ' + str(dev)}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _flags(t, what, dev, n):
    """A bool or uint8 [n] (or [n, 1]) flag array as the kernels read it: one byte per pixel, 0 or 1."""
    if t.dtype not in (torch.bool, torch.uint8) or t.numel() != n or not t.is_contiguous() or t.device != dev:
        raise RuntimeError(f"shacira_amd: {what} must be a contiguous bool or uint8 [{n}] tensor on {dev}, got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device}")
    return t


def shade_view(mode, normal=None, dirs=None, hit=None, rgb=None, matcap=None, mm=None, with_uv=False, with_rgb8=False):
    """One pass over a traced view: shade by ``mode`` ('rb', 'normal', 'matcap'), then where ``hit`` is false set ``normal`` and
    the colour to 1. ``normal`` fp32 [n, 3] is updated IN PLACE; ``rgb`` fp32 [n, 3] is updated in place when given ('rb' reads
    it) and allocated otherwise. ``matcap``: uint8 [mh, mw, 3 or 4] texture on the device; ``mm``: 3x3 rotation of the view
    (any device: nine floats are read on the host) or None. Returns (rgb, uv fp32 [n, 2] or None, rgb8 uint8 [n, 3] or None).
    'matcap' with ``matcap=None`` and ``with_uv`` returns only the coordinates (rgb None): spherical_envmap. Not
    differentiable."""
    if mode not in SHADE_MODES:
        raise RuntimeError(f"shacira_amd: shade_view mode must be one of {sorted(SHADE_MODES)}, got {mode!r}")
    _need_gpu(normal, dirs, hit, rgb, matcap)
    first = next((t for t in (normal, rgb, dirs) if t is not None), None)
    if first is None:
        raise RuntimeError("shacira_amd: shade_view needs normal or rgb")
    dev, n = first.device, first.shape[0]
    if mode != "rb" and normal is None:
        raise RuntimeError(f"shacira_amd: shade_view mode {mode!r} needs normal")
    if normal is not None:
        _rows(normal, "shade_view normal", dev=dev, n=n)
    if mode == "matcap":
        if dirs is None:
            raise RuntimeError("shacira_amd: shade_view mode 'matcap' needs dirs")
        _rows(dirs, "shade_view dirs", dev=dev, n=n)
    coords_only = mode == "matcap" and matcap is None
    if coords_only and (not with_uv or with_rgb8 or hit is not None or rgb is not None):
        raise RuntimeError("shacira_amd: shade_view without a matcap texture computes the coordinates only (with_uv=True)")
    if with_uv and mode != "matcap":
        raise RuntimeError("shacira_amd: shade_view with_uv needs mode 'matcap'")
    mh = mw = mc = 0
    if mode == "matcap" and matcap is not None:
        if matcap.dtype != torch.uint8 or matcap.dim() != 3 or not matcap.is_contiguous() or matcap.device != dev:
            raise RuntimeError(f"shacira_amd: shade_view matcap must be a contiguous uint8 [mh, mw, 3 or 4] tensor on {dev}, got "
                               f"{matcap.dtype} {tuple(matcap.shape)} on {matcap.device}")
        mh, mw, mc = matcap.shape
    if hit is not None:
        _flags(hit, "shade_view hit", dev, n)
    if rgb is not None:
        _rows(rgb, "shade_view rgb", dev=dev, n=n)
    elif mode == "rb":
        raise RuntimeError("shacira_amd: shade_view mode 'rb' needs rgb")
    elif not coords_only:
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    mm_host = None
    if mm is not None and mode == "matcap":
        flat = [float(v) for v in mm.detach().to("cpu", torch.float32).reshape(-1)]
        if len(flat) != 9:
            raise RuntimeError(f"shacira_amd: shade_view mm must be 3 x 3, got {tuple(mm.shape)}")
        mm_host = (ctypes.c_float * 9)(*flat)
    uv = torch.empty((n, 2), dtype=torch.float32, device=dev) if with_uv else None
    rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev) if with_rgb8 else None
    with _on_device(dev):
        rc = _lib.lib().shacira_shade_view(n, SHADE_MODES[mode], _ptr(normal), _ptr(dirs) if mode == "matcap" else None, _ptr(hit),
                                           mm_host, _ptr(matcap) if mode == "matcap" else None, mh, mw, mc, _ptr(rgb), _ptr(uv),
                                           _ptr(rgb8), _stream(first))
    _lib.check(rc, "shade_view")
    return rgb, uv, rgb8


def shadow_rays(origins, dirs, depth, xyz, normal, hit, point_light=(1.5, 4.5, 1.5), min_y=-2.0, seed=0):
    """The ground plane y = ``min_y`` and one shadow ray per pixel towards the jittered point light. ``depth`` fp32 [n] or
    [n, 1], ``xyz`` / ``normal`` fp32 [n, 3] and ``hit`` bool [n] are updated IN PLACE where the plane is in front. Returns
    (shadow origins fp32 [n, 3], shadow dirs fp32 [n, 3], light_hit bool [n], plane_hit bool [n]). The jitter is a function of
    (seed, ray index). Not differentiable."""
    _need_gpu(origins, dirs, depth, xyz, normal, hit)
    dev, n = origins.device, origins.shape[0]
    for name, t in (("origins", origins), ("dirs", dirs), ("xyz", xyz), ("normal", normal)):
        _rows(t, f"shadow_rays {name}", dev=dev, n=n)
    if depth.dtype != torch.float32 or depth.numel() != n or not depth.is_contiguous() or depth.device != dev:
        raise RuntimeError(f"shacira_amd: shadow_rays depth must be a contiguous fp32 [{n}] tensor on {dev}, got {depth.dtype} "
                           f"{tuple(depth.shape)} on {depth.device}")
    _flags(hit, "shadow_rays hit", dev, n)
    light = (ctypes.c_float * 3)(*[float(v) for v in point_light])
    so = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sd = torch.empty((n, 3), dtype=torch.float32, device=dev)
    light_hit = torch.empty((n,), dtype=torch.bool, device=dev)
    plane_hit = torch.empty((n,), dtype=torch.bool, device=dev)
    with _on_device(dev):
        rc = _lib.lib().shacira_shadow_rays(n, _ptr(origins), _ptr(dirs), light, float(min_y), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                            _ptr(depth), _ptr(xyz), _ptr(normal), _ptr(hit), _ptr(so), _ptr(sd), _ptr(light_hit),
                                            _ptr(plane_hit), _stream(origins))
    _lib.check(rc, "shadow_rays")
    return so, sd, light_hit, plane_hit


def shadow_apply(height, width, occluded, light_hit, rgb):
    """shadow = occluded & light_hit; the map 1 / 0.7 blurred over the [height, width] view as
    scipy.ndimage.gaussian_filter(sigma=2) does; ``rgb`` fp32 [height * width, 3 or 4] is multiplied IN PLACE (first three
    channels). Returns shadow bool [height * width]. Not differentiable."""
    _need_gpu(occluded, light_hit, rgb)
    H, W = int(height), int(width)
    dev, n = rgb.device, H * W
    if H < 1 or W < 1:
        raise RuntimeError(f"shacira_amd: shadow_apply needs a view of at least 1 x 1, got {H} x {W}")
    if rgb.dtype != torch.float32 or rgb.dim() != 2 or rgb.shape[0] != n or rgb.shape[1] not in (3, 4) or not rgb.is_contiguous():
        raise RuntimeError(f"shacira_amd: shadow_apply rgb must be a contiguous fp32 [{n}, 3 or 4] tensor (the shadows are blurred "
                           f"over the {H} x {W} view), got {rgb.dtype} {tuple(rgb.shape)}")
    _flags(occluded, "shadow_apply occluded", dev, n)
    _flags(light_hit, "shadow_apply light_hit", dev, n)
    shadow = torch.empty((n,), dtype=torch.bool, device=dev)
    nbytes = int(_lib.lib().shacira_shadow_apply_workspace_bytes(H, W))
    ws = _workspace(dev, nbytes)
    with _on_device(dev):
        rc = _lib.lib().shacira_shadow_apply(H, W, rgb.shape[1], _ptr(occluded), _ptr(light_hit), _ptr(shadow), _ptr(rgb),
                                             _ptr(ws), nbytes, _stream(rgb))
    _lib.check(rc, "shadow_apply")
    return shadow


def sdf_slice_colors(d):
    """The colour map of an SDF slice: fp32 distances of any shape -> fp32 [*shape, 3] (orange inside, blue to yellow outside,
    grey isolines every 0.04, black at the surface). Not differentiable."""
    _need_gpu(d)
    if d.dtype != torch.float32 or not d.is_contiguous():
        raise RuntimeError(f"shacira_amd: sdf_slice_colors expects a contiguous fp32 tensor, got {d.dtype} {tuple(d.shape)}")
    vis = torch.empty((*d.shape, 3), dtype=torch.float32, device=d.device)
    with _on_device(d.device):
        rc = _lib.lib().shacira_sdf_slice_colors(d.numel(), _ptr(d), _ptr(vis), _stream(d))
    _lib.check(rc, "sdf_slice_colors")
    return vis
