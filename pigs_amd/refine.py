"""Refinement: prune and split (or clone) Gaussians on the GPU, with one host read.

Stands in for the reference's chains of boolean indexing, ``torch.linalg.eig``, ``repeat_interleave`` and ``cat``:

    mode="split"   Model.forward(split=True): the prune of model_pn.py:703-714 and Model.split (:578-605).
                   Output rows: the rows with ``keep & ~split`` in input order, then for every split parent in
                   input order its two children (mean - e, mean + e), adjacent, with ``value_scale * values``
                   (default 0.5, the reference's ``/ 2.0``) and the parent's scaling and transforms.
                   e = lambda_max * v of the covariance [[s0, tau], [tau, s1]], tau = tanh(t) sqrt(s0 s1) -- the unit
                   eigenvector times the eigenVALUE, as model_pn.py:587-589 has it -- signed so that e_x > 0, or
                   e_x = 0 and e_y > 0.  e is a constant for autograd (:584-585).
    mode="clone"   the densification of test_no_mlp.py:198-240: all kept rows in input order, then one unchanged
                   copy of every split parent.

Both return N' = (kept rows) + (split rows) rows and the maps ``source`` [N'] (int64: the input row of every output
row) and ``child`` [N'] (int32: -1 kept row, 0 / 1 the -e / +e child, 0 a copy), through which any other per-Gaussian
array follows with one ``index_select`` and one ``where``.  The effective split set is ``split & keep``.

Five HIP launches (C ABI: pigs_refine_*) and ONE host wait: the pinned read of the two row totals that size the
outputs.  d = 2, float32 / float64, GPU only.
"""
import collections
import ctypes

import torch

from . import _lib

_DTYPES = {torch.float32: 0, torch.float64: 1}
MODES = {"split": 0, "clone": 1}
ROWS_PER_WORKGROUP = 1024      # PIGS_REFINE_ROWS: rows per workgroup of the index kernels
SCAN_WIDTH = 256               # PIGS_REFINE_SCAN_WIDTH: workgroup totals per pass of the one-workgroup scan

Refined = collections.namedtuple("Refined", "means scaling transforms values source child")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode must be 'split' or 'clone', got {mode!r}")
    return MODES[mode]


def _check_mask_type(name, mask):
    if mask is None:
        return
    if isinstance(mask, torch.Tensor) and mask.requires_grad:
        raise TypeError(f"{name} is a mask: it cannot require a gradient")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise TypeError(f"{name} must be a torch.bool tensor or None")


def _check_mask(name, mask, N, device):
    _check_mask_type(name, mask)
    if mask is None:
        return None
    if mask.dim() != 1 or mask.shape[0] != N:
        raise ValueError(f"{name} must be [N] = [{N}], got {tuple(mask.shape)}")
    if not mask.is_cuda or (device is not None and mask.device != device):
        raise RuntimeError(f"{name} is on {mask.device}: refinement runs on one GPU (no CPU fallback)")
    return mask.contiguous()


def _index(keep, split, mode, N, device):
    """kept_pos [N], child_pos [N] (device, int64) and the host's (n_kept, n_split): the path's one host wait."""
    lib = _lib.load()
    kept_pos = torch.empty(N, dtype=torch.int64, device=device)
    child_pos = torch.empty(N, dtype=torch.int64, device=device)
    if N == 0:
        return kept_pos, child_pos, 0, 0
    ws_bytes = lib.pigs_refine_workspace_bytes(N)
    if ws_bytes == 0:
        raise NotImplementedError(f"N = {N}: refinement takes up to 2^31 - 1 rows")
    workspace = torch.empty(ws_bytes // 8, dtype=torch.int64, device=device)
    counts = torch.empty(2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        rc = lib.pigs_refine_index(mode, N, _ptr(keep), _ptr(split), _ptr(workspace), ws_bytes, _ptr(kept_pos),
                                   _ptr(child_pos), _ptr(counts), _stream(device))
        _lib.check(rc, "pigs_refine_index")
        host = torch.empty(2, dtype=torch.int64, pin_memory=True)
        host.copy_(counts)         # synchronises: stands for the reference's indices.sum().item()
    return kept_pos, child_pos, int(host[0]), int(host[1])


def _apply(mode, value_scale, kept_pos, child_pos, rows, arrays, device):
    """arrays = (means, scaling, transforms [N], values) or None (the maps alone) -> outputs, source, child"""
    lib = _lib.load()
    N = kept_pos.shape[0]
    source = torch.empty(rows, dtype=torch.int64, device=device)
    child = torch.empty(rows, dtype=torch.int32, device=device)
    outs, dtype, c = (None,) * 4, 0, 1
    if arrays is not None:
        outs = tuple(torch.empty((rows,) + a.shape[1:], dtype=a.dtype, device=device) for a in arrays)
        dtype, c = _DTYPES[arrays[0].dtype], arrays[3].shape[1]
    else:
        arrays = (None,) * 4
    with torch.cuda.device(device):
        rc = lib.pigs_refine_apply(dtype, mode, c, N, rows, value_scale, _ptr(kept_pos), _ptr(child_pos),
                                   *[_ptr(a) for a in arrays], *[_ptr(o) for o in outs], _ptr(source), _ptr(child),
                                   _stream(device))
    _lib.check(rc, "pigs_refine_apply")
    return outs, source, child


def refine_index(keep, split, mode="split"):
    """The maps alone, ``(source, child)``, for arrays the library does not know (optimiser state, boundary
    flags): ``new = old.index_select(0, source)``, then ``torch.where(child >= 0, fresh, new)`` where the children
    start from something else.  ``keep`` / ``split``: torch.bool [N] on the GPU; one of them may be None."""
    m = _mode(mode)
    ref = keep if keep is not None else split
    if ref is None:
        raise ValueError("refine_index needs keep or split (their length is N)")
    if not isinstance(ref, torch.Tensor) or ref.dim() != 1:
        raise TypeError("keep and split must be 1-d torch.bool tensors")
    N = ref.shape[0]
    keep = _check_mask("keep", keep, N, None)
    split = _check_mask("split", split, N, keep.device if keep is not None else None)
    device = ref.device
    kept_pos, child_pos, n_kept, n_split = _index(keep, split, m, N, device)
    _, source, child = _apply(m, 1.0, kept_pos, child_pos, n_kept + n_split, None, device)
    return source, child


def _aligned(t):
    # a row of means / scaling is one 8- or 16-byte access
    return t if t.data_ptr() % (2 * t.element_size()) == 0 else t.clone()


class _SplitGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, scaling, transforms, values, keep, split, mode, value_scale):
        device = means.device
        N = means.shape[0]
        arrays = (_aligned(means.contiguous()), _aligned(scaling.contiguous()), transforms.contiguous().reshape(N),
                  values.contiguous())
        kept_pos, child_pos, n_kept, n_split = _index(keep, split, mode, N, device)
        rows = n_kept + n_split
        (o_means, o_scaling, o_transforms, o_values), source, child = _apply(
            mode, value_scale, kept_pos, child_pos, rows, arrays, device)
        ctx.save_for_backward(kept_pos, child_pos)
        ctx.refine = (mode, value_scale, rows, transforms.shape, values.shape[1], means.dtype)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(source, child)
        return o_means, o_scaling, o_transforms.reshape((rows,) + transforms.shape[1:]), o_values, source, child

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_means, g_scaling, g_transforms, g_values, _g_source, _g_child):
        kept_pos, child_pos = ctx.saved_tensors
        mode, value_scale, rows, t_shape, c, dtype = ctx.refine
        gouts = [g_means, g_scaling, g_transforms, g_values]
        wanted = ctx.needs_input_grad[:4]
        if all(g is None for g in gouts) or not any(wanted):
            return (None,) * 8
        lib = _lib.load()
        device = kept_pos.device
        N = kept_pos.shape[0]
        gouts = [_aligned(g.contiguous()) if g is not None else None for g in gouts]
        shapes = ((N, 2), (N, 2), (N,), (N, c))
        gins = [torch.empty(s, dtype=dtype, device=device) if w else None for s, w in zip(shapes, wanted)]
        with torch.cuda.device(device):
            rc = lib.pigs_refine_backward(_DTYPES[dtype], mode, c, N, rows, value_scale, _ptr(kept_pos), _ptr(child_pos),
                                          *[_ptr(g) for g in gouts], *[_ptr(g) for g in gins], _stream(device))
        _lib.check(rc, "pigs_refine_backward")
        if gins[2] is not None:
            gins[2] = gins[2].reshape(t_shape)
        return (*gins, None, None, None, None)


def _check(means, scaling, transforms, values):
    names = ("means", "scaling", "transforms", "values")
    arrays = (means, scaling, transforms, values)
    for n, a in zip(names, arrays):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor")
    if means.dim() != 2 or means.shape[1] != 2:
        raise NotImplementedError(f"means must be [N, 2] (d = 2), got {tuple(means.shape)}")
    N = means.shape[0]
    if scaling.dim() != 2 or scaling.shape[1] != 2:
        raise NotImplementedError(f"scaling must be [N, 2] (d = 2), got {tuple(scaling.shape)}")
    if transforms.dim() not in (1, 2) or (transforms.dim() == 2 and transforms.shape[1] != 1):
        raise NotImplementedError(f"transforms must be [N] or [N, 1] (d = 2), got {tuple(transforms.shape)}")
    if values.dim() != 2 or values.shape[1] < 1:
        raise ValueError(f"values must be [N, c] with c >= 1, got {tuple(values.shape)}")
    for n, a in zip(names[1:], arrays[1:]):
        if a.shape[0] != N:
            raise ValueError(f"{n} holds {a.shape[0]} rows, means {N}")
    for n, a in zip(names, arrays):
        if not a.is_cuda or a.device != means.device:
            raise RuntimeError(f"{n} is on {a.device}, means on {means.device}: refinement runs on one GPU "
                               "(no CPU fallback)")
    if means.dtype not in _DTYPES or any(a.dtype != means.dtype for a in arrays):
        raise TypeError(f"dtypes {[str(a.dtype) for a in arrays]}: float32 or float64, all alike")


def split_gaussians(means, scaling, transforms, values, split, keep=None, *, mode="split", value_scale=0.5):
    """Prune the rows outside ``keep`` and split (or clone) the rows in ``split & keep``; see the module text.

    means [N,2], scaling [N,2] (variances), transforms [N,1] or [N], values [N,c]: float32 or float64 on one GPU;
    ``split`` / ``keep``: torch.bool [N] or None (none / all; ``split=None`` is prune-only).  Returns the named tuple
    ``(means, scaling, transforms, values, source, child)``; differentiable with respect to the four float inputs.
    ``value_scale`` applies to the children of mode="split" only."""
    m = _mode(mode)
    _check_mask_type("keep", keep)
    _check_mask_type("split", split)
    _check(means, scaling, transforms, values)
    N = means.shape[0]
    keep = _check_mask("keep", keep, N, means.device)
    split = _check_mask("split", split, N, means.device)
    return Refined(*_SplitGaussians.apply(means, scaling, transforms, values, keep, split, m, float(value_scale)))
