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

The criteria that choose the ``split`` mask, on the device and without a host wait (C ABI: pigs_criterion_*):

    split_criterion   the whole of model_pn.py:716-754: two sampling passes and the quantile rule
    split_mask        the quantile rule alone (:733-754) from the three sampled fields
    threshold_mask    score > mean + k std, the rule of test_no_mlp.py:203-205
"""
import collections

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream

MODES = {"split": 0, "clone": 1}
ROWS_PER_WORKGROUP = 1024      # PIGS_REFINE_ROWS: rows per workgroup of the index kernels
SCAN_WIDTH = 256               # PIGS_REFINE_SCAN_WIDTH: workgroup totals per pass of the one-workgroup scan

Refined = collections.namedtuple("Refined", "means scaling transforms values source child")


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


# ---- the criteria: which rows to split -------------------------------------------------------------------------
VARIANTS = {"auto": 0, "one": 1, "many": 2}
CRITERION_LDS_VALUES = 16384   # PIGS_CRITERION_LDS_VALUES: most values n * c of the one-workgroup variant
CRITERION_MAX_VALUES = 1 << 24  # n * c beyond this is refused, as torch.quantile refuses it


def _variant(variant, values):
    if variant not in VARIANTS:
        raise ValueError(f"variant must be 'auto', 'one' or 'many', got {variant!r}")
    if values > CRITERION_MAX_VALUES:
        raise NotImplementedError(f"{values} values: the criteria take up to 2^24 (as torch.quantile)")
    if variant == "one" and values > CRITERION_LDS_VALUES:
        raise NotImplementedError(f"variant='one' takes up to {CRITERION_LDS_VALUES} values, got {values}")
    return VARIANTS[variant], variant == "one" or (variant == "auto" and values <= CRITERION_LDS_VALUES)


def _row_mask(name, mask, n, device):
    """a bool [n] or [n, 1] on the device -> contiguous [n]"""
    _check_mask_type(name, mask)
    if mask is not None and mask.dim() == 2 and mask.shape[1] == 1:
        mask = mask.reshape(-1)
    return _check_mask(name, mask, n, device)


def _criterion_workspace(lib, one, dtype, n, c, device):
    if one:
        return None, 0
    ws_bytes = lib.pigs_criterion_workspace_bytes(_DTYPES[dtype], n, c)
    return torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=device), ws_bytes


def split_mask(sample_u, prev_sample_u, density, boundary_mask=None, *, q=0.98, variant="auto", return_stats=False):
    """The quantile rule of model_pn.py:733-754 as a torch.bool mask [n] on the device, without a host wait:

        w = 1 - (density - density.min()) / density.max();   metric = (sample_u - prev_sample_u) ** 2 * w
        mask = (metric > torch.quantile(metric, q)).any(-1) & boundary_mask

    sample_u, prev_sample_u [n, c] and density [n] or [n, 1]: float32 or float64 on one GPU, all alike;
    ``boundary_mask``: torch.bool [n] or [n, 1], or None (all).  Inputs that require a gradient are detached (the
    reference computes the criterion under no_grad).  ``variant``: "auto", "one" (one launch of one workgroup, up to
    CRITERION_LDS_VALUES values n * c) or "many" (6 launches in float32, 10 in float64).  With ``return_stats`` the
    result is ``(mask, metric [n, c], stats [4])``, stats = (quantile, x_lo, x_hi, 1.0 if a NaN was seen else 0.0);
    a NaN makes the quantile NaN and the mask all False."""
    names = ("sample_u", "prev_sample_u", "density")
    arrays = (sample_u, prev_sample_u, density)
    for name, a in zip(names, arrays):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if sample_u.dim() != 2 or sample_u.shape[1] < 1:
        raise ValueError(f"sample_u must be [n, c] with c >= 1, got {tuple(sample_u.shape)}")
    n, c = sample_u.shape
    if prev_sample_u.shape != sample_u.shape:
        raise ValueError(f"prev_sample_u must be [n, c] = [{n}, {c}], got {tuple(prev_sample_u.shape)}")
    if tuple(density.shape) not in ((n,), (n, 1)):
        raise ValueError(f"density must be [n] or [n, 1] with n = {n}, got {tuple(density.shape)}")
    for name, a in zip(names, arrays):
        if not a.is_cuda or a.device != sample_u.device:
            raise RuntimeError(f"{name} is on {a.device}, sample_u on {sample_u.device}: the criterion runs on one GPU "
                               "(no CPU fallback)")
    if sample_u.dtype not in _DTYPES or any(a.dtype != sample_u.dtype for a in arrays):
        raise TypeError(f"dtypes {[str(a.dtype) for a in arrays]}: float32 or float64, all alike")
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q must lie in [0, 1], got {q}")
    device, dtype = sample_u.device, sample_u.dtype
    boundary_mask = _row_mask("boundary_mask", boundary_mask, n, device)
    code, one = _variant(variant, n * c)
    mask = torch.empty(n, dtype=torch.bool, device=device)
    metric = torch.empty((n, c), dtype=dtype, device=device) if return_stats else None
    stats = torch.empty(4, dtype=dtype, device=device) if return_stats else None
    if n > 0:
        lib = _lib.load()
        su, pu, dn = (a.detach().contiguous() for a in arrays)
        workspace, ws_bytes = _criterion_workspace(lib, one, dtype, n, c, device)
        with torch.cuda.device(device):
            rc = lib.pigs_criterion_quantile_mask(_DTYPES[dtype], code, c, n, q, _ptr(su), _ptr(pu), _ptr(dn),
                                                  _ptr(boundary_mask), _ptr(workspace), ws_bytes, _ptr(metric), _ptr(stats),
                                                  _ptr(mask), _stream(device))
        _lib.check(rc, "pigs_criterion_quantile_mask")
    elif return_stats:
        stats.fill_(float("nan"))
    return (mask, metric, stats) if return_stats else mask


def threshold_mask(score, keep=None, *, k=1.6, variant="auto", return_stats=False):
    """The rule of test_no_mlp.py:203-205 as a torch.bool mask [n] on the device, without a host wait:

        mask = (score > torch.mean(score) + k * torch.std(score)) & keep

    score [n]: float32 or float64 on the GPU (detached if it requires a gradient); ``keep``: torch.bool [n] or None.
    The mean and the squared deviations are summed in double; n = 1 (std NaN) and a NaN score give an all-False mask.
    ``variant``: "auto", "one" (one launch, n up to CRITERION_LDS_VALUES) or "many" (three launches).  With
    ``return_stats`` the result is ``(mask, stats [3])``, stats = (threshold, mean, std)."""
    if not isinstance(score, torch.Tensor):
        raise TypeError("score must be a torch.Tensor")
    if score.dim() != 1:
        raise ValueError(f"score must be [n], got {tuple(score.shape)}")
    if not score.is_cuda:
        raise RuntimeError(f"score is on {score.device}: the criterion runs on one GPU (no CPU fallback)")
    if score.dtype not in _DTYPES:
        raise TypeError(f"dtype {score.dtype}: float32 or float64")
    k = float(k)
    if k != k:
        raise ValueError("k must not be NaN")
    n, device, dtype = score.shape[0], score.device, score.dtype
    keep = _check_mask("keep", keep, n, device)
    code, one = _variant(variant, n)
    mask = torch.empty(n, dtype=torch.bool, device=device)
    stats = torch.empty(3, dtype=dtype, device=device) if return_stats else None
    if n > 0:
        lib = _lib.load()
        sc = score.detach().contiguous()
        workspace, ws_bytes = _criterion_workspace(lib, one, dtype, n, 1, device)
        with torch.cuda.device(device):
            rc = lib.pigs_criterion_meanstd_mask(_DTYPES[dtype], code, n, k, _ptr(sc), _ptr(keep), _ptr(workspace), ws_bytes,
                                                 _ptr(stats), _ptr(mask), _stream(device))
        _lib.check(rc, "pigs_criterion_meanstd_mask")
    elif return_stats:
        stats.fill_(float("nan"))
    return (mask, stats) if return_stats else mask


def _one_pass(sampler, n, c):
    """values and the channel of ones in ONE preprocess: within the sampler's 4 channels, and not where the extra
    channel would take a pass that runs binned (c <= 2 there) off that path"""
    if c + 1 > 4:
        return False
    backend = getattr(sampler, "backend", "auto")
    binned = backend == "binned" or (backend == "auto" and n * n >= getattr(sampler, "BINNED_AUTO_MIN_PAIRS", 1 << 62))
    return c + 1 <= 2 or not binned


def split_criterion(sampler, means, values, covariances, conics, prev_means, prev_values, prev_covariances, prev_conics,
                    boundary_mask=None, *, q=0.98):
    """The whole criterion of Model.forward(split=True), model_pn.py:716-754, under no_grad: the current field and the
    density of the current Gaussians at their own means, the previous field there, then ``split_mask``.  Returns the
    torch.bool mask [n] that goes into ``split_gaussians`` / ``refine_index``; nothing waits for the device.

    The density (a field of ones, :729-732) rides as one more channel of the first pass where the sampler takes it in
    the same path (c + 1 <= 4 channels; a pass that runs binned keeps its c <= 2), else it is a pass of its own.  The
    sampler picks dense or binned as it always does, with either host and with ``periodic=``.  The sampler is left
    bound to the LAST pass: the previous Gaussians at the current means."""
    with torch.no_grad():
        means, values = means.detach(), values.detach()
        if values.dim() == 1:
            values = values.reshape(-1, 1)
        n, c = values.shape
        ones = torch.ones((n, 1), dtype=values.dtype, device=values.device)
        if _one_pass(sampler, n, c):
            sampler.preprocess(means, torch.cat((values, ones), -1), covariances, conics, means)
            both = sampler.sample_gaussians()
            sample_u, density = both[:, :c], both[:, c]
        else:
            sampler.preprocess(means, values, covariances, conics, means)
            sample_u = sampler.sample_gaussians()
            sampler.preprocess(means, ones, covariances, conics, means)
            density = sampler.sample_gaussians()
        sampler.preprocess(prev_means, prev_values, prev_covariances, prev_conics, means)
        prev_sample_u = sampler.sample_gaussians()
        return split_mask(sample_u, prev_sample_u.reshape(n, c), density, boundary_mask, q=q)
