"""advance_gaussians: the dynamics network's deltas applied to the Gaussians, in two HIP launches and one for the backward.

The loop with the network (main_pn.py:171-232 driving model_pn.Model) ends every time step with an O(N) chain of a few
dozen small torch launches: four strided slices of the network's output (model_pn.py:270-273), six ``detach().clone()``
(:677-682), the masked update (:684-687), the periodic wrap (:689-693), ``build_full_covariances`` and
``flatten_covariances`` (:695-698), and in ``compute_loss`` four masked mean squares (:878-882).  Six of those lines
index with a boolean mask and wait for the host, so the step cannot be captured into a graph.  Here (C ABI:
pigs_advance_forward / pigs_advance_backward):

    out = advance_gaussians(means, u, scaling, transforms, deltas, boundary_mask, wrap=None)
    out.means [N,2]  out.u [N,c]  out.scaling [N,2]  out.transforms (the shape of ``transforms``: [N,1] or [N])
    out.covariances [N,3]  out.conics [N,3]  out.full_covariances [N,2,2]  out.full_conics [N,2,2]
    out.penalty [4], in the order of ADVANCE_PENALTY_COLUMNS = ("dmeans", "dscaling", "dtransforms", "du")

``deltas`` is the network's output as it comes, [N, 5 + c] or [1, N, 5 + c]: columns 0:2 dmeans, 2:4 dscaling, 4:5
dtransforms, 5:5+c du.  It is never sliced, and its gradient is ONE [N, 5 + c] tensor.  ``boundary_mask`` is torch.bool
[N] or [N, 1]; True marks a FREE Gaussian (m = 1), as the reference uses it:

    means' = means + dmeans m        scaling' = scaling exp(dscaling m)
    transforms' = transforms + dtransforms m        u' = u + du m

A boundary row (m = 0) keeps its inputs bit for bit, whatever its deltas hold.  ``wrap=(lo, hi)``: afterwards a coordinate
of means' > hi is lowered by hi - lo and one < lo raised by it (one shift, strict inequalities: GaussianAdam's rule); the
gradient passes through.  The covariances and conics are those of ``build_covariances(out.scaling, out.transforms)``,
bit for bit, and the full forms hold the same values.  ``penalty[k]`` is ``torch.mean(x[mask] ** 2)`` of block k: the sum
over the free rows divided by n_free times the block's width, NaN with no free row; the caller applies the model's weights.
Nothing is read back to the host.  The inputs are never written: they are the previous state (the ``prev_*`` of :677-682).

Gradients may arrive at any subset of the nine outputs and leave towards means, u, scaling, transforms and deltas.
d = 2, c = 1..4, float32 / float64, contiguous GPU tensors, N >= 1; no CPU fallback.  Capturable into a hipGraph.
"""
import collections

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream

ADVANCE_PENALTY_COLUMNS = ("dmeans", "dscaling", "dtransforms", "du")
DELTA_COLUMNS = 5        # dmeans 2, dscaling 2, dtransforms 1; then du c

Advanced = collections.namedtuple(
    "Advanced", "means u scaling transforms covariances conics full_covariances full_conics penalty")


def _check(means, u, scaling, transforms, deltas, boundary_mask, wrap):
    """the refusals, with the exception types of optim._check; returns (lo, hi) or None"""
    if wrap is not None:
        lo, hi = (float(x) for x in wrap)
        if not lo < hi:
            raise ValueError(f"wrap = ({lo}, {hi}): needs lo < hi")
        wrap = (lo, hi)
    names = ("means", "u", "scaling", "transforms", "deltas", "boundary_mask")
    arrays = (means, u, scaling, transforms, deltas, boundary_mask)
    for n, a in zip(names, arrays):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor")
    if means.dim() != 2 or means.shape[1] != 2:
        raise NotImplementedError(f"means must be [N, 2] (d = 2), got {tuple(means.shape)}")
    N = means.shape[0]
    if N < 1:
        raise ValueError("no Gaussians: N must be at least 1")
    if scaling.dim() != 2 or scaling.shape[1] != 2:
        raise NotImplementedError(f"scaling must be [N, 2] (d = 2), got {tuple(scaling.shape)}")
    if transforms.dim() not in (1, 2) or (transforms.dim() == 2 and transforms.shape[1] != 1):
        raise NotImplementedError(f"transforms must be [N] or [N, 1] (d = 2), got {tuple(transforms.shape)}")
    if u.dim() != 2 or not 1 <= u.shape[1] <= 4:
        raise NotImplementedError(f"u must be [N, c] with c = 1..4, got {tuple(u.shape)}")
    for n, a in zip(names[1:4], arrays[1:4]):
        if a.shape[0] != N:
            raise ValueError(f"{n} holds {a.shape[0]} rows, means {N}")
    width = DELTA_COLUMNS + u.shape[1]
    if tuple(deltas.shape) not in ((N, width), (1, N, width)):
        raise ValueError(f"deltas must be [N, 5 + c] = [{N}, {width}] (a leading 1 allowed), got {tuple(deltas.shape)}")
    if tuple(boundary_mask.shape) not in ((N,), (N, 1)):
        raise ValueError(f"boundary_mask must be [N] or [N, 1] with N = {N}, got {tuple(boundary_mask.shape)}")
    floats = arrays[:5]
    if means.dtype not in _DTYPES or any(a.dtype != means.dtype for a in floats):
        raise TypeError(f"dtypes {[str(a.dtype) for a in floats]}: float32 or float64, all alike")
    if boundary_mask.dtype != torch.bool:
        raise TypeError(f"boundary_mask must be torch.bool, got {boundary_mask.dtype}")
    for n, a in zip(names, arrays):
        if not a.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    for n, a in zip(names, arrays):
        if not a.is_cuda or a.device != means.device:
            raise RuntimeError(f"{n} is on {a.device}" + (f", means on {means.device}" if a is not means else "")
                               + ": the update runs on one GPU (no CPU fallback)")
    for n, a in ((names[0], means), (names[2], scaling)):
        if a.data_ptr() % (2 * a.element_size()):
            raise ValueError(f"{n} must be aligned to a row ({2 * a.element_size()} bytes)")
    return wrap


def _rows_of_two(g):
    """an incoming gradient of a [N, 2] output, as the kernel reads it: contiguous and aligned to a row"""
    if g is None:
        return None
    g = g.contiguous()
    return g.clone() if g.data_ptr() % (2 * g.element_size()) else g


class _Advance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, u, scaling, transforms, deltas, mask, wrap):
        lib = _lib.load()
        N, c = u.shape
        dtype, device = means.dtype, means.device

        def new(*shape):
            return torch.empty(shape, dtype=dtype, device=device)
        outs = (new(N, 2), new(N, c), new(N, 2), torch.empty_like(transforms), new(N, 3), new(N, 3), new(N, 2, 2),
                new(N, 2, 2), new(4))
        nbytes = lib.pigs_advance_scratch_bytes(N)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        lo, hi = wrap if wrap is not None else (0.0, 0.0)
        with torch.cuda.device(device):
            rc = lib.pigs_advance_forward(_DTYPES[dtype], c, N, int(wrap is not None), lo, hi, _ptr(means), _ptr(u),
                                          _ptr(scaling), _ptr(transforms), _ptr(deltas), _ptr(mask), _ptr(scratch), nbytes,
                                          *[_ptr(o) for o in outs], _stream(device))
        _lib.check(rc, "pigs_advance_forward")
        ctx.save_for_backward(outs[2], outs[3], deltas, mask, scratch)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gout):
        o_scaling, o_transforms, deltas, mask, scratch = ctx.saved_tensors
        needs = ctx.needs_input_grad[:5]
        if all(g is None for g in gout) or not any(needs):
            return (None,) * 7
        lib = _lib.load()
        N, c = o_scaling.shape[0], deltas.shape[1] - DELTA_COLUMNS
        gout = [g.contiguous() if g is not None else None for g in gout]
        gout[0], gout[2] = _rows_of_two(gout[0]), _rows_of_two(gout[2])
        like = (o_scaling, None, o_scaling, o_transforms, deltas)
        grads = [None] * 5
        for k, need in enumerate(needs):
            if need:
                grads[k] = (torch.empty((N, c), dtype=deltas.dtype, device=deltas.device) if k == 1
                            else torch.empty_like(like[k]))
        with torch.cuda.device(deltas.device):
            rc = lib.pigs_advance_backward(_DTYPES[deltas.dtype], c, N, _ptr(o_scaling), _ptr(o_transforms), _ptr(deltas),
                                           _ptr(mask), _ptr(scratch), *[_ptr(g) for g in gout], *[_ptr(g) for g in grads],
                                           _stream(deltas.device))
        _lib.check(rc, "pigs_advance_backward")
        return (*grads, None, None)


def advance_gaussians(means, u, scaling, transforms, deltas, boundary_mask, wrap=None):
    """The state update, the next covariances and the conservation penalty; see the module text.  Returns ``Advanced``."""
    wrap = _check(means, u, scaling, transforms, deltas, boundary_mask, wrap)
    packed = deltas.reshape(deltas.shape[-2], deltas.shape[-1])      # a view: the gradient keeps the caller's shape
    mask = boundary_mask.reshape(-1).view(torch.uint8)
    return Advanced(*_Advance.apply(means, u, scaling, transforms, packed, mask, wrap))
