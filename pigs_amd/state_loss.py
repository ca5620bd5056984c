"""state_loss_terms: the TEST problem's state terms in one HIP launch and one for the backward, with no host wait.

``Problem.TEST`` is the problem the reference's training script constructs (main_pn.py:30-34).  Its loss never looks at a
sample: ``pde_loss`` (model_pn.py:851-852), ``bc_loss`` (:854-861) and ``conservation_loss`` (:866-876) read the Gaussians'
new state and the network's deltas through three ``if torch.any(...)`` and about seventeen boolean indexings, each of
which waits for the host, so the step cannot be captured.  Here (C ABI: pigs_state_loss_forward / pigs_state_loss_backward):

    terms = state_loss_terms(means, u, deltas, boundary_mask, wall=0.8, drift=5.0)      # [8], the inputs' dtype

``means [N,2]`` and ``u [N,c]`` are the NEW state (``advance_gaussians(...).means`` / ``.u``); ``deltas`` is the network's
packed output, [N, 5 + c] or [1, N, 5 + c] (columns 0:2 dmeans, 5:5+c du, as in pigs_amd.advance); ``boundary_mask`` is
torch.bool [N] or [N, 1], True = a FREE Gaussian.  Over the free rows, with F their count, y = means[:, 1], dx, dy =
deltas[:, 0], deltas[:, 1], du = deltas[:, 5:5+c], u0 = u[:, 0] and LOW = {y < -wall}, HIGH = {y > wall}, MID = {|y| < wall}
(strict, in the dtype, against ``wall`` rounded to it: a row at +-wall or with a NaN height is in no set), in the order
of STATE_LOSS_COLUMNS:

    drift          sum (dy - u0 / drift)^2 / F                         (:852; the division in the dtype)
    wall_low       sum_LOW sum_c (u - 1)^2 / (|LOW| c), 0 when empty   (:855-857)
    wall_high      sum_HIGH sum_c (u + 1)^2 / (|HIGH| c), 0 when empty (:859-861)
    dmeans_x       sum dx^2 / F                                        (:867)
    dmeans_spread  sum [(dx - mean dx)^2 + (dy - mean dy)^2] / (2 F)   (:868-869)
    height_spread  sum (y - mean y)^2 / F                              (:870-871)
    unit_u         sum_MID (|u0| - 1)^2 / |MID|, 0 when empty          (:875)
    du_mid         sum_MID sum_c du^2 / (|MID| c), 0 when empty        (:876)

With no free row the entries 0, 3, 4, 5 are NaN (``torch.mean`` of nothing) and the conditional ones 0.  Boundary rows are
branched around: NaN or Inf there reaches neither a term nor a gradient.  ``Model.compute_loss`` for TEST is then

    pde_loss = terms[0]        bc_loss = terms[1] + terms[2]
    conservation_loss = dmean_weight (terms[3] + terms[4] + terms[5]) + du_weight (terms[6] + terms[7])
                      + dscale_weight penalty[1] + dtransform_weight penalty[2]        (advance_gaussians' penalty)

Gradients leave towards means, u and deltas (ONE tensor in the caller's shape); the membership sets, their counts and the
means inside the centred sums are constants of the backward.  d = 2, c = 1..4, float32 / float64, contiguous GPU tensors,
N >= 1; no CPU fallback.  Nothing is read back; capturable into a hipGraph.
"""
import math

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream
from .advance import DELTA_COLUMNS

STATE_LOSS_COLUMNS = ("drift", "wall_low", "wall_high", "dmeans_x", "dmeans_spread", "height_spread", "unit_u", "du_mid")


def _check(means, u, deltas, boundary_mask, wall, drift):
    """the refusals, with the exception types of advance._check; returns (wall, drift) as floats"""
    wall, drift = float(wall), float(drift)
    if not (wall >= 0.0 and math.isfinite(wall)):
        raise ValueError(f"wall = {wall}: needs a finite wall >= 0")
    if not (drift != 0.0 and math.isfinite(drift)):
        raise ValueError(f"drift = {drift}: needs a finite drift other than 0")
    names = ("means", "u", "deltas", "boundary_mask")
    arrays = (means, u, deltas, boundary_mask)
    for n, a in zip(names, arrays):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor")
    if means.dim() != 2 or means.shape[1] != 2:
        raise NotImplementedError(f"means must be [N, 2] (d = 2), got {tuple(means.shape)}")
    N = means.shape[0]
    if N < 1:
        raise ValueError("no Gaussians: N must be at least 1")
    if u.dim() != 2 or not 1 <= u.shape[1] <= 4:
        raise NotImplementedError(f"u must be [N, c] with c = 1..4, got {tuple(u.shape)}")
    if u.shape[0] != N:
        raise ValueError(f"u holds {u.shape[0]} rows, means {N}")
    width = DELTA_COLUMNS + u.shape[1]
    if tuple(deltas.shape) not in ((N, width), (1, N, width)):
        raise ValueError(f"deltas must be [N, 5 + c] = [{N}, {width}] (a leading 1 allowed), got {tuple(deltas.shape)}")
    if tuple(boundary_mask.shape) not in ((N,), (N, 1)):
        raise ValueError(f"boundary_mask must be [N] or [N, 1] with N = {N}, got {tuple(boundary_mask.shape)}")
    floats = arrays[:3]
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
                               + ": the terms are computed on one GPU (no CPU fallback)")
    return wall, drift


class _StateLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, u, deltas, mask, wall, drift):
        lib = _lib.load()
        N, c = u.shape
        dtype, device = means.dtype, means.device
        terms = torch.empty(len(STATE_LOSS_COLUMNS), dtype=dtype, device=device)
        nbytes = lib.pigs_state_loss_scratch_bytes(N)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            rc = lib.pigs_state_loss_forward(_DTYPES[dtype], c, N, wall, drift, _ptr(means), _ptr(u), _ptr(deltas),
                                             _ptr(mask), _ptr(scratch), nbytes, _ptr(terms), _stream(device))
        _lib.check(rc, "pigs_state_loss_forward")
        ctx.save_for_backward(means, u, deltas, mask, scratch)
        ctx.constants = (wall, drift)
        ctx.set_materialize_grads(False)
        return terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        means, u, deltas, mask, scratch = ctx.saved_tensors
        needs = ctx.needs_input_grad[:3]
        if g is None or not any(needs):
            return (None,) * 6
        lib = _lib.load()
        N, c = u.shape
        wall, drift = ctx.constants
        g = g.contiguous()
        grads = [torch.empty_like(t) if need else None for t, need in zip((means, u, deltas), needs)]
        with torch.cuda.device(means.device):
            rc = lib.pigs_state_loss_backward(_DTYPES[means.dtype], c, N, wall, drift, _ptr(means), _ptr(u), _ptr(deltas),
                                              _ptr(mask), _ptr(scratch), _ptr(g), *[_ptr(t) for t in grads],
                                              _stream(means.device))
        _lib.check(rc, "pigs_state_loss_backward")
        return (*grads, None, None, None)


def state_loss_terms(means, u, deltas, boundary_mask, wall=0.8, drift=5.0):
    """The eight unweighted state terms of Problem.TEST's loss, [8] on the device; see the module text."""
    wall, drift = _check(means, u, deltas, boundary_mask, wall, drift)
    packed = deltas.reshape(deltas.shape[-2], deltas.shape[-1])      # a view: the gradient keeps the caller's shape
    mask = boundary_mask.reshape(-1).view(torch.uint8)
    return _StateLoss.apply(means, u, packed, mask, wall, drift)
