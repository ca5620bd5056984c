"""grid_lookup: the pixel of an image under every sample point, in one HIP launch (C ABI: pigs_grid_lookup).

The reference makes the data of its vorticity fits -- the ``recon_loss`` of the Navier-Stokes loop (main_pn.py:202-212) and
the whole loss of the fit that produces its initial conditions (test_initialize.py:131-136) -- with

    coords = ((samples + 1.0) / 2.0 * res).to(torch.long).clamp(0, res - 1)
    coords = coords[:, 1] * res + coords[:, 0]
    data = torch.take(desired, coords)

nine small launches a step.  Here

    data = grid_lookup(image, samples, box=(-1.0, 1.0))        # [M], the image's dtype

with, each operation rounded once in the samples' dtype, a true division and no contraction into an FMA,

    tx = (x - lo) / (hi - lo) * W ;  ix = clamp(trunc(tx), 0, W - 1)        # ty, iy with H likewise
    data[m] = image[iy][ix]

A non-finite coordinate reads pixel 0 of its axis.  With ``box=(-1, 1)`` and a square image these are the reference's
lines bit for bit (``x - (-1)`` is ``x + 1``, the division by 2 is exact); ``box`` is the ``scale`` that main_pn.py:206
leaves out.  ``image`` [H, W] and ``samples`` [M, 2]: float32 or float64 (each its own), contiguous, on one GPU.  No
gradient; nothing is read back, and only the output is allocated, through torch: capturable into a hipGraph.  The result
goes straight into ``GaussianSampler.vorticity_residual(..., data=data)``.
"""
import math

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream


def grid_lookup(image, samples, box=(-1.0, 1.0)):
    """``image[iy, ix]`` of the pixel under every row of ``samples``, [M] in the image's dtype; see the module text."""
    for n, a in (("image", image), ("samples", samples)):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor")
    if image.dim() != 2 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"image must be [H, W] with at least one pixel, got {tuple(image.shape)}")
    if samples.dim() != 2 or samples.shape[1] != 2:
        raise ValueError(f"samples must be [M, 2], got {tuple(samples.shape)}")
    lo, hi = (float(v) for v in box)
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"box = ({lo}, {hi}): needs finite lo < hi")
    if image.dtype not in _DTYPES or samples.dtype not in _DTYPES:
        raise TypeError(f"dtypes {image.dtype}, {samples.dtype}: float32 or float64")
    for n, a in (("image", image), ("samples", samples)):
        if not a.is_cuda or a.device != image.device:
            raise RuntimeError(f"{n} is on {a.device}" + (f", image on {image.device}" if a is not image else "")
                               + ": the lookup runs on one GPU (no CPU fallback)")
    image, samples = image.detach().contiguous(), samples.detach().contiguous()
    H, W = image.shape
    M = samples.shape[0]
    lib = _lib.load()
    out = torch.empty(M, dtype=image.dtype, device=image.device)
    with torch.cuda.device(image.device):
        rc = lib.pigs_grid_lookup(_DTYPES[image.dtype], _DTYPES[samples.dtype], H, W, M, lo, hi, _ptr(image), _ptr(samples),
                                  _ptr(out), _stream(image.device))
    _lib.check(rc, "pigs_grid_lookup")
    return out
