"""``preprocess_aggregate`` / ``aggregate_neighbors`` of the reference's sampler surface (SURVEY.md 8f-2;
call sites /root/reference/model_pn.py:257-264, test_neighbor_aggregation.py:75-98), on the HIP
library (pigs_amd/csrc/aggregate.hip behind pigs_aggregate_* of include/pigs_amd.h).

PARITY UNPINNED.  The arithmetic of these two methods exists only in the reference's absent CUDA
source; the call sites fix the signature, the shapes (features [N,L], transform [L,L], queries / keys
[N,K], frequencies [F], distance_transform [L,2E] with E = 2 d F + 1 -> [N,L]), the dtype (float64 in
the reference's gradcheck) and that the result is differentiable wrt all six arguments -- nothing
else.  The definition is this repository's own (DESIGN.md "aggregate_neighbors"; the checker is
oracle/aggregate_torch.py):

* neighbours of Gaussian i = the Gaussians j whose q <= q_max ellipse reaches the centre of i;
* weight a_ij = softmax over the neighbours j of <queries_i, keys_j> / sqrt(K);
* message m_ij = transform @ features_j + distance_transform @ [e_ij ; g_ij e_ij], with e_ij the
  Fourier embedding of mu_j - mu_i and g_ij = exp(-q_ij / 2) the density of Gaussian j at the centre of i;
* out_i = sum_j a_ij m_ij.

The neighbour relation lives in index lists (``NeighborLists``: [N, cap] with cap = the longest list,
found by a counting pass).  Forward = one launch, backward = four (the three small GEMMs
gout @ [transform | distance_transform], gout^T @ acc included).  d = 2, float32 / float64.

Periodic lists (``NeighborLists(..., periodic=(lo, period))``; ``GaussianSampler(periodic=...,
periodic_aggregate=True)``): the same definition on the torus [lo, lo + period)^2 -- the neighbours of i are the
pairs (j, k), image k of Gaussian j, each with its own offset mu'_j + s_k L - mu'_i, density and softmax entry;
equivalently the definition above on the 9N images of pigs_periodic_images, rows of block 0.  ``means`` must already
be wrapped into the box (block 0 of the image arrays).  One j can appear through several images, so a list can be
longer than N and ``cap`` always comes from the counting pass unless given.
"""
import ctypes

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream

BRUTE_MAX = 2048     # pigs_amd/csrc/aggregate.hip AGG_BRUTE_MAX: up to here every pair is tested, cap = N
LDS_MAX = 163840     # PIGS_AGGREGATE_LDS_MAX of include/pigs_amd.h: the LDS of a CU
MAX_NEIGHBORS = {torch.float32: 8192, torch.float64: 4096}      # slab size when the counting pass cannot be read back (capture)


class NeighborLists:
    """Index lists of the neighbour relation: by rows (the j of an i) and by columns (the i of a j),
    ``cap`` int32 slots per Gaussian.  Up to N = 2048 (the model's sizes) every pair is tested and cap = N:
    two launches, nothing read back.  Beyond: built through the sampler's multi-level Gaussian grid (one wave per
    Gaussian walks the cells around its centre / its ellipse; pigs_amd/csrc/aggregate.hip), in two passes:
    a counting pass, then -- with ``cap`` = the longest list rounded up to 64, read back ONCE (the only
    host synchronisation of ``preprocess_aggregate``) -- the lists themselves.  ``cap`` given (or a hipGraph
    being captured, where nothing may be read back): one pass into slabs of that size, and a list that does
    not fit sets ``overflow`` (checked by :meth:`check`; debug mode calls it).

    ``periodic=(lo, period)``: the lists of the torus (module docstring; entries j | k << 28, read by the periodic
    sampling entries only).  ``means`` are the wrapped centres.  A row can be longer than N, so cap = N is not safe:
    the counting pass runs at every N unless ``cap`` is given or a capture is running (slab ``min(4N,
    MAX_NEIGHBORS)`` then)."""

    def __init__(self, means, conics, q_max, cap=None, periodic=None):
        lib = _lib.load()
        self.periodic = None if periodic is None else (float(periodic[0]), float(periodic[1]))
        self.period = 0.0 if self.periodic is None else self.periodic[1]
        if means.dim() != 2 or means.shape[1] != 2:
            raise NotImplementedError("aggregate_neighbors is implemented for d = 2")
        if means.dtype not in _DTYPES:
            raise TypeError(f"dtype {means.dtype} is not supported (float32 / float64)")
        self.means = means.detach().contiguous()
        self.conics = conics.detach().reshape(means.shape[0], 3).contiguous()
        self.N = N = means.shape[0]
        dev = means.device
        dt = _DTYPES[means.dtype]
        nbytes = lib.pigs_aggregate_workspace_bytes(dt, N)
        if nbytes == 0:
            raise _lib.PigsError(f"aggregate_neighbors does not support N={N}")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.row_counts = torch.empty(N, dtype=torch.int32, device=dev)
        self.col_counts = torch.empty(N, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.row_lists = self.col_lists = None

        def run(flags, cap_, with_lists):
            tail = (_ptr(self.workspace), nbytes, flags, _ptr(self.row_counts),
                    _ptr(self.row_lists) if with_lists else ctypes.c_void_p(0), _ptr(self.col_counts),
                    _ptr(self.col_lists) if with_lists else ctypes.c_void_p(0), _ptr(self.overflow), _stream(dev))
            with torch.cuda.device(dev):
                if self.periodic is None:
                    rc = lib.pigs_aggregate_lists(dt, N, cap_, _ptr(self.means), _ptr(self.conics), float(q_max), *tail)
                else:
                    rc = lib.pigs_aggregate_lists_periodic(dt, N, cap_, _ptr(self.means), _ptr(self.conics), float(q_max),
                                                           self.periodic[0], self.periodic[1], *tail)
            _lib.check(rc, "pigs_aggregate_lists_periodic" if self.periodic else "pigs_aggregate_lists")

        flags = 1                                                  # PIGS_AGGREGATE_BUILD_GRID
        if cap is None and N <= BRUTE_MAX and self.periodic is None:
            cap = max(1, N)                                        # every pair is tested; a slab of N cannot overflow
        if cap is None and N > 0 and torch.cuda.is_current_stream_capturing():
            # nothing can be read back inside a capture (periodic: a j can come through several images)
            cap = min(N if self.periodic is None else 4 * N, MAX_NEIGHBORS[means.dtype])
        if cap is None and N > 0:
            run(flags, 1, False)                                   # counting pass (full lengths)
            flags = 0
            longest = int(torch.maximum(self.row_counts.max(), self.col_counts.max()).item())
            cap = max(64, (longest + 63) // 64 * 64)
        self.cap = max(1, int(cap if cap is not None else 1))
        self.row_lists = torch.empty((N, self.cap), dtype=torch.int32, device=dev)
        self.col_lists = torch.empty((N, self.cap), dtype=torch.int32, device=dev)
        if N > 0:
            run(flags, self.cap, True)

    def check(self):
        """Synchronising check (debug mode): a neighbour list longer than its slab was truncated."""
        if int(self.overflow.item()):
            raise _lib.PigsError(f"aggregate: a Gaussian has more than {self.cap} neighbours (list truncated)")


class _Aggregate(torch.autograd.Function):
    """One launch path for both calls: `heads` says whether the caller's tensors carry a head axis (transforms [H, L, L],
    queries / keys [N, H, K], distance_transforms [H, L, 2E] -> [N, H, L]) or are one head's ([L, L], [N, K], [L, 2E]
    -> [N, L]: the same memory as H = 1)."""

    @staticmethod
    def forward(ctx, nb, heads, features, transforms, queries, keys, frequencies, distance_transforms):
        lib = _lib.load()
        N, L = features.shape
        H, K, F = queries.shape[1] if heads else 1, queries.shape[-1], frequencies.shape[0]
        E = 4 * F + 1
        dt = nb.means.dtype
        ins = (features, transforms, queries, keys, frequencies, distance_transforms)
        f, tr, q, k, fr, dist = (a.detach().to(dt).contiguous() for a in ins)
        lead = (N, H) if heads else (N,)
        out = torch.empty(lead + (L,), dtype=dt, device=f.device)
        lse = torch.empty(lead, dtype=dt, device=f.device)
        acc = torch.empty(lead + (L + 2 * E,), dtype=dt, device=f.device)
        with torch.cuda.device(f.device):
            rc = lib.pigs_aggregate_heads_forward(
                _DTYPES[dt], N, nb.cap, H, L, K, F, nb.period, _ptr(nb.means), _ptr(nb.conics), _ptr(nb.row_counts),
                _ptr(nb.row_lists), _ptr(f), _ptr(tr), _ptr(q), _ptr(k), _ptr(fr), _ptr(dist), _ptr(out), _ptr(lse), _ptr(acc),
                _stream(f.device))
        _lib.check(rc, "pigs_aggregate_heads_forward")
        ctx.nb = nb
        ctx.save_for_backward(f, tr, q, k, fr, dist, lse, acc)
        ctx.dims = (N, H, L, K, F)
        ctx.in_dtypes = tuple(a.dtype for a in ins)
        return out.to(features.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        lib = _lib.load()
        nb = ctx.nb
        f, tr, q, k, fr, dist, lse, acc = ctx.saved_tensors
        N, H, L, K, F = ctx.dims
        dt = f.dtype
        gout = gout.to(dt).contiguous()
        g_f, g_tr, g_q, g_k, g_fr, g_dist = (torch.empty_like(t) for t in (f, tr, q, k, fr, dist))
        nbytes = lib.pigs_aggregate_heads_backward_scratch_bytes(_DTYPES[dt], N, H, L, F)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
        with torch.cuda.device(f.device):
            rc = lib.pigs_aggregate_heads_backward(
                _DTYPES[dt], N, nb.cap, H, L, K, F, nb.period, _ptr(nb.means), _ptr(nb.conics), _ptr(nb.row_counts),
                _ptr(nb.row_lists), _ptr(nb.col_counts), _ptr(nb.col_lists), _ptr(f), _ptr(tr), _ptr(q), _ptr(k), _ptr(fr),
                _ptr(dist), _ptr(lse), _ptr(acc), _ptr(gout), _ptr(scratch), nbytes, _ptr(g_f), _ptr(g_tr), _ptr(g_q), _ptr(g_k),
                _ptr(g_fr), _ptr(g_dist), _stream(f.device))
        _lib.check(rc, "pigs_aggregate_heads_backward")
        if N == 0:
            for g in (g_tr, g_fr, g_dist):
                g.zero_()
        grads = (g_f, g_tr, g_q, g_k, g_fr, g_dist)
        return (None, None) + tuple(g.to(d) for g, d in zip(grads, ctx.in_dtypes))


def _refuse_one_head(dt, L, K, F):
    """The size checks of one head, in aggregate()'s words."""
    E = 4 * F + 1
    if L + 2 * E > 128:
        raise NotImplementedError(f"L + 2E = {L + 2 * E} > 128 is not supported")
    lds = _lib.load().pigs_aggregate_lds_bytes(_DTYPES[dt], L, K, F)
    if lds > LDS_MAX:      # the backward's kernels included: a forward that cannot be differentiated is refused
        raise NotImplementedError(f"{str(dt).replace('torch.', '')} with L = {L}, K = {K}, F = {F} needs {lds} bytes of LDS "
                                  f"in one of the forward's or the backward's kernels; the limit is {LDS_MAX}")


def aggregate(nb, features, transform, queries, keys, frequencies, distance_transform):
    N = nb.N
    if features.dim() != 2 or features.shape[0] != N:
        raise ValueError(f"features must be [N={N}, L], got {tuple(features.shape)}")
    L, K, F = features.shape[1], queries.shape[1], frequencies.shape[0]
    E = 4 * F + 1
    if (transform.shape != (L, L) or queries.shape != (N, K) or keys.shape != (N, K)
            or distance_transform.shape != (L, 2 * E)):
        raise ValueError(f"aggregate_neighbors: expected transform [{L},{L}], queries/keys [{N},{K}], "
                         f"distance_transform [{L},{2 * E}] (E = 2*d*F + 1 = {E})")
    for name, t in (("features", features), ("transform", transform), ("queries", queries), ("keys", keys),
                    ("frequencies", frequencies), ("distance_transform", distance_transform)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: aggregate_neighbors runs on the GPU only (no CPU fallback)")
    _refuse_one_head(nb.means.dtype, L, K, F)
    return _Aggregate.apply(nb, False, features, transform, queries, keys, frequencies, distance_transform)


# ---- all heads of a layer in one launch ----------------------------------------------------------------------------
MAX_HEADS = 4        # PIGS_AGGREGATE_HEADS_MAX of include/pigs_amd.h


def heads_refusal(dtype, H, L, K, F):
    """None when the kernels admit the shape, else the reason.  The rule is the library's
    (pigs_aggregate_heads_lds_bytes: 0 = more than 128 components in one kernel, else the LDS the kernels ask for)."""
    lds = _lib.load().pigs_aggregate_heads_lds_bytes(_DTYPES[dtype], H, L, K, F)
    shape = f"{str(dtype).replace('torch.', '')} with H = {H}, L = {L}, K = {K}, F = {F}"
    if lds == 0:
        return f"{shape} has more than 128 components in one kernel (L + 2E, H K + F, H (L + K) <= 128)"
    if lds > LDS_MAX:
        return f"{shape} needs {lds} bytes of LDS in one of the forward's or the backward's kernels; the limit is {LDS_MAX}"
    return None


def aggregate_heads(nb, features, transforms, queries, keys, frequencies, distance_transforms):
    """out[:, h] = aggregate(nb, features, transforms[h], queries[:, h], keys[:, h], frequencies, distance_transforms[h])
    for every head h in one forward launch (features, frequencies and the lists are the heads' common part).
    transforms [H, L, L], queries / keys [N, H, K], distance_transforms [H, L, 2E] -> [N, H, L]."""
    N = nb.N
    if features.dim() != 2 or features.shape[0] != N:
        raise ValueError(f"features must be [N={N}, L], got {tuple(features.shape)}")
    if queries.dim() != 3 or frequencies.dim() != 1:
        raise ValueError(f"aggregate_neighbors_heads: queries must be [N={N}, H, K] and frequencies [F], got "
                         f"{tuple(queries.shape)} and {tuple(frequencies.shape)}")
    L, H, K, F = features.shape[1], queries.shape[1], queries.shape[2], frequencies.shape[0]
    E = 4 * F + 1
    if (transforms.shape != (H, L, L) or queries.shape != (N, H, K) or keys.shape != (N, H, K)
            or distance_transforms.shape != (H, L, 2 * E)):
        raise ValueError(f"aggregate_neighbors_heads: expected transforms [{H},{L},{L}], queries/keys [{N},{H},{K}], "
                         f"distance_transforms [{H},{L},{2 * E}] (E = 2*d*F + 1 = {E})")
    ins = (("features", features), ("transforms", transforms), ("queries", queries), ("keys", keys),
           ("frequencies", frequencies), ("distance_transforms", distance_transforms))
    for name, t in ins:
        if not t.is_cuda:
            raise RuntimeError(f"{name} is on {t.device}: aggregate_neighbors_heads runs on the GPU only (no CPU fallback)")
    if H < 1 or H > MAX_HEADS:
        raise NotImplementedError(f"H = {H} heads: one launch serves 1 <= H <= {MAX_HEADS}; H separate aggregate_neighbors "
                                  f"calls remain available")
    if H == 1:       # one head: aggregate()'s rule, in its words
        _refuse_one_head(nb.means.dtype, L, K, F)
    else:
        why = heads_refusal(nb.means.dtype, H, L, K, F)
        if why is not None:
            raise NotImplementedError(f"aggregate_neighbors_heads: {why}; H separate aggregate_neighbors calls remain available")
    return _Aggregate.apply(nb, True, features, transforms, queries, keys, frequencies, distance_transforms)
