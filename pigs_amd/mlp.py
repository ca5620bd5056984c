"""fused_mlp: one per-Gaussian tanh network in ONE HIP launch forward and at most two backward.

The dynamics network (model_pn.Model) applies three kinds of small nets row by row to its [1, N, width] features:
``input_projection`` (model_pn.py:187-198), the ``query_transform`` / ``key_transform`` nets (:203-226) and ``delta_net``
(:154-174), each an ``nn.Sequential`` of ``nn.Linear`` with ``nn.Tanh`` (:425-426) between them and none after the last.
In torch every layer is a GEMM launch, a bias / activation launch and their backward launches.  Here (C ABI:
pigs_mlp_forward / pigs_mlp_backward):

    y = fused_mlp(x, weights, biases)

``x`` is [N, w_0] or [1, N, w_0]; ``weights[l]`` is [w_{l+1}, w_l] and ``biases[l]`` [w_{l+1}], nn.Linear's own layout;
``y`` has the leading shape of ``x`` and w_L columns:

    a_0 = x;   a_{l+1} = tanh(a_l W_l^T + b_l) for l < L - 1;   y = a_{L-1} W_{L-1}^T + b_{L-1}

1 <= L <= 6, every width (input and output included) in 1..48, float32, contiguous GPU tensors, N >= 1; no CPU fallback.
The backward recomputes the activations from ``x`` (nothing else is saved, so the forward is the same launch with and
without autograd), gives the gradients that ``needs_input_grad`` asks for, and is once-differentiable.  No float atomics:
the same inputs give the same bits on every call.  Capturable into a hipGraph (pigs_amd.graphs.GraphedStep).

    net = FusedMLP.from_sequential(seq)      # an nn.Sequential of the same children (the same Parameters and
                                             # state_dict keys) whose forward is the launch above

A bank: B nets of ONE shape over ONE input, in one launch forward and at most two backward (C ABI: pigs_mlp_bank_forward
/ pigs_mlp_bank_backward; 1 <= B <= 8).  The model's four query_transform / key_transform nets (:259-261) are one:

    qk = fused_mlp_bank(x, weights, biases, groups=2)     # weights[b][l], biases[b][l]; nets (q0, q1, k0, k1)

``qk`` is [G, N, B / G, w_L] with ``qk[b // (B / G), :, b % (B / G)] = fused_mlp(x, weights[b], biases[b])``, bit for
bit: ``qk[0]`` and ``qk[1]`` are the contiguous ``queries`` / ``keys`` [N, H, K] of aggregate_neighbors_heads.  The
gradient of ``x`` is the nets' gradients added in the order of the nets.

    bank = FusedMLPBank([*query_transform, *key_transform], groups=2)      # non-owning: registers no parameter

A row that lies in several arrays (C ABI: pigs_mlp_joined_forward / pigs_mlp_joined_backward): delta_net reads the features
and the heads' neighbour features side by side (:265-268, a cat), and magnitude_loss (:892-901) is the mean square of each
head's block of that row.  Without the cat, its backward's split, or any reduction launch:

    deltas, mags = delta_net.joined((features, nf), block_means=(0, H))      # FusedMLP.joined -> fused_mlp_joined
    magnitude_loss = ((mags - 1) ** 2).mean()
"""
import ctypes

import torch

from . import _lib
from ._lib import pointers as _pointers, ptr as _ptr, stream as _stream

MAX_LAYERS = 6
MAX_WIDTH = 48
MAX_NETS = 8
MAX_PARTS = 4
MAX_BLOCKS = 8


def _check(x, weights, biases, joined=None):
    """the refusals, with the exception types of advance._check; returns the widths.  ``joined``: (N, w_0, [(name,
    part)]) when the row lies in several arrays (``_check_joined``, which has looked at their shapes; ``x`` is None)"""
    weights, biases = tuple(weights), tuple(biases)
    if joined is None and not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    L = len(weights)
    if len(biases) != L:
        raise ValueError(f"{L} weights and {len(biases)} biases")
    if not 1 <= L <= MAX_LAYERS:
        raise NotImplementedError(f"{L} layers: 1..{MAX_LAYERS} per call")
    for l in range(L):
        for n, a in ((f"weights[{l}]", weights[l]), (f"biases[{l}]", biases[l])):
            if not isinstance(a, torch.Tensor):
                raise TypeError(f"{n} must be a torch.Tensor" + (" (a net without biases is not built)" if a is None else ""))
    if joined is not None:
        N, widths, inputs = joined[0], [joined[1]], list(joined[2])
    elif x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[0] != 1):
        raise ValueError(f"x must be [N, w] or [1, N, w], got {tuple(x.shape)}")
    else:
        N, widths, inputs = x.shape[-2], [x.shape[-1]], [("x", x)]
    if N < 1:
        raise ValueError("no rows: N must be at least 1")
    for l in range(L):
        if weights[l].dim() != 2 or weights[l].shape[1] != widths[-1]:
            raise ValueError(f"weights[{l}] must be [w_{l + 1}, {widths[-1]}], got {tuple(weights[l].shape)}")
        widths.append(weights[l].shape[0])
        if tuple(biases[l].shape) != (widths[-1],):
            raise ValueError(f"biases[{l}] must be [{widths[-1]}], got {tuple(biases[l].shape)}")
    for l, w in enumerate(widths):
        if not 1 <= w <= MAX_WIDTH:
            raise NotImplementedError(f"width {w} (w_{l}): every width must be in 1..{MAX_WIDTH}")
    arrays = inputs + [(f"weights[{l}]", weights[l]) for l in range(L)] + [(f"biases[{l}]", biases[l]) for l in range(L)]
    if any(a.dtype != torch.float32 for _, a in arrays):
        raise TypeError(f"dtypes {sorted({str(a.dtype) for _, a in arrays})}: float32 only")
    for n, a in arrays:
        if not a.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    first, x = arrays[0]
    for n, a in arrays:
        if not a.is_cuda or a.device != x.device:
            raise RuntimeError(f"{n} is on {a.device}" + (f", {first} on {x.device}" if a is not x else "")
                               + ": the network runs on one GPU (no CPU fallback)")
    return widths


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, *params):
        lib = _lib.load()
        L = len(params) // 2
        weights, biases = params[:L], params[L:]
        N = x.shape[0]
        widths = [x.shape[1]] + [w.shape[0] for w in weights]
        y = torch.empty((N, widths[-1]), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib.pigs_mlp_forward(_lib.PIGS_F32, N, L, (ctypes.c_int * (L + 1))(*widths), _ptr(x), _pointers(weights),
                                      _pointers(biases), _ptr(y), _stream(x.device))
        _lib.check(rc, "pigs_mlp_forward")
        ctx.save_for_backward(x, *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        x, *params = ctx.saved_tensors
        needs = ctx.needs_input_grad
        if not any(needs):
            return (None,) * len(needs)
        lib = _lib.load()
        L = len(params) // 2
        weights, biases = params[:L], params[L:]
        N = x.shape[0]
        g_y = g_y.contiguous()
        widths = (ctypes.c_int * (L + 1))(x.shape[1], *[w.shape[0] for w in weights])
        grads = [torch.empty_like(t) if need else None for t, need in zip((x, *params), needs)]
        nbytes = lib.pigs_mlp_scratch_bytes(N, L, widths) if any(needs[1:]) else 0
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
        with torch.cuda.device(x.device):
            rc = lib.pigs_mlp_backward(_lib.PIGS_F32, N, L, widths, _ptr(x), _pointers(weights), _pointers(biases),
                                       _ptr(g_y), _ptr(scratch), nbytes, _ptr(grads[0]),
                                       _pointers(grads[1:1 + L]), _pointers(grads[1 + L:]), _stream(x.device))
        _lib.check(rc, "pigs_mlp_backward")
        return tuple(grads)


def fused_mlp(x, weights, biases):
    """The net of ``weights`` / ``biases`` applied to every row of ``x``; see the module text."""
    weights, biases = tuple(weights), tuple(biases)
    _check(x, weights, biases)
    rows = x.reshape(x.shape[-2], x.shape[-1])          # a view: the gradient keeps the caller's shape
    y = _FusedMLP.apply(rows, *weights, *biases)
    return y.reshape(*x.shape[:-1], y.shape[-1])


class FusedMLP(torch.nn.Sequential):
    """``fused_mlp`` as a module over an existing ``nn.Sequential`` of alternating ``nn.Linear`` / ``nn.Tanh``.  It is an
    ``nn.Sequential`` of the SAME child modules under the same names ("0", "1", ...), so the Parameters are the same
    objects under the same ``state_dict`` keys: optimisers and checkpoints of the wrapped net stay valid.  Only
    ``forward`` differs."""

    def __init__(self, seq):
        linears = self._linears_of(seq)
        super().__init__(*list(seq))
        self._linears = tuple(range(0, 2 * len(linears), 2))      # the children that are nn.Linear

    @staticmethod
    def _linears_of(seq):
        if not isinstance(seq, torch.nn.Sequential):
            raise TypeError(f"from_sequential takes an nn.Sequential, got {type(seq).__name__}")
        mods = list(seq)
        if not mods:
            raise NotImplementedError("an empty nn.Sequential")
        linears = []
        for k, m in enumerate(mods):
            if k % 2 == 0:
                if not isinstance(m, torch.nn.Linear):
                    raise NotImplementedError(f"module {k} is {type(m).__name__}: nn.Linear expected "
                                              "(alternating nn.Linear / nn.Tanh, ending with nn.Linear)")
                if m.bias is None:
                    raise NotImplementedError(f"module {k} is nn.Linear with bias=False: not built")
                for w in (m.in_features, m.out_features):
                    if not 1 <= w <= MAX_WIDTH:
                        raise NotImplementedError(f"module {k} is nn.Linear({m.in_features}, {m.out_features}): width {w} "
                                                  f"is outside 1..{MAX_WIDTH}")
                linears.append(m)
            elif not isinstance(m, torch.nn.Tanh):
                raise NotImplementedError(f"module {k} is {type(m).__name__}: nn.Tanh is the only activation built")
        if len(mods) % 2 == 0:
            raise NotImplementedError(f"the nn.Sequential ends with {type(mods[-1]).__name__}: no activation after the "
                                      "last nn.Linear is built")
        if len(linears) > MAX_LAYERS:
            raise NotImplementedError(f"{len(linears)} nn.Linear layers: at most {MAX_LAYERS} per launch")
        return linears

    @classmethod
    def from_sequential(cls, seq):
        return cls(seq)

    def forward(self, x):
        linears = [self[k] for k in self._linears]
        return fused_mlp(x, [m.weight for m in linears], [m.bias for m in linears])

    def joined(self, parts, block_means=None):
        """``fused_mlp_joined`` with this net's ``nn.Linear`` children as they are now (read at every call, as ``forward``
        does): the net on a row that lies in several arrays, and optionally the block means of its squares."""
        linears = [self[k] for k in self._linears]
        return fused_mlp_joined(parts, [m.weight for m in linears], [m.bias for m in linears], block_means)


def _check_joined(parts, weights, biases, block_means):
    """the joined call's refusals, with ``_check``'s exception types, naming the part: the parts among themselves first,
    then ``_check`` with the parts in the place of x.  Returns N, where each part's rows begin (1 for [1, N, ...]), the
    parts' widths and the blocks (a tuple of P ints, or None for none)."""
    parts = tuple(parts)
    P = len(parts)
    if not 1 <= P <= MAX_PARTS:
        raise NotImplementedError(f"{P} parts: 1..{MAX_PARTS} per call")
    for p, t in enumerate(parts):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"parts[{p}] must be a torch.Tensor")
        if t.dim() < 2:
            raise ValueError(f"parts[{p}] must be [N, ...] or [1, N, ...] with at least one column, got {tuple(t.shape)}")
    # [1, n, ...] reads as one row or as n rows behind a leading 1: a part that reads one way only says which N it is
    sure = [t.shape[0] for t in parts if t.shape[0] != 1 or t.dim() == 2]
    N = sure[0] if sure else parts[0].shape[1]
    leads, part_widths = [], []
    for p, t in enumerate(parts):
        lead = 1 if t.dim() >= 3 and t.shape[0] == 1 and t.shape[1] == N else 0
        if t.shape[lead] != N:
            raise ValueError(f"parts[{p}] {tuple(t.shape)} has {t.shape[lead]} rows, the others {N}")
        w = 1
        for n in t.shape[lead + 1:]:
            w *= n
        if not 1 <= w <= MAX_WIDTH:
            raise NotImplementedError(f"parts[{p}] {tuple(t.shape)} is {w} columns wide: 1..{MAX_WIDTH}")
        if t.dtype != torch.float32:
            raise TypeError(f"parts[{p}] is {t.dtype}: float32 only")
        leads.append(lead)
        part_widths.append(w)
    weights = tuple(weights)
    if weights and isinstance(weights[0], torch.Tensor) and weights[0].dim() == 2 and weights[0].shape[1] != sum(part_widths):
        raise ValueError(f"the parts' widths {part_widths} add up to {sum(part_widths)}, weights[0] is "
                         f"{tuple(weights[0].shape)}")
    blocks = None
    if block_means is not None:
        blocks = tuple(block_means)
        if len(blocks) != P:
            raise ValueError(f"block_means has {len(blocks)} entries for {P} parts")
        for p, b in enumerate(blocks):
            if not isinstance(b, int) or isinstance(b, bool) or b < 0:
                raise ValueError(f"block_means[{p}] = {b!r} must be an int >= 0")
            if b and part_widths[p] % b:
                raise ValueError(f"block_means[{p}] = {b} does not divide parts[{p}]'s {part_widths[p]} columns")
        if sum(blocks) > MAX_BLOCKS:
            raise NotImplementedError(f"{sum(blocks)} blocks: at most {MAX_BLOCKS} per call")
    _check(None, weights, biases, joined=(N, sum(part_widths), [(f"parts[{p}]", t) for p, t in enumerate(parts)]))
    return N, leads, part_widths, blocks


class _FusedMLPJoined(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, blocks, *tensors):
        lib = _lib.load()
        parts, params = tensors[:P], tensors[P:]
        L = len(params) // 2
        weights, biases = params[:L], params[L:]
        x0 = parts[0]
        N = x0.shape[0]
        part_widths = (ctypes.c_int * P)(*[t.shape[1] for t in parts])
        widths = (ctypes.c_int * (L + 1))(sum(part_widths), *[w.shape[0] for w in weights])
        count = sum(blocks) if blocks else 0
        cblocks = (ctypes.c_int * P)(*blocks) if count else None
        y = torch.empty((N, widths[L]), dtype=x0.dtype, device=x0.device)
        m = torch.empty((count,), dtype=x0.dtype, device=x0.device) if count else None
        nbytes = lib.pigs_mlp_joined_scratch_bytes(N, L, widths, P, cblocks, 0) if count else 0
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=x0.device) if nbytes else None
        with torch.cuda.device(x0.device):
            rc = lib.pigs_mlp_joined_forward(_lib.PIGS_F32, N, L, widths, P, part_widths, _pointers(parts), cblocks,
                                             _pointers(weights), _pointers(biases), _ptr(scratch), nbytes, _ptr(y), _ptr(m),
                                             _stream(x0.device))
        _lib.check(rc, "pigs_mlp_joined_forward")
        ctx.save_for_backward(*tensors)
        ctx.joined = (P, L, count, widths, part_widths, cblocks)
        ctx.set_materialize_grads(False)          # an output that is not used arrives as None, and stays a null pointer
        return (y, m) if count else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y, g_m=None):
        tensors = ctx.saved_tensors
        P, L, count, widths, part_widths, cblocks = ctx.joined
        needs = ctx.needs_input_grad[2:]
        if not any(needs) or (g_y is None and g_m is None):
            return (None,) * (2 + len(needs))
        lib = _lib.load()
        parts, weights, biases = tensors[:P], tensors[P:P + L], tensors[P + L:]
        N = parts[0].shape[0]
        g_y = g_y.contiguous() if g_y is not None else None
        g_m = g_m.contiguous() if g_m is not None else None
        grads = [torch.empty_like(t) if need else None for t, need in zip(tensors, needs)]
        nbytes = lib.pigs_mlp_joined_scratch_bytes(N, L, widths, P, cblocks, 1) if any(needs[P:]) else 0
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=parts[0].device) if nbytes else None
        with torch.cuda.device(parts[0].device):
            rc = lib.pigs_mlp_joined_backward(_lib.PIGS_F32, N, L, widths, P, part_widths, _pointers(parts), cblocks,
                                              _pointers(weights), _pointers(biases), _ptr(g_y), _ptr(g_m), _ptr(scratch),
                                              nbytes, _pointers(grads[:P]), _pointers(grads[P:P + L]),
                                              _pointers(grads[P + L:]), _stream(parts[0].device))
        _lib.check(rc, "pigs_mlp_joined_backward")
        return (None, None, *grads)


def fused_mlp_joined(parts, weights, biases, block_means=None):
    """``fused_mlp`` on a row that lies in several arrays, without the cat; optionally the block means of squares.

        y = fused_mlp_joined(parts, weights, biases)
        y, m = fused_mlp_joined(parts, weights, biases, block_means=(b_0, .., b_{P-1}))

    ``parts``: 1..4 contiguous float32 GPU tensors [N, ...] or [1, N, ...] with one N; a part's trailing dimensions are
    its columns (w_p >= 1 of them), so the heads' [N, H, L] goes in as it is.  The parts' widths add up to w_0 <= 48.
    ``y`` is ``fused_mlp(torch.cat(flat parts, -1), weights, biases)`` bit for bit, with the leading shape of part 0.
    ``block_means``: None, or one int per part: 0 takes nothing of that part; b >= 1 must divide w_p and cuts the part's
    columns into b equal blocks; at most 8 blocks in all.  ``m`` is float32 [sum b_p], in the order of the parts:
    ``m[j]`` = the mean over the N rows and the block's w_p / b_p columns of x**2.  Without block means one launch and no
    scratch; with them the same launch and a one-workgroup finish.  The backward is ``fused_mlp``'s launches and gives one
    gradient per part, in the part's own shape, only where asked:

        g_part_p[row, k] = dA_0[row, K_p + k] + g_m[block of k] * 2 x[row, k] / (N w_p / b_p)

    with the parameter gradients bit for bit ``fused_mlp``'s on the cat, and without ``m`` in the loss every g_part the
    bits of its slice of ``fused_mlp``'s g_x.  Once-differentiable, no float atomics, capturable (GraphedStep).  The
    model's call (model_pn.py:265-268, :892-901): ``deltas, mags = delta_net.joined((features, nf), block_means=(0, H))``,
    ``magnitude_loss = ((mags - 1) ** 2).mean()``."""
    parts, weights, biases = tuple(parts), tuple(weights), tuple(biases)
    N, leads, part_widths, blocks = _check_joined(parts, weights, biases, block_means)
    rows = [t.reshape(N, w) for t, w in zip(parts, part_widths)]          # views: a gradient keeps its part's shape
    out = _FusedMLPJoined.apply(len(parts), blocks if blocks and sum(blocks) else None, *rows, *weights, *biases)
    y, m = out if isinstance(out, tuple) else (out, None)
    y = y.reshape(*parts[0].shape[:leads[0] + 1], y.shape[-1])
    if blocks is None:
        return y
    return y, (m if m is not None else y.new_zeros((0,)))


def _check_bank(x, weights, biases, groups):
    """the bank's refusals: every net against net 0's layer count and shapes first (so that the first differing net and
    layer are named), then those of ``_check`` per net"""
    if len(weights) != len(biases):
        raise ValueError(f"{len(weights)} nets of weights and {len(biases)} of biases")
    B = len(weights)
    if not 1 <= B <= MAX_NETS:
        raise NotImplementedError(f"{B} nets: 1..{MAX_NETS} per bank")
    if not isinstance(groups, int) or groups < 1 or B % groups:
        raise ValueError(f"groups = {groups!r} must be a positive integer that divides the {B} nets")
    L = len(weights[0])
    for b in range(B):
        if len(weights[b]) != L or len(biases[b]) != L:
            raise ValueError(f"net {b} has {len(weights[b])} weights and {len(biases[b])} biases, net 0 has {L} weights: "
                             "a bank holds nets of one shape")
        for l in range(L):
            for what, t, t0 in (("weight", weights[b][l], weights[0][l]), ("bias", biases[b][l], biases[0][l])):
                if isinstance(t, torch.Tensor) and isinstance(t0, torch.Tensor) and t.shape != t0.shape:
                    raise ValueError(f"net {b}, layer {l}: {what} {tuple(t.shape)}, net 0 has {tuple(t0.shape)}: a bank "
                                     "holds nets of one shape")
    for b in range(B):
        try:
            _check(x, weights[b], biases[b])
        except (TypeError, ValueError, NotImplementedError, RuntimeError) as e:
            raise type(e)(f"net {b}: {e}") from None


class _FusedMLPBank(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B, G, *params):
        lib = _lib.load()
        L = len(params) // (2 * B)
        weights, biases = params[:B * L], params[B * L:]          # net b's layer l at b * L + l
        N = x.shape[0]
        widths = [x.shape[1]] + [w.shape[0] for w in weights[:L]]
        y = torch.empty((G, N, B // G, widths[-1]), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib.pigs_mlp_bank_forward(_lib.PIGS_F32, N, B, G, L, (ctypes.c_int * (L + 1))(*widths), _ptr(x),
                                           _pointers(weights), _pointers(biases), _ptr(y), _stream(x.device))
        _lib.check(rc, "pigs_mlp_bank_forward")
        ctx.save_for_backward(x, *params)
        ctx.bank = (B, G, L)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        x, *params = ctx.saved_tensors
        B, G, L = ctx.bank
        needs = (ctx.needs_input_grad[0],) + tuple(ctx.needs_input_grad[3:])
        if not any(needs):
            return (None,) * (3 + len(params))
        lib = _lib.load()
        N = x.shape[0]
        g_y = g_y.contiguous()
        widths = (ctypes.c_int * (L + 1))(x.shape[1], *[w.shape[0] for w in params[:L]])
        grads = [torch.empty_like(t) if need else None for t, need in zip((x, *params), needs)]
        nbytes = lib.pigs_mlp_bank_scratch_bytes(N, B, L, widths) if any(needs[1:]) or (needs[0] and B > 1) else 0
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
        with torch.cuda.device(x.device):
            rc = lib.pigs_mlp_bank_backward(_lib.PIGS_F32, N, B, G, L, widths, _ptr(x), _pointers(params[:B * L]),
                                            _pointers(params[B * L:]), _ptr(g_y), _ptr(scratch), nbytes, _ptr(grads[0]),
                                            _pointers(grads[1:1 + B * L]), _pointers(grads[1 + B * L:]), _stream(x.device))
        _lib.check(rc, "pigs_mlp_bank_backward")
        return (grads[0], None, None, *grads[1:])


def fused_mlp_bank(x, weights, biases, groups=1):
    """The B nets ``weights[b]`` / ``biases[b]`` of one shape applied to every row of ``x`` [N, w_0] or [1, N, w_0]:
    [G, N, B / G, w_L], ``G = groups``; see the module text."""
    weights, biases = [tuple(w) for w in weights], [tuple(b) for b in biases]
    _check_bank(x, weights, biases, groups)
    rows = x.reshape(x.shape[-2], x.shape[-1])          # a view: the gradient keeps the caller's shape
    return _FusedMLPBank.apply(rows, len(weights), groups, *[w for net in weights for w in net],
                               *[b for net in biases for b in net])


class FusedMLPBank:
    """``fused_mlp_bank`` over existing nets: ``nn.Sequential``s of alternating ``nn.Linear`` / ``nn.Tanh`` (``FusedMLP``s
    among them) of one shape.  NOT an ``nn.Module`` and non-owning: the nets stay where they are registered (the
    model's ``query_transform`` / ``key_transform``), so that ``parameters()`` and ``state_dict()`` of whatever holds the
    bank keep their keys and order and list no parameter twice.  ``m.weight`` / ``m.bias`` are read at every call: a
    ``load_state_dict`` or an optimiser's step is seen by the next one."""

    def __init__(self, nets, groups=1):
        nets = list(nets)
        if not 1 <= len(nets) <= MAX_NETS:
            raise NotImplementedError(f"{len(nets)} nets: 1..{MAX_NETS} per bank")
        if not isinstance(groups, int) or groups < 1 or len(nets) % groups:
            raise ValueError(f"groups = {groups!r} must be a positive integer that divides the {len(nets)} nets")
        self._linears = []
        for b, net in enumerate(nets):
            try:
                self._linears.append(tuple(FusedMLP._linears_of(net)))
            except (TypeError, NotImplementedError) as e:
                raise type(e)(f"net {b}: {e}") from None
        shape = [(m.in_features, m.out_features) for m in self._linears[0]]
        for b, linears in enumerate(self._linears):
            other = [(m.in_features, m.out_features) for m in linears]
            if len(other) != len(shape):
                raise ValueError(f"net {b} has {len(other)} nn.Linear layers, net 0 has {len(shape)}: a bank holds nets "
                                 "of one shape")
            for l, (a, a0) in enumerate(zip(other, shape)):
                if a != a0:
                    raise ValueError(f"net {b}, layer {l}: nn.Linear{a}, net 0 has nn.Linear{a0}: a bank holds nets of "
                                     "one shape")
        self.groups = groups

    @classmethod
    def from_sequentials(cls, nets, groups=1):
        return cls(nets, groups)

    def arguments(self):
        """(weights, biases) as the next call passes them: the nets' Parameters as they are now"""
        return ([[m.weight for m in net] for net in self._linears], [[m.bias for m in net] for net in self._linears])

    def __call__(self, x):
        weights, biases = self.arguments()
        return fused_mlp_bank(x, weights, biases, self.groups)
