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
"""
import ctypes

import torch

from . import _lib
from ._lib import pointers as _pointers, ptr as _ptr, stream as _stream

MAX_LAYERS = 6
MAX_WIDTH = 48
MAX_NETS = 8


def _check(x, weights, biases):
    """the refusals, with the exception types of advance._check; returns the widths"""
    weights, biases = tuple(weights), tuple(biases)
    if not isinstance(x, torch.Tensor):
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
    if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[0] != 1):
        raise ValueError(f"x must be [N, w] or [1, N, w], got {tuple(x.shape)}")
    N, widths = x.shape[-2], [x.shape[-1]]
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
    arrays = [("x", x)] + [(f"weights[{l}]", weights[l]) for l in range(L)] + [(f"biases[{l}]", biases[l]) for l in range(L)]
    if any(a.dtype != torch.float32 for _, a in arrays):
        raise TypeError(f"dtypes {sorted({str(a.dtype) for _, a in arrays})}: float32 only")
    for n, a in arrays:
        if not a.is_contiguous():
            raise ValueError(f"{n} must be contiguous")
    for n, a in arrays:
        if not a.is_cuda or a.device != x.device:
            raise RuntimeError(f"{n} is on {a.device}" + (f", x on {x.device}" if a is not x else "")
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
