"""The dynamics network's input transform: ``t_params`` in three HIP launches forward and at most five backward.

``InputTransform`` (model_pn.py:51-152) as ``DynamicsNetwork.forward`` uses it (:237-249) is, in torch, a ``cat`` of eight
tensors, three 1 x 1 ``Conv1d`` with ``tanh``, a mean over the Gaussians, five ``TransformNet``s on the 16 latent values,
seven broadcast matrix products and a second ``cat``.  Here (C ABI: pigs_input_transform_*), for d = 2, c = 1..4 channels
and p = pde_size = 1..4, float32 on one GPU:

    x_n      = (means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde)_n
    latent   = mean_n tanh(W3 tanh(W2 tanh(W1 x_n + b1) + b2) + b3)                        latent_net
    T_j      = I + reshape(net_j(latent), k_j, k_j),   k = (2, c, 2c, 2c, p)               the five TransformNets
    t_params = (T Sigma_n, T_u u_n, boundaries_n, T_u sample_u_n, T_ux ux_n, T_uxx uxx_n, T_pde pde_n)

    matrices = transform_matrices(means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde,
                                  params)                                 # [4 + 9 c^2 + p^2], two launches
    t_params = apply_transforms(matrices, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx,
                                sample_pde)                               # [1, N, 5 + 6c + p], one launch

They are two autograd Functions so that the split path (``transform_gaussians``, :137-152, :280-296) applies the SAME
matrices to new rows; autograd adds the matrices' two gradients.  ``params`` is the 36 tensors of ``PARAM_ORDER``.
Gradients go to means, full_covariances, u and the parameters, where ``needs_input_grad`` asks; boundaries and the four
``sample_*`` are made under ``no_grad`` in the model, and one of them that requires a gradient is refused.  The reference's
``T means`` is computed and never used there; it is not built.  Once-differentiable, no float atomics (the same inputs
give the same bits on every call), capturable into a hipGraph; no CPU fallback.

    net = FusedInputTransform.from_module(model.dynamics_network.input_transform)
    t_params = net(means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde)
    more = net.transform_gaussians(full_covariances2, u2, sample_u2, sample_ux2, sample_uxx2, sample_pde2)
"""
import math

import torch

from . import _lib
from ._lib import pointers as _pointers, ptr as _ptr, stream as _stream

LATENT, HIDDEN1, HIDDEN2, LATENT_HIDDEN = 16, 48, 32, (16, 32, 16)
NET_NAMES = ("latent_net", "transform_net", "transform_u_net", "transform_ux_net", "transform_uxx_net", "transform_pde_net")
# the order of ``params``: per net of NET_NAMES, (weight, bias) of its three layers
PARAM_ORDER = tuple(f"{net}.layers.{2 * l}.{kind}" for net in NET_NAMES for l in range(3) for kind in ("weight", "bias"))
ROW_NAMES = ("means", "full_covariances", "u", "boundaries", "sample_u", "sample_ux", "sample_uxx", "sample_pde")


def in_dims(c, p):
    """columns of t_params (DynamicsNetwork.in_dims at d = 2)"""
    return 5 + 6 * c + p


def matrix_floats(c, p):
    return 4 + 9 * c * c + p * p


def matrix_blocks(c, p):
    """(offset, k) of T, T_u, T_ux, T_uxx, T_pde in the packed matrices"""
    ks = (2, c, 2 * c, 2 * c, p)
    offs = [0]
    for k in ks[:-1]:
        offs.append(offs[-1] + k * k)
    return tuple(zip(offs, ks))


def param_shapes(c, p):
    """the 36 shapes of ``params`` (a Conv1d weight [out, in, 1] counts as [out, in])"""
    shapes = []
    widths = (7 + 6 * c + p,) + LATENT_HIDDEN
    for i, o in zip(widths[:-1], widths[1:]):
        shapes += [(o, i), (o,)]
    for k in (2, c, 2 * c, 2 * c, p):
        for i, o in ((LATENT, HIDDEN1), (HIDDEN1, HIDDEN2), (HIDDEN2, k * k)):
            shapes += [(o, i), (o,)]
    return shapes


def _check(rows, need_means, others):
    """the refusals, with the exception types of mlp._check; returns (N, c, p, the row arrays as the ABI reads them).
    ``rows``: the eight of ROW_NAMES (means None where not read, boundaries None = zeros); ``others(c, p)``: (name,
    tensor, shape) of the further tensors of the call"""
    for name, t in zip(ROW_NAMES, rows):
        if t is None and ((name == "boundaries" and not need_means) or (name == "means" and not need_means)):
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    means, cov, u, bnd, su, ux, uxx, pde = rows
    if u.dim() != 2:
        raise ValueError(f"u must be [N, c], got {tuple(u.shape)}")
    N, c = u.shape
    if pde.dim() != 2:
        raise ValueError(f"sample_pde must be [N, pde_size], got {tuple(pde.shape)}")
    p = pde.shape[1]
    if N < 1:
        raise ValueError("no rows: N must be at least 1")
    if not 1 <= c <= 4:
        raise NotImplementedError(f"{c} channels: c must be in 1..4")
    if not 1 <= p <= 4:
        raise NotImplementedError(f"pde_size {p}: it must be in 1..4")
    if means is not None and means.dim() == 2 and means.shape[1] != 2:
        raise NotImplementedError(f"means of shape {tuple(means.shape)}: d = 2 only")
    if cov.dim() == 3 and cov.shape[1:] != (2, 2):
        raise NotImplementedError(f"full_covariances of shape {tuple(cov.shape)}: d = 2 only")
    want = {"means": [(N, 2)], "full_covariances": [(N, 2, 2), (N, 4)], "u": [(N, c)], "boundaries": [(N, 1), (1, N, 1), (N,)],
            "sample_u": [(N, c)], "sample_ux": [(N, 2 * c)], "sample_uxx": [(N, 2 * c)], "sample_pde": [(N, p)]}
    present = [(name, t) for name, t in zip(ROW_NAMES, rows) if t is not None]
    for name, t in present:
        if tuple(t.shape) not in want[name]:
            raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in want[name])}, got {tuple(t.shape)}")
    for name, t in present:
        if name not in ("means", "full_covariances", "u") and t.requires_grad:
            raise NotImplementedError(f"{name} requires a gradient: the model makes it under no_grad, and its gradient "
                                      "is not built")
    for name, t, shape in others(c, p):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        got = tuple(t.shape[:2]) if t.dim() == 3 and t.shape[2] == 1 and len(shape) == 2 else tuple(t.shape)
        if got != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)} at c = {c}, pde_size = {p}, got {tuple(t.shape)}")
        present.append((name, t))
    if any(t.dtype != torch.float32 for _, t in present):
        raise TypeError(f"dtypes {sorted({str(t.dtype) for _, t in present})}: float32 only")
    for name, t in present:
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    for name, t in present:
        if not t.is_cuda or t.device != u.device:
            raise RuntimeError(f"{name} is on {t.device}" + (f", u on {u.device}" if t is not u else "")
                               + ": the input transform runs on one GPU (no CPU fallback)")
    flat = (means, cov.reshape(N, 4), u, None if bnd is None else bnd.reshape(N), su, ux, uxx, pde)
    return N, c, p, flat


def _scratch(lib, N, c, p, device):
    nbytes = lib.pigs_input_transform_scratch_bytes(N, c, p)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


class _TransformMatrices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, cov, u, bnd, su, ux, uxx, pde, *params):
        lib = _lib.load()
        N, c, p = u.shape[0], u.shape[1], pde.shape[1]
        latent = torch.empty(LATENT, dtype=u.dtype, device=u.device)
        matrices = torch.empty(matrix_floats(c, p), dtype=u.dtype, device=u.device)
        scratch, nbytes = _scratch(lib, N, c, p, u.device)
        rows = (means, cov, u, bnd, su, ux, uxx, pde)
        with torch.cuda.device(u.device):
            rc = lib.pigs_input_transform_matrices_forward(_lib.PIGS_F32, N, c, p, *[_ptr(t) for t in rows], _pointers(params),
                                                           _ptr(scratch), nbytes, _ptr(latent), _ptr(matrices),
                                                           _stream(u.device))
        _lib.check(rc, "pigs_input_transform_matrices_forward")
        ctx.save_for_backward(*rows, latent, *params)
        ctx.mark_non_differentiable(latent)
        ctx.set_materialize_grads(False)           # no zeros launched for latent's absent gradient
        return matrices, latent

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_matrices, _g_latent):
        saved = ctx.saved_tensors
        rows, latent, params = saved[:8], saved[8], saved[9:]
        needs = ctx.needs_input_grad
        if not any(needs):
            return (None,) * len(needs)
        lib = _lib.load()
        u = rows[2]
        N, c, p = u.shape[0], u.shape[1], rows[7].shape[1]
        g_matrices = g_matrices.contiguous()
        g_rows = [torch.empty_like(rows[k]) if needs[k] else None for k in range(3)]
        g_params = [torch.empty_like(t) if need else None for t, need in zip(params, needs[8:])]
        scratch, nbytes = _scratch(lib, N, c, p, u.device)
        with torch.cuda.device(u.device):
            rc = lib.pigs_input_transform_matrices_backward(_lib.PIGS_F32, N, c, p, *[_ptr(t) for t in rows], _pointers(params),
                                                            _ptr(latent), _ptr(g_matrices), _ptr(scratch), nbytes,
                                                            *[_ptr(t) for t in g_rows], _pointers(g_params),
                                                            _stream(u.device))
        _lib.check(rc, "pigs_input_transform_matrices_backward")
        return (*g_rows, None, None, None, None, None, *g_params)


class _ApplyTransforms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, matrices, cov, u, bnd, su, ux, uxx, pde):
        lib = _lib.load()
        N, c, p = u.shape[0], u.shape[1], pde.shape[1]
        out = torch.empty((N, in_dims(c, p)), dtype=u.dtype, device=u.device)
        with torch.cuda.device(u.device):
            rc = lib.pigs_input_transform_apply_forward(_lib.PIGS_F32, N, c, p, _ptr(matrices), _ptr(cov), _ptr(u), _ptr(bnd),
                                                        _ptr(su), _ptr(ux), _ptr(uxx), _ptr(pde), _ptr(out), _stream(u.device))
        _lib.check(rc, "pigs_input_transform_apply_forward")
        ctx.save_for_backward(matrices, cov, u, su, ux, uxx, pde)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        matrices, cov, u, su, ux, uxx, pde = ctx.saved_tensors
        needs = ctx.needs_input_grad
        if not any(needs[:3]):
            return (None,) * 8
        lib = _lib.load()
        N, c, p = u.shape[0], u.shape[1], pde.shape[1]
        g_out = g_out.contiguous()
        g_matrices, g_cov, g_u = [torch.empty_like(t) if need else None for t, need in zip((matrices, cov, u), needs)]
        scratch, nbytes = _scratch(lib, N, c, p, u.device) if needs[0] else (None, 0)
        with torch.cuda.device(u.device):
            rc = lib.pigs_input_transform_apply_backward(_lib.PIGS_F32, N, c, p, _ptr(matrices), _ptr(cov), _ptr(u), _ptr(su),
                                                         _ptr(ux), _ptr(uxx), _ptr(pde), _ptr(g_out), _ptr(scratch), nbytes,
                                                         _ptr(g_cov), _ptr(g_u), _ptr(g_matrices), _stream(u.device))
        _lib.check(rc, "pigs_input_transform_apply_backward")
        return g_matrices, g_cov, g_u, None, None, None, None, None


def transform_matrices(means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde, params,
                       return_latent=False):
    """The packed matrices (T, T_u, T_ux, T_uxx, T_pde) [4 + 9 c^2 + p^2] of the Gaussians; see the module text.  With
    ``return_latent`` also the latent mean [16] (not differentiable: the backward recomputes from it)."""
    params = tuple(params)
    if len(params) != len(PARAM_ORDER):
        raise ValueError(f"{len(params)} parameters: {len(PARAM_ORDER)} expected, in the order of PARAM_ORDER")
    N, c, p, rows = _check((means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde), True,
                           lambda c, p: zip(PARAM_ORDER, params, param_shapes(c, p)))
    flat = [t.reshape(t.shape[0], t.shape[1]) if t.dim() == 3 else t for t in params]      # Conv1d [out, in, 1]: a view
    matrices, latent = _TransformMatrices.apply(*rows, *flat)
    return (matrices, latent) if return_latent else matrices


def apply_transforms(matrices, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde):
    """t_params [1, N, 5 + 6c + p] of the rows under the packed ``matrices``; ``boundaries`` None = zeros (new
    Gaussians, model_pn.py:282)."""
    N, c, p, rows = _check((None, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde), False,
                           lambda c, p: [("matrices", matrices, (matrix_floats(c, p),))])
    return _ApplyTransforms.apply(matrices, *rows[1:])[None]


def _layers_of(module, name, conv):
    """the three layers of child ``name`` (found by name and type), refusing what the kernels do not cover"""
    nn = torch.nn
    child = getattr(module, name, None)
    seq = getattr(child, "layers", None)
    if not isinstance(seq, nn.Sequential):
        raise TypeError(f"{name}.layers: an nn.Sequential expected, got {type(seq).__name__}")
    mods = list(seq)
    kind = nn.Conv1d if conv else nn.Linear
    expected = 6 if conv else 5
    if len(mods) != expected:
        raise NotImplementedError(f"{name}.layers has {len(mods)} modules: {expected} expected (three {kind.__name__} with "
                                  f"nn.Tanh {'after each' if conv else 'between them'})")
    layers = []
    for k, m in enumerate(mods):
        if k % 2:
            if not isinstance(m, nn.Tanh):
                raise NotImplementedError(f"{name}.layers.{k} is {type(m).__name__}: nn.Tanh is the only activation built")
            continue
        if not isinstance(m, kind):
            raise NotImplementedError(f"{name}.layers.{k} is {type(m).__name__}: {kind.__name__} expected")
        if conv and (tuple(m.kernel_size) != (1,) or tuple(m.stride) != (1,) or tuple(m.padding) != (0,)
                     or tuple(m.dilation) != (1,) or m.groups != 1):
            raise NotImplementedError(f"{name}.layers.{k} is {m}: a kernel size other than 1 (stride 1, no padding, one "
                                      "group) is not built")
        if m.bias is None:
            raise NotImplementedError(f"{name}.layers.{k} has bias=False: not built")
        layers.append(m)
    return layers


def _widths(layers):
    w = [layers[0].weight.shape[1]] + [m.weight.shape[0] for m in layers]
    for a, m in zip(w[:-1], layers):
        if m.weight.shape[1] != a:
            raise NotImplementedError(f"widths {w} do not chain")
    return w


class FusedInputTransform(torch.nn.Module):
    """``InputTransform`` over the SAME child modules under the same names (``latent_net``, ``transform_net``, ...), so the
    Parameters are the same objects under the same ``state_dict`` keys; only the forward differs.  ``forward`` returns
    ``t_params`` [1, N, in_dims] (the cat of model_pn.py:248-249) and keeps the packed matrices in ``self.matrices`` for
    ``transform_gaussians``."""

    def __init__(self, module):
        layers = {name: _layers_of(module, name, conv=(name == "latent_net")) for name in NET_NAMES}
        ks = []
        for name in NET_NAMES[1:]:
            w = _widths(layers[name])
            k = math.isqrt(w[3])
            if w[:3] != [LATENT, HIDDEN1, HIDDEN2] or k * k != w[3]:
                raise NotImplementedError(f"{name} has widths {w}: {[LATENT, HIDDEN1, HIDDEN2]} and a square expected")
            ks.append(k)
        if ks[0] != 2:
            raise NotImplementedError(f"transform_net gives {ks[0]} x {ks[0]} matrices: d = 2 only")
        c, p = ks[1], ks[4]
        if not 1 <= c <= 4 or not 1 <= p <= 4:
            raise NotImplementedError(f"c = {c}, pde_size = {p}: both must be in 1..4")
        if ks[2] != 2 * c or ks[3] != 2 * c:
            raise NotImplementedError(f"transform_ux_net / transform_uxx_net give {ks[2]} and {ks[3]} rows at c = {c}: widths "
                                      f"other than d c = {2 * c} are not built")
        w = _widths(layers["latent_net"])
        if w != [7 + 6 * c + p, *LATENT_HIDDEN]:
            raise NotImplementedError(f"latent_net has widths {w}: {[7 + 6 * c + p, *LATENT_HIDDEN]} expected at c = {c}, "
                                      f"pde_size = {p}")
        super().__init__()
        for name in NET_NAMES:
            setattr(self, name, getattr(module, name))
        self.c, self.d, self.pde_size = c, 2, p
        self.matrices = None
        self.latent = None

    @classmethod
    def from_module(cls, module):
        return cls(module)

    def params(self):
        """the 36 Parameters in PARAM_ORDER"""
        out = []
        for name in NET_NAMES:
            seq = getattr(self, name).layers
            for k in (0, 2, 4):
                out += [seq[k].weight, seq[k].bias]
        return out

    def forward(self, means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde):
        self.matrices, self.latent = transform_matrices(means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx,
                                                        sample_pde, self.params(), return_latent=True)
        return apply_transforms(self.matrices, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde)

    def transform_gaussians(self, full_covariances, u, sample_u, sample_ux, sample_uxx, sample_pde):
        """``t_params`` [1, n, in_dims] of new Gaussians under the matrices of the last ``forward`` (boundaries = 0), one
        launch (model_pn.py:137-152, :280-295; the reference's transformed means are unused and not built)"""
        if self.matrices is None:
            raise RuntimeError("transform_gaussians before forward: there are no matrices yet")
        return apply_transforms(self.matrices, full_covariances, u, None, sample_u, sample_ux, sample_uxx, sample_pde)
