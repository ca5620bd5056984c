"""GaussianAdam: the Gaussians' parameterisation, its backward and Adam in one HIP launch per step.

In the reference's MLP-free loops the Gaussians themselves are the parameters (test_no_mlp.py:99-104, 146, 185-186;
test_initialize.py:100-111, 151, 172-180).  Around the sampler such a step runs ``tanh(raw_means) * scale``,
``exp(raw_scaling)``, ``build_covariances``, the autograd backward of each, ``torch.optim.Adam`` over four tensors and
``zero_grad``: about twenty launches of O(N) work.  Here that is ONE launch (C ABI: pigs_optim_step):

    opt = GaussianAdam(raw_means, values, raw_scaling, transform, lr=1e-2, means_map="tanh", scale=2.5)
    for step in ...:
        g = opt.gaussians()                    # (means, values, covariances, conics): leaves that require grad
        sampler.preprocess(g.means, g.values, g.covariances, g.conics, samples)
        loss = ...; loss.backward()            # fills g.means.grad, g.values.grad, g.conics.grad (g.covariances.grad if used)
        opt.step()                             # one launch; then the four .grad are None

``step()`` applies the chain rule to the leaves' gradients, updates the four parameters in place as torch.optim.Adam
would, wraps the means (identity map with ``wrap=(lo, hi)``) and writes the NEXT step's means, covariances and conics,
so the next ``gaussians()`` launches nothing.  The only other launch is the materialising one (pigs_optim_materialize):
at the first ``gaussians()`` and after ``load_state_dict`` / ``refine``.

    means_map="tanh"      means = tanh(raw_means) * scale
    means_map="identity"  means = raw_means; ``wrap=(lo, hi)``: after the update a coordinate > hi is lowered by hi - lo
                          and one < lo raised by it (one shift, strict inequalities: test_initialize.py:175-180)
    s = exp(raw_scaling), tau = tanh(transform) sqrt(s0 s1), covariances [s0, tau, s1], conics their inverses (flat)

Four groups -- means, values, scaling, transform -- each with its own rate (``lr``: a float or a dict over the four
names, mutable between steps) and its own step count: a group whose gradient is None is left untouched, as torch
leaves a parameter with ``p.grad is None`` (scaling and transform are present when the conics' or the covariances'
gradient is).  The powers beta^t are running products in double: on the host, or with ``capturable=True`` in a small
device state that a one-thread launch in front of the update advances, the rates in ``opt.lr_tensor`` (double [4] on
the device, written in place between replays); the two modes give bit-identical updates.  In the capturable mode the
means, covariances and conics live in three static buffers (a graph replay must read what the replay before it wrote)
and ``gaussians()`` returns fresh leaves over them; otherwise every step writes fresh tensors.

``grad_stats=True`` keeps, in the same launch (C ABI: pigs_optim_step_stats), what the reference's densification reads
from ``raw_means.grad`` and ``scaling.grad`` (test_no_mlp.py:149-155, 203-205; test_no_mlp_1d.py:156-162, 215-222), which
here exist only in the kernel's registers.  With G the gradient of a raw parameter as Adam consumes it, per step and for
a group whose gradient is present:  last = G,  sum += G,  norm += ||sum||_2 per row (of the sum AFTER adding):

    opt.grad_stats           GradStats(mean_grad, mean_grad_norm, scale_grad, scale_grad_norm, last_mean_grad,
                             last_scale_grad): live buffers in the parameters' dtype, updated in place by step()
    opt.grad_counts          {"means": n, "scaling": n}: steps accumulated (capturable mode: a device read)
    opt.reset_grad_stats()   zero the sums and the counts, in place (the reference starts after its warm-up, :149)
    opt.refine(source, child, shift_means=None)   the statistics restart as zeros of the new row count (:249-252);
                             ``shift_means [N_old, d]``: a row with child >= 0 gets raw_means[source] + shift_means[source],
                             the ``+ split_dir`` of test_no_mlp_1d.py:219-222

``GaussianAdam1D(raw_means [N,1], values [N,c], raw_scaling [N,1], ...)`` is the same for d = 1 (test_no_mlp_1d.py:109-111,
test_initialize_1d.py:54-56; C ABI: pigs_optim1d_materialize, pigs_optim1d_step): three groups (means, values, scaling),
s = exp(raw_scaling), covariances = s, conics = 1 / s, all leaves [N,1].

GaussianAdam: d = 2; GaussianAdam1D: d = 1.  c = 1..4, float32 / float64, GPU tensors only, no CPU fallback.
weight_decay, amsgrad and maximize are not built.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream

MEANS_MAPS = {"tanh": 0, "identity": 1}
GROUPS = ("means", "values", "scaling", "transform")

GROUPS_1D = ("means", "values", "scaling")
STAT_GROUPS = ("means", "scaling")

Gaussians = collections.namedtuple("Gaussians", "means values covariances conics")
GradStats = collections.namedtuple("GradStats", "mean_grad mean_grad_norm scale_grad scale_grad_norm last_mean_grad "
                                                "last_scale_grad")


def _check(raw_means, values, raw_scaling, transform):
    names = ("raw_means", "values", "raw_scaling", "transform")
    arrays = (raw_means, values, raw_scaling, transform)
    for n, a in zip(names, arrays):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor")
    if raw_means.dim() != 2 or raw_means.shape[1] != 2:
        raise NotImplementedError(f"raw_means must be [N, 2] (d = 2), got {tuple(raw_means.shape)}")
    N = raw_means.shape[0]
    if N < 1:
        raise ValueError("no Gaussians: N must be at least 1")
    if raw_scaling.dim() != 2 or raw_scaling.shape[1] != 2:
        raise NotImplementedError(f"raw_scaling must be [N, 2] (d = 2), got {tuple(raw_scaling.shape)}")
    if transform.dim() not in (1, 2) or (transform.dim() == 2 and transform.shape[1] != 1):
        raise NotImplementedError(f"transform must be [N] or [N, 1] (d = 2), got {tuple(transform.shape)}")
    if values.dim() != 2 or not 1 <= values.shape[1] <= 4:
        raise NotImplementedError(f"values must be [N, c] with c = 1..4, got {tuple(values.shape)}")
    for n, a in zip(names[1:], arrays[1:]):
        if a.shape[0] != N:
            raise ValueError(f"{n} holds {a.shape[0]} rows, raw_means {N}")
    if raw_means.dtype not in _DTYPES or any(a.dtype != raw_means.dtype for a in arrays):
        raise TypeError(f"dtypes {[str(a.dtype) for a in arrays]}: float32 or float64, all alike")
    for n, a in zip(names, arrays):
        if not a.is_cuda or a.device != raw_means.device:
            raise RuntimeError(f"{n} is on {a.device}" + (f", raw_means on {raw_means.device}" if a is not raw_means else "")
                               + ": the optimiser runs on one GPU (no CPU fallback)")
    for n, a in zip(names, arrays):
        if not a.is_contiguous():
            raise ValueError(f"{n} must be contiguous: it is updated in place")
    for n, a in ((names[0], raw_means), (names[2], raw_scaling)):
        if a.data_ptr() % (2 * a.element_size()):
            raise ValueError(f"{n} must be aligned to a row ({2 * a.element_size()} bytes): it is updated in place")


def _check_1d(raw_means, values, raw_scaling):
    names = ("raw_means", "values", "raw_scaling")
    arrays = (raw_means, values, raw_scaling)
    for n, a in zip(names, arrays):
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor")
    for n, a in ((names[0], raw_means), (names[2], raw_scaling)):
        if a.dim() != 2 or a.shape[1] != 1:
            raise NotImplementedError(f"{n} must be [N, 1] (d = 1; GaussianAdam is d = 2), got {tuple(a.shape)}")
    N = raw_means.shape[0]
    if N < 1:
        raise ValueError("no Gaussians: N must be at least 1")
    if values.dim() != 2 or not 1 <= values.shape[1] <= 4:
        raise NotImplementedError(f"values must be [N, c] with c = 1..4, got {tuple(values.shape)}")
    for n, a in zip(names[1:], arrays[1:]):
        if a.shape[0] != N:
            raise ValueError(f"{n} holds {a.shape[0]} rows, raw_means {N}")
    if raw_means.dtype not in _DTYPES or any(a.dtype != raw_means.dtype for a in arrays):
        raise TypeError(f"dtypes {[str(a.dtype) for a in arrays]}: float32 or float64, all alike")
    for n, a in zip(names, arrays):
        if not a.is_cuda or a.device != raw_means.device:
            raise RuntimeError(f"{n} is on {a.device}" + (f", raw_means on {raw_means.device}" if a is not raw_means else "")
                               + ": the optimiser runs on one GPU (no CPU fallback)")
    for n, a in zip(names, arrays):
        if not a.is_contiguous():
            raise ValueError(f"{n} must be contiguous: it is updated in place")


def _rates(lr, GROUPS=GROUPS):
    if isinstance(lr, dict):
        if set(lr) != set(GROUPS):
            raise ValueError(f"lr as a dict needs exactly the keys {GROUPS}, got {sorted(lr)}")
        out = {g: float(lr[g]) for g in GROUPS}
    else:
        out = {g: float(lr) for g in GROUPS}
    for g, r in out.items():
        if not r >= 0.0:
            raise ValueError(f"lr[{g!r}] = {r}: a rate is not negative")
    return out


def follow_maps(param, exp_avg, exp_avg_sq, source, child, shift=None):
    """One group through ``pigs_amd.refine``'s maps (test_no_mlp.py:218-240): the parameter and its two moments
    ``index_select``-ed by ``source``, the moments of the rows with ``child >= 0`` zeroed.  With ``shift`` (of the old
    parameter's shape) a row with ``child >= 0`` is ``param[source] + shift[source]`` (test_no_mlp_1d.py:219-222).
    Torch ops, any device."""
    with torch.no_grad():
        fresh = (child >= 0).reshape((-1,) + (1,) * (param.dim() - 1))
        moments = []
        for m in (exp_avg, exp_avg_sq):
            carried = m.index_select(0, source)
            moments.append(torch.where(fresh, torch.zeros_like(carried), carried))
        new = param.detach().index_select(0, source)
        if shift is not None:
            new = torch.where(fresh, new + shift.detach().index_select(0, source), new)
        return new, moments[0], moments[1]


class GaussianAdam:
    """Adam over (raw_means [N,2], values [N,c], raw_scaling [N,2], transform [N,1] or [N]); see the module text.
    The four tensors (plain or nn.Parameter) are updated in place."""

    GROUPS = GROUPS
    _WIDTHS = (2, 3, 3)               # means, covariances, conics
    _ROWS_OF_TWO = True

    def __init__(self, raw_means, values, raw_scaling, transform, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *,
                 means_map="tanh", scale=1.0, wrap=None, capturable=False, grad_stats=False, weight_decay=0, amsgrad=False,
                 maximize=False):
        self._setup((raw_means, values, raw_scaling, transform), lr, betas, eps, means_map, scale, wrap, capturable,
                    grad_stats, weight_decay, amsgrad, maximize)

    def _setup(self, params, lr, betas, eps, means_map, scale, wrap, capturable, grad_stats, weight_decay, amsgrad, maximize):
        GROUPS = self.GROUPS
        if weight_decay != 0 or amsgrad or maximize:
            raise NotImplementedError("weight_decay, amsgrad and maximize are not built")
        if means_map not in MEANS_MAPS:
            raise ValueError(f"means_map must be 'tanh' or 'identity', got {means_map!r}")
        if wrap is not None:
            if means_map != "identity":
                raise ValueError("wrap goes with means_map='identity'")
            lo, hi = (float(x) for x in wrap)
            if not lo < hi:
                raise ValueError(f"wrap = ({lo}, {hi}): needs lo < hi")
            wrap = (lo, hi)
        beta1, beta2 = (float(b) for b in betas)
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError(f"betas = {betas}: each in [0, 1)")
        if not float(eps) >= 0.0:
            raise ValueError(f"eps = {eps}: not negative")
        rates = _rates(lr, GROUPS)
        self._check_params(*params)
        _lib.load()
        self._set_params(params)
        self.means_map, self.scale, self.wrap = means_map, float(scale), wrap
        self.betas, self.eps, self.capturable = (beta1, beta2), float(eps), bool(capturable)
        self._lr = rates
        self.device, self.dtype = self.raw_means.device, self.raw_means.dtype
        self.lr_tensor = self.state_tensor = self.counts_tensor = None
        if self.capturable:
            self.lr_tensor = torch.tensor(self._four(self._lr, 0.0), dtype=torch.float64, device=self.device)
            # beta1^t [4], beta2^t [4], step counts [4]
            self.state_tensor = torch.tensor([1.0] * 8 + [0.0] * 4, dtype=torch.float64, device=self.device)
        self._steps = {g: 0 for g in GROUPS}
        self._pow1 = {g: 1.0 for g in GROUPS}
        self._pow2 = {g: 1.0 for g in GROUPS}
        self._zero_moments()
        self._stats = None        # GradStats, with grad_stats=True
        self._stat_counts = {g: 0 for g in STAT_GROUPS}
        if grad_stats:
            self._stats = self._zero_stats()
            if self.capturable:   # steps accumulated for means, scaling: advanced by the one-thread launch
                self.counts_tensor = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._static = None       # capturable: the three buffers every step writes
        self._next = None         # (means, covariances, conics) of the current parameters, or None: materialise
        self._leaves = None       # what gaussians() handed out and step() reads the gradients of

    _check_params = staticmethod(_check)

    def _four(self, per_group, pad):
        """a per-group dict as the four slots of the C ABI's arrays (d = 1 leaves the last one unused)"""
        return [per_group[g] for g in self.GROUPS] + [pad] * (4 - len(self.GROUPS))

    # ---- state ------------------------------------------------------------------------------------------------
    def _set_params(self, params):
        self.raw_means, self.values, self.raw_scaling, self.transform = params

    def _params(self):
        return (self.raw_means, self.values, self.raw_scaling, self.transform)

    def _zero_moments(self):
        self.exp_avg = {g: torch.zeros_like(p, requires_grad=False) for g, p in zip(self.GROUPS, self._params())}
        self.exp_avg_sq = {g: torch.zeros_like(p, requires_grad=False) for g, p in zip(self.GROUPS, self._params())}

    def _zero_stats(self):
        N, d = self.raw_means.shape
        rows = lambda: torch.zeros((N, d), dtype=self.dtype, device=self.device)
        norm = lambda: torch.zeros(N, dtype=self.dtype, device=self.device)
        return GradStats(rows(), norm(), rows(), norm(), rows(), rows())

    @property
    def lr(self):
        """The rates, a dict over the groups; assign a float or a dict.  Host mode reads it at every step (entries may
        be changed in place); the capturable mode reads ``lr_tensor``, which an assignment rewrites."""
        return self._lr

    @lr.setter
    def lr(self, lr):
        self._lr = _rates(lr, self.GROUPS)
        if self.capturable:
            self.lr_tensor.copy_(torch.tensor(self._four(self._lr, 0.0), dtype=torch.float64))

    @property
    def steps(self):
        """Steps taken per group (a group whose gradient was None did not step).  Capturable mode: a device read."""
        if self.capturable:
            counts = self.state_tensor[8:].tolist()
            return {g: int(n) for g, n in zip(self.GROUPS, counts)}
        return dict(self._steps)

    def _need_stats(self):
        if self._stats is None:
            raise RuntimeError("this optimiser keeps no gradient statistics: construct it with grad_stats=True")

    @property
    def grad_stats(self):
        """GradStats(mean_grad, mean_grad_norm, scale_grad, scale_grad_norm, last_mean_grad, last_scale_grad): the live
        buffers ``step()`` updates in place (replaced by ``refine`` alone)."""
        self._need_stats()
        return self._stats

    @property
    def grad_counts(self):
        """Steps accumulated since the last reset, {"means": n, "scaling": n}.  Capturable mode: a device read."""
        self._need_stats()
        if self.capturable:
            return {g: int(n) for g, n in zip(STAT_GROUPS, self.counts_tensor.tolist())}
        return dict(self._stat_counts)

    def reset_grad_stats(self):
        """Zero the sums, the last gradients and the counts, in place (capturable: launches that a graph may hold)."""
        self._need_stats()
        for t in self._stats:
            t.zero_()
        self._stat_counts = {g: 0 for g in STAT_GROUPS}
        if self.capturable:
            self.counts_tensor.zero_()

    def state_dict(self):
        """This class's own layout: counts and running products per group, clones of the moments, the rates; with
        ``grad_stats`` the statistics and their counts under "grad_stats"."""
        GROUPS = self.GROUPS
        if self.capturable:
            host = self.state_tensor.tolist()
            pow1, pow2 = dict(zip(GROUPS, host[:4])), dict(zip(GROUPS, host[4:8]))
            lr = dict(zip(GROUPS, self.lr_tensor.tolist()))
        else:
            pow1, pow2, lr = dict(self._pow1), dict(self._pow2), dict(self._lr)
        out = {"step": self.steps, "beta1_pow": pow1, "beta2_pow": pow2, "lr": lr, "betas": self.betas, "eps": self.eps,
               "exp_avg": {g: t.clone() for g, t in self.exp_avg.items()},
               "exp_avg_sq": {g: t.clone() for g, t in self.exp_avg_sq.items()}}
        if self._stats is not None:
            out["grad_stats"] = dict({k: t.clone() for k, t in self._stats._asdict().items()}, counts=self.grad_counts)
        return out

    def load_state_dict(self, state):
        GROUPS = self.GROUPS
        for key in ("exp_avg", "exp_avg_sq"):
            for g, p in zip(GROUPS, self._params()):
                t = state[key][g]
                if t.shape != p.shape:
                    raise ValueError(f"{key}[{g!r}] is {tuple(t.shape)}, the parameter {tuple(p.shape)}")
        if self._stats is not None and "grad_stats" in state:
            for k, mine in self._stats._asdict().items():
                if state["grad_stats"][k].shape != mine.shape:
                    raise ValueError(f"grad_stats[{k!r}] is {tuple(state['grad_stats'][k].shape)}, here {tuple(mine.shape)}")
        self.exp_avg = {g: state["exp_avg"][g].to(device=self.device, dtype=self.dtype, copy=True).contiguous()
                           for g in GROUPS}
        self.exp_avg_sq = {g: state["exp_avg_sq"][g].to(device=self.device, dtype=self.dtype, copy=True).contiguous()
                           for g in GROUPS}
        self.betas, self.eps = tuple(float(b) for b in state["betas"]), float(state["eps"])
        self._steps = {g: int(state["step"][g]) for g in GROUPS}
        self._pow1 = {g: float(state["beta1_pow"][g]) for g in GROUPS}
        self._pow2 = {g: float(state["beta2_pow"][g]) for g in GROUPS}
        if self.capturable:
            host = self._four(self._pow1, 1.0) + self._four(self._pow2, 1.0) + self._four(self._steps, 0.0)
            self.state_tensor.copy_(torch.tensor(host, dtype=torch.float64))
        self.lr = state["lr"]
        if self._stats is not None:
            self.reset_grad_stats()               # a dict without the key: zeros
            if "grad_stats" in state:
                for k, mine in self._stats._asdict().items():
                    mine.copy_(state["grad_stats"][k])
                self._stat_counts = {g: int(state["grad_stats"]["counts"][g]) for g in STAT_GROUPS}
                if self.capturable:
                    self.counts_tensor.copy_(torch.tensor([float(self._stat_counts[g]) for g in STAT_GROUPS],
                                                          dtype=torch.float64))
        self._next = self._leaves = None          # the parameters may have been reloaded too: materialise again

    # ---- the Gaussians ----------------------------------------------------------------------------------------
    def _outputs(self):
        N = self.raw_means.shape[0]
        if self.capturable:
            if self._static is None or self._static[0].shape[0] != N:
                self._static = tuple(torch.empty((N, w), dtype=self.dtype, device=self.device) for w in self._WIDTHS)
            return self._static
        return tuple(torch.empty((N, w), dtype=self.dtype, device=self.device) for w in self._WIDTHS)

    def _call_materialize(self, lib, outs):
        rc = lib.pigs_optim_materialize(_DTYPES[self.dtype], MEANS_MAPS[self.means_map], self.raw_means.shape[0],
                                        self.scale, _ptr(self.raw_means), _ptr(self.raw_scaling), _ptr(self.transform),
                                        *[_ptr(o) for o in outs], _stream(self.device))
        _lib.check(rc, "pigs_optim_materialize")

    def _materialize(self):
        lib = _lib.load()
        outs = self._outputs()
        with torch.cuda.device(self.device):
            self._call_materialize(lib, outs)
        for o in outs:
            torch.autograd.graph.increment_version(o)
        return outs

    def gaussians(self):
        """(means [N,d], values [N,c], covariances, conics ([N,3]; d = 1: [N,1])): leaves that require grad.  ``values``
        shares the parameter's storage.  Launches nothing after a ``step()``; the same leaves until the next ``step()``."""
        if self._leaves is not None:
            return self._leaves
        if self._next is None:
            self._next = self._materialize()
        means, cov, con = (t.detach().requires_grad_(True) for t in self._next)
        self._leaves = Gaussians(means, self.values.detach().requires_grad_(True), cov, con)
        return self._leaves

    def _grad(self, leaf, rows_of_two=False):
        g = leaf.grad
        if g is None:
            return None
        if g.dtype != self.dtype or g.device != self.device or g.shape != leaf.shape:
            raise TypeError(f"a gradient of {g.dtype} {tuple(g.shape)} on {g.device} for a leaf of {self.dtype} "
                            f"{tuple(leaf.shape)} on {self.device}")
        g = g.contiguous()
        if rows_of_two and g.data_ptr() % (2 * g.element_size()):
            g = g.clone()
        return g

    def _stats_struct(self):
        s = _lib.PigsGradStats()
        for k, t in self._stats._asdict().items():
            setattr(s, k, t.data_ptr())
        if self.capturable:
            s.device_counts = self.counts_tensor.data_ptr()
        return s

    def _call_step(self, lib, h, grads, outs):
        args = (_DTYPES[self.dtype], self.values.shape[1], self.raw_means.shape[0], ctypes.byref(h),
                *[_ptr(p) for p in self._params()], *[_ptr(self.exp_avg[g]) for g in GROUPS],
                *[_ptr(self.exp_avg_sq[g]) for g in GROUPS], *[_ptr(g) for g in grads], *[_ptr(o) for o in outs])
        if self._stats is None:
            _lib.check(lib.pigs_optim_step(*args, _stream(self.device)), "pigs_optim_step")
        else:
            s = self._stats_struct()
            _lib.check(lib.pigs_optim_step_stats(*args, ctypes.byref(s), _stream(self.device)), "pigs_optim_step_stats")

    def step(self):
        """One launch (two with ``capturable=True``): chain rule, Adam, wrap, the statistics, the next step's Gaussians."""
        if self._leaves is None:
            raise RuntimeError("step() without gaussians(): the gradients are read from the leaves it returns")
        GROUPS = self.GROUPS
        leaves = self._leaves
        grads = (self._grad(leaves.means, self._ROWS_OF_TWO), self._grad(leaves.values), self._grad(leaves.covariances),
                 self._grad(leaves.conics))
        if all(g is None for g in grads):
            return                # as torch.optim.Adam with no gradient anywhere: nothing moves, nothing is launched
        present = (grads[0] is not None, grads[1] is not None, grads[2] is not None or grads[3] is not None)
        present = dict(zip(GROUPS, present + (present[2],)))      # the transform (d = 2) goes with the scaling
        lib = _lib.load()
        h = _lib.PigsAdamStep()
        h.beta1, h.beta2, h.eps, h.scale = self.betas[0], self.betas[1], self.eps, self.scale
        h.means_map, h.wrap = MEANS_MAPS[self.means_map], int(self.wrap is not None)
        if self.wrap is not None:
            h.wrap_lo, h.wrap_hi = self.wrap
        if self.capturable:
            h.device_lr, h.device_state = self.lr_tensor.data_ptr(), self.state_tensor.data_ptr()
        else:
            for k, g in enumerate(GROUPS):
                if present[g]:
                    self._steps[g] += 1
                    self._pow1[g] *= self.betas[0]
                    self._pow2[g] *= self.betas[1]
                h.lr[k], h.beta1_pow[k], h.beta2_pow[k] = self._lr[g], self._pow1[g], self._pow2[g]
            if self._stats is not None:
                for g in STAT_GROUPS:
                    self._stat_counts[g] += int(present[g])
        outs = self._outputs()
        params = self._params()
        with torch.cuda.device(self.device):
            self._call_step(lib, h, grads, outs)
        # the writes went through raw pointers: a stale autograd node must complain as it would after torch.optim
        for g, p in zip(GROUPS, params):
            if present[g]:
                torch.autograd.graph.increment_version(p)
        if self._stats is not None:
            st = self._stats
            for g, arrays in zip(STAT_GROUPS, ((st.mean_grad, st.mean_grad_norm, st.last_mean_grad),
                                               (st.scale_grad, st.scale_grad_norm, st.last_scale_grad))):
                if present[g]:
                    for t in arrays:
                        torch.autograd.graph.increment_version(t)
        if self.capturable:
            for o in outs:
                torch.autograd.graph.increment_version(o)
        for leaf in leaves:
            leaf.grad = None
        self._next, self._leaves = outs, None

    # ---- refinement -------------------------------------------------------------------------------------------
    def refine(self, source, child, shift_means=None):
        """Make the parameters and their moments follow ``pigs_amd.refine``'s maps: ``index_select`` by ``source``, the
        moments of the rows with ``child >= 0`` zeroed (test_no_mlp.py:218-240).  With ``shift_means [N_old, d]`` a row
        with ``child >= 0`` gets ``raw_means[source] + shift_means[source]`` (the ``+ split_dir`` of
        test_no_mlp_1d.py:219-222, test_initialize_1d.py:108-111).  The parameters are replaced (their row count changes)
        and returned in the constructor's order, nn.Parameters where they were; the statistics restart as zeros of the
        new row count with counts 0 (test_no_mlp.py:249-252); the Gaussians are materialised again at the next
        ``gaussians()``.  Torch ops, not capturable."""
        if not (isinstance(source, torch.Tensor) and isinstance(child, torch.Tensor)):
            raise TypeError("source and child must be torch.Tensors (pigs_amd.refine_index)")
        if source.dim() != 1 or child.shape != source.shape:
            raise ValueError(f"source and child must be [N'] alike, got {tuple(source.shape)} and {tuple(child.shape)}")
        if source.device != self.device or child.device != self.device:
            raise RuntimeError(f"source is on {source.device}, child on {child.device}, the parameters on {self.device}")
        if source.shape[0] < 1:
            raise ValueError("refine would leave no Gaussians")
        if shift_means is not None:
            if not isinstance(shift_means, torch.Tensor) or shift_means.shape != self.raw_means.shape:
                raise ValueError(f"shift_means must be a tensor of raw_means' shape {tuple(self.raw_means.shape)}")
            if shift_means.device != self.device or shift_means.dtype != self.dtype:
                raise TypeError(f"shift_means is {shift_means.dtype} on {shift_means.device}, the parameters "
                                f"{self.dtype} on {self.device}")
        new = []
        for g, p in zip(self.GROUPS, self._params()):
            q, self.exp_avg[g], self.exp_avg_sq[g] = follow_maps(p, self.exp_avg[g], self.exp_avg_sq[g], source, child,
                                                                 shift_means if g == "means" else None)
            new.append(torch.nn.Parameter(q, requires_grad=p.requires_grad) if isinstance(p, torch.nn.Parameter) else q)
        self._set_params(new)
        if self._stats is not None:
            self._stats = self._zero_stats()
            self._stat_counts = {g: 0 for g in STAT_GROUPS}
            if self.capturable:
                self.counts_tensor.zero_()
        self._next = self._leaves = None
        return tuple(new)


class GaussianAdam1D(GaussianAdam):
    """Adam over (raw_means [N,1], values [N,c], raw_scaling [N,1]): GaussianAdam for d = 1, three groups; see the module
    text.  ``gaussians()`` returns means, covariances and conics as [N,1] leaves (reshape to [N,1,1] as the reference does
    at test_no_mlp_1d.py:74 if wanted)."""

    GROUPS = GROUPS_1D
    _WIDTHS = (1, 1, 1)
    _ROWS_OF_TWO = False
    _check_params = staticmethod(_check_1d)

    def __init__(self, raw_means, values, raw_scaling, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, means_map="tanh",
                 scale=1.0, wrap=None, capturable=False, grad_stats=False, weight_decay=0, amsgrad=False, maximize=False):
        self._setup((raw_means, values, raw_scaling), lr, betas, eps, means_map, scale, wrap, capturable, grad_stats,
                    weight_decay, amsgrad, maximize)

    def _set_params(self, params):
        self.raw_means, self.values, self.raw_scaling = params

    def _params(self):
        return (self.raw_means, self.values, self.raw_scaling)

    def _call_materialize(self, lib, outs):
        rc = lib.pigs_optim1d_materialize(_DTYPES[self.dtype], MEANS_MAPS[self.means_map], self.raw_means.shape[0],
                                          self.scale, _ptr(self.raw_means), _ptr(self.raw_scaling),
                                          *[_ptr(o) for o in outs], _stream(self.device))
        _lib.check(rc, "pigs_optim1d_materialize")

    def _call_step(self, lib, h, grads, outs):
        s = self._stats_struct() if self._stats is not None else None
        rc = lib.pigs_optim1d_step(_DTYPES[self.dtype], self.values.shape[1], self.raw_means.shape[0], ctypes.byref(h),
                                   *[_ptr(p) for p in self._params()], *[_ptr(self.exp_avg[g]) for g in GROUPS_1D],
                                   *[_ptr(self.exp_avg_sq[g]) for g in GROUPS_1D], *[_ptr(g) for g in grads],
                                   *[_ptr(o) for o in outs], ctypes.byref(s) if s is not None else None,
                                   _stream(self.device))
        _lib.check(rc, "pigs_optim1d_step")
