"""NetworkAdam: the network's Adam step and the loss-weighted rate of the loop with the network, in two HIP launches.

The loop the reference trains with (main_pn.py:171-232 driving model_pn.Model) steps ``torch.optim.Adam(model.parameters())``
(:59): 90 trainable tensors of some 30 000 elements, most under 1 024 -- a chain of launches at the launch floor -- and
before every step it sets ``g["lr"] = g["prev_lr"] * loss_weight`` (:217-218) from ``loss_weight *= np.exp(-epsilon *
current_loss.item())`` (:225), a device read per time step.  ``NetworkAdam`` is a drop-in for that optimiser
(C ABI: pigs_network_adam_step, csrc/network_adam.hip):

    opt = NetworkAdam(model.parameters(), lr=1e-3)                 # or capturable=True inside a GraphedStep
    for epoch in ...:
        opt.reset_rate_scale()                                     # loss_weight = 1 (:157)
        for time_step in ...:
            loss = ...; loss.backward()
            opt.step(loss=loss.detach(), decay=epsilon)            # two launches; every .grad is None afterwards
        total, worst, count = opt.loss_stats()                     # ONE device read per epoch: total_loss, all_sufficient
        opt.reset_loss_stats()

``step(loss=None, decay=0.0)`` reads ``p.grad`` of every tensor (``None``: the tensor sits the step out, its step count not
advanced, as torch does), launches the two kernels, advances the parameters' version counters and sets every ``.grad`` to
``None``.  With no gradient anywhere nothing is launched.  The step's rate is ``lr * rate_scale``; with a ``loss`` (a
one-element float32 / float64 tensor on the device) the launch then does, in double, ``rate_scale *= exp(-decay * loss)``,
``loss_sum += loss``, ``loss_max = max(loss_max, loss)``, ``loss_count += 1``: the step uses the rate from BEFORE the decay,
the order of main_pn.py:217-225.  A non-finite loss has no special case: IEEE arithmetic gives what the reference's line
gives (a NaN loss makes ``rate_scale``, the sum and the maximum NaN until they are reset; guard the loss with
``torch.where(torch.isfinite(l), l, 0)`` as the reference's :183-192 do).

    lr              eager: ``param_groups[0]["lr"]``, read at every step (the writes of main_pn.py:168-169, 217-218, 234-235
                    work as they are);  ``capturable=True``: ``opt.lr_tensor``, a 0-dim double on the device written in
                    place between replays.  The two modes give the same bits.
    rate_scale      a 0-dim double view of the device state; ``reset_rate_scale()`` sets it to 1 in place (capturable)
    loss_stats()    (sum, max, count) in one device read; ``reset_loss_stats()`` zeroes them in place (capturable)
    steps           the step count of every trainable tensor (a device read)

What it takes: ONE parameter group; at most 128 tensors that require grad (a tensor with ``requires_grad=False``, such as
the model's ``frequencies``, is accepted, never touched and takes no slot); GPU tensors on one device, contiguous, one
dtype (float32 or float64).  The parameters' addresses are read once, at construction; the gradients' at every step (under
capture they are the graph pool's and are recorded with the launch).  ``weight_decay``, ``amsgrad`` and ``maximize`` are
not built.  There is no CPU fallback.

Checkpoints are torch's: the moments live in two flat arrays (every tensor's segment padded to 4 elements), the step
counts and the running products beta^t in the device state, and ``opt.state`` is assembled from them when it is read (a
device read): per stepped parameter ``step`` (a float32 0-dim tensor), ``exp_avg`` and ``exp_avg_sq`` (views of the flat
arrays in the parameter's shape).  So ``state_dict()`` is what ``torch.optim.Adam`` writes and
``torch.optim.Adam.load_state_dict`` takes it; ``load_state_dict`` accepts a ``torch.optim.Adam`` state dict with state
for some, all or none of the parameters, copies into the flat arrays and rebuilds beta^t as ``step`` double
multiplications from 1.0, which is how the kernel forms them: a loaded run continues with the bits of an uninterrupted one.
The packing between the flat arrays and the per-tensor layout (``segment_offsets``, ``pack_moments``, ``unpack_moments``,
``running_products``) is pure functions of tensors on any device.
"""
import ctypes

import torch

from . import _lib
from ._lib import DTYPES as _DTYPES, stream as _stream

MAX_TENSORS = _lib.NETWORK_ADAM_MAX_TENSORS
HEAD = 4                      # rate_scale, loss_sum, loss_max, loss_count in front of the per-tensor arrays of the state


# ---- the layout, on any device ------------------------------------------------------------------------------
def segment_offsets(counts):
    """(offsets, total): tensor s owns ``counts[s]`` elements of a flat moment array from ``offsets[s]``; every segment
    starts at a multiple of 4 and ``total`` is one too."""
    offsets, at = [], 0
    for n in counts:
        offsets.append(at)
        at = (at + int(n) + 3) & ~3
    return offsets, at


def running_products(beta, steps):
    """beta^t for every t of ``steps``, as t double multiplications from 1.0 (how the kernel forms them)"""
    out, p, t = {}, 1.0, 0
    for n in sorted(set(int(s) for s in steps)):
        while t < n:
            p *= beta
            t += 1
        out[n] = p
    return [out[int(s)] for s in steps]


def pack_moments(state, positions, shapes, exp_avg, exp_avg_sq):
    """The ``state`` half of a torch.optim.Adam state dict (keyed by the parameter's position in its group) into the two
    flat arrays, in place: slot s is the parameter at ``positions[s]``, of shape ``shapes[s]``; a slot without an entry
    gets zeros.  Returns the slots' step counts."""
    offsets, total = segment_offsets([_numel(s) for s in shapes])
    if exp_avg.shape != (total,) or exp_avg_sq.shape != (total,):
        raise ValueError(f"the flat moments hold {tuple(exp_avg.shape)} and {tuple(exp_avg_sq.shape)} elements, the layout {total}")
    steps = []
    for pos, shape, at in zip(positions, shapes, offsets):
        entry, n = state.get(pos), _numel(shape)
        for flat, key in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            if entry is None:
                flat[at:at + n].zero_()
                continue
            if tuple(entry[key].shape) != tuple(shape):
                raise ValueError(f"{key} of parameter {pos} is {tuple(entry[key].shape)}, the parameter {tuple(shape)}")
            flat[at:at + n].copy_(entry[key].detach().reshape(-1))
        step = 0 if entry is None else float(entry["step"])
        if step != int(step) or step < 0:
            raise ValueError(f"step of parameter {pos} is {step}")
        steps.append(int(step))
    return steps


def unpack_moments(exp_avg, exp_avg_sq, steps, positions, shapes):
    """The inverse: {position: {"step": float32 0-dim tensor, "exp_avg", "exp_avg_sq": views of the flat arrays in the
    parameter's shape}} for the slots that have stepped, the entries torch.optim.Adam keeps."""
    offsets, _ = segment_offsets([_numel(s) for s in shapes])
    out = {}
    for pos, shape, at, t in zip(positions, shapes, offsets, steps):
        if t > 0:
            n = _numel(shape)
            out[pos] = {"step": torch.tensor(float(t), dtype=torch.float32),
                        "exp_avg": exp_avg[at:at + n].view(tuple(shape)), "exp_avg_sq": exp_avg_sq[at:at + n].view(tuple(shape))}
    return out


def _numel(shape):
    n = 1
    for k in shape:
        n *= int(k)
    return n


# ---- the optimiser ------------------------------------------------------------------------------------------
def _check(params):
    """the refusals; returns the tensors that take a slot and their positions in the group"""
    if len(params) == 0:
        raise ValueError("NetworkAdam got an empty parameter list")
    if any(isinstance(p, dict) for p in params):
        raise ValueError("NetworkAdam takes ONE parameter group: an iterable of tensors, not of dicts")
    for i, p in enumerate(params):
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"parameter {i} must be a torch.Tensor, got {type(p).__name__}")
    positions = [i for i, p in enumerate(params) if p.requires_grad]
    slots = [params[i] for i in positions]
    if not slots:
        raise ValueError("no parameter requires grad")
    if len(slots) > MAX_TENSORS:
        raise ValueError(f"{len(slots)} tensors require grad: NetworkAdam takes at most {MAX_TENSORS}")
    if slots[0].dtype not in _DTYPES or any(p.dtype != slots[0].dtype for p in slots):
        raise TypeError(f"dtypes {sorted({str(p.dtype) for p in slots})}: float32 or float64, all alike")
    for i, p in zip(positions, slots):
        if not p.is_contiguous():
            raise ValueError(f"parameter {i} must be contiguous: it is updated in place")
        if p.numel() < 1:
            raise ValueError(f"parameter {i} is empty")
    for i, p in zip(positions, slots):
        if not p.is_cuda or p.device != slots[0].device:
            raise RuntimeError(f"parameter {i} is on {p.device}" + (f", parameter {positions[0]} on {slots[0].device}"
                               if p is not slots[0] else "") + ": the optimiser runs on one GPU (no CPU fallback)")
    return slots, positions


class NetworkAdam(torch.optim.Optimizer):
    """Adam over a network's parameters in two launches per step, with the loss-weighted rate on the device; see the
    module text.  A drop-in for ``torch.optim.Adam(model.parameters())`` in main_pn.py."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, capturable=False, weight_decay=0, amsgrad=False,
                 maximize=False):
        for name, value in (("weight_decay", weight_decay), ("amsgrad", amsgrad), ("maximize", maximize)):
            if value:
                raise NotImplementedError(f"{name} is not built")
        # torch's own group keys and its checks of lr, betas and eps: the state dict is then what torch.optim.Adam writes
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=float(lr), betas=tuple(float(b) for b in betas),
                                         eps=float(eps)).defaults, capturable=bool(capturable))
        params = list(params)
        slots, positions = _check(params)
        lib = _lib.load()
        self._entries = None                      # the state property answers from the plain dict until the arrays exist
        self._block = None                        # add_param_group is the constructor's alone
        super().__init__(params, defaults)
        self.capturable = bool(capturable)
        self.device, self.dtype = slots[0].device, slots[0].dtype
        self._slots, self._positions = slots, positions
        self._shapes = [tuple(p.shape) for p in slots]
        S = len(slots)
        _, total = segment_offsets([p.numel() for p in slots])
        self.exp_avg_flat = torch.zeros(total, dtype=self.dtype, device=self.device)
        self.exp_avg_sq_flat = torch.zeros(total, dtype=self.dtype, device=self.device)
        doubles = lib.pigs_network_adam_state_doubles(S)
        host = [1.0, 0.0, 0.0, 0.0] + [0.0] * S + [1.0] * (2 * S) + [0.0] * (2 * S)
        assert doubles == len(host)
        self._state_tensor = torch.tensor(host, dtype=torch.float64, device=self.device)
        self.rate_scale = self._state_tensor[0]
        self.lr_tensor = torch.tensor(float(lr), dtype=torch.float64, device=self.device) if self.capturable else None
        block = self._block = _lib.PigsNetworkAdam()
        block.tensors = S
        for s, p in enumerate(slots):
            block.counts[s] = p.numel()
            block.params[s] = p.data_ptr()
        views = unpack_moments(self.exp_avg_flat, self.exp_avg_sq_flat, [1] * S, range(S), self._shapes)
        self._entries = [views[s] for s in range(S)]

    def add_param_group(self, param_group):
        if self._block is not None:
            raise ValueError("NetworkAdam takes ONE parameter group, fixed at construction")
        super().add_param_group(param_group)

    # ---- state ------------------------------------------------------------------------------------------------
    @property
    def steps(self):
        """the step count of every tensor that takes a slot, in the parameters' order (a device read)"""
        return [int(t) for t in self._state_tensor[HEAD:HEAD + len(self._slots)].tolist()]

    @property
    def state(self):
        """torch's per-parameter state, assembled from the device (a device read): an entry for every stepped tensor"""
        if self._entries is None:
            return self._plain_state
        live = self._plain_state
        for p, entry, t in zip(self._slots, self._entries, self.steps):
            if t > 0:
                entry["step"].fill_(float(t))
                live[p] = entry
            else:
                live.pop(p, None)
        return live

    @state.setter
    def state(self, value):
        self._plain_state = value

    def reset_rate_scale(self):
        """rate_scale = 1 in place, the ``loss_weight = 1`` of main_pn.py:157 (one launch that a graph may hold)"""
        self.rate_scale.fill_(1.0)

    def loss_stats(self):
        """(sum, max, count) of the losses the steps were given since the last reset: one device read"""
        total, worst, count = self._state_tensor[1:HEAD].tolist()
        return total, worst, int(count)

    def reset_loss_stats(self):
        """zero the sum, the maximum and the count in place (one launch that a graph may hold)"""
        self._state_tensor[1:HEAD].zero_()

    def load_state_dict(self, state_dict):
        """a ``torch.optim.Adam`` (or NetworkAdam) state dict, with state for some, all or none of the parameters"""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"the state dict holds {len(groups)} parameter groups: NetworkAdam has one")
        saved, group = groups[0], self.param_groups[0]
        if len(saved["params"]) != len(group["params"]):
            raise ValueError(f"the state dict's group holds {len(saved['params'])} parameters, this optimiser's "
                             f"{len(group['params'])}")
        for name in ("weight_decay", "amsgrad", "maximize"):
            if saved.get(name):
                raise NotImplementedError(f"the state dict was written with {name} = {saved[name]}: {name} is not built")
        by_position = {i: state_dict["state"][key] for i, key in enumerate(saved["params"]) if key in state_dict["state"]}
        steps = pack_moments(by_position, self._positions, self._shapes, self.exp_avg_flat, self.exp_avg_sq_flat)
        for name in ("lr", "betas", "eps"):
            if name in saved:
                group[name] = saved[name]
        beta1, beta2 = (float(b) for b in group["betas"])
        host = [float(t) for t in steps] + running_products(beta1, steps) + running_products(beta2, steps)
        S = len(self._slots)
        self._state_tensor[HEAD:HEAD + 3 * S].copy_(torch.tensor(host, dtype=torch.float64))
        if self.capturable:
            self.lr_tensor.fill_(float(group["lr"]))

    # ---- the step ---------------------------------------------------------------------------------------------
    def step(self, loss=None, decay=0.0):
        """Two launches: the running products, the rate and the loss; then Adam on every tensor that has a gradient."""
        if loss is not None:
            if callable(loss) and not isinstance(loss, torch.Tensor):
                raise TypeError("NetworkAdam.step takes the loss as a tensor, not a closure")
            if (not isinstance(loss, torch.Tensor) or loss.numel() != 1 or loss.dtype not in _DTYPES
                    or loss.device != self.device):
                raise TypeError(f"loss must be one float32 / float64 element on {self.device}")
        dtype, device, block = self.dtype, self.device, self._block
        grads, present = block.grads, []
        for s, p in enumerate(self._slots):
            g = p.grad
            if g is None:
                grads[s] = None
                continue
            if (g.dtype != dtype or g.device != device or g.shape != p.shape or g.layout != torch.strided
                    or not g.is_contiguous()):
                raise TypeError(f"the gradient of parameter {self._positions[s]} is {g.dtype} {tuple(g.shape)} "
                                f"{'' if g.layout != torch.strided or g.is_contiguous() else 'non-contiguous '}"
                                f"({g.layout}) on {g.device}: it must be dense, contiguous and {dtype} {tuple(p.shape)} "
                                f"on {device}")
            grads[s] = g.data_ptr()
            present.append(p)
        if not present:
            return                # as torch.optim.Adam with no gradient anywhere: nothing moves, nothing is launched
        group = self.param_groups[0]
        block.lr = float(group["lr"])
        block.beta1, block.beta2 = group["betas"]
        block.eps = group["eps"]
        block.decay = float(decay)
        block.dev_lr = self.lr_tensor.data_ptr() if self.capturable else None
        lib = _lib.load()
        with torch.cuda.device(device):
            rc = lib.pigs_network_adam_step(_DTYPES[dtype], ctypes.byref(block), self._state_tensor.data_ptr(),
                                            self.exp_avg_flat.data_ptr(), self.exp_avg_sq_flat.data_ptr(),
                                            loss.data_ptr() if loss is not None else None,
                                            _DTYPES[loss.dtype] if loss is not None else 0, _stream(device))
        _lib.check(rc, "pigs_network_adam_step")
        # the writes went through raw pointers: a stale autograd node must complain as it would after torch.optim
        torch.autograd.graph.increment_version(present)
        for p in present:
            p.grad = None
