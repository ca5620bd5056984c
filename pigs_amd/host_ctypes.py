"""The ctypes host of the sampler: the plans, the raw launches, the autograd nodes and, at the end, ``SamplerCore`` --
the logic of the native core ``_pigs_host.SamplerCore`` (csrc_host/pigs_host.cpp) in Python, with the same constructor
and the same public names: the interface ``GaussianSampler`` (pigs_amd/sampler.py) drives, whichever core it holds.
"""
import ctypes
import threading

import torch

from . import _lib, aggregate
from ._lib import DTYPES as _DTYPES, ptr as _ptr, stream as _stream

TRACE = 4       # order index of the Hessian's trace (mask bit 16); it travels in pointer slot 2
# the columns of GaussianSampler.vorticity_terms(): the field, its divergence, the vorticity w = d_x u_y - d_y u_x,
# its gradient and its Laplacian
VORTICITY_COLUMNS = ("u_x", "u_y", "div", "w", "w_x", "w_y", "lap_w")
# the columns of GaussianSampler.vorticity_residual(): the blended divergence and the vorticity equation's residual
VORTICITY_RESIDUAL_COLUMNS = ("div", "r")
# the columns of GaussianSampler.vorticity_residual(data=...): the same two and the weighted data term
VORTICITY_FIT_COLUMNS = ("div", "r", "fit")
# the right-hand sides of GaussianSampler.network_inputs(), in the order of the C ABI's PIGS_NET_* codes
NETWORK_PDES = ("zero", "diffusion", "burgers", "wave", "navier_stokes")
_NET_WAVE, _NET_NAVIER_STOKES = NETWORK_PDES.index("wave"), NETWORK_PDES.index("navier_stokes")


def network_pde_width(kind, c):
    """Columns of sample_pde: two for the wave system, one for the vorticity equation, else the channels."""
    return 2 if kind == _NET_WAVE else 1 if kind == _NET_NAVIER_STOKES else c


def _out_shape(order, M, d, c):
    return (M, c) if order == TRACE else (M,) + (d,) * order + (c,)


class _on_device:
    """``torch.cuda.device(dev)`` only when ``dev`` is not already current (the context manager
    costs microseconds, which matters for the launch-bound problem sizes of the PINN loops)."""

    def __init__(self, device):
        self.ctx = None if torch.cuda.current_device() == device.index else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


_WORKSPACE_BYTES = {}


def _mask_orders(mask):
    return [k for k in range(5) if mask >> k & 1]


def _slot2(ts):
    """Pointer slot 2 of the C ABI: the full Hessian, or its trace when that is what the mask asks for."""
    return ts[2] if ts[2] is not None else ts[TRACE]


def _error_flag(workspace, offset):
    return int(workspace[offset:offset + 4].view(torch.int32).item())


class SamplePlan:
    """The samples half of what ``preprocess`` builds (C ABI: pigs_samples_*): the sample points
    sorted into 16-point cells.  A function of ``samples`` alone and immutable once built, so one
    object serves every ``preprocess`` that is handed the same, unmodified samples tensor again --
    the reference's roll-out (main_pn.py:317-324) and any fixed collocation grid."""

    __slots__ = ("workspace", "M", "source", "points", "version", "built")

    def __init__(self, samples, source=None):
        lib = _lib.load()
        self.M = samples.shape[0]
        nbytes = _WORKSPACE_BYTES.get(("s", self.M))
        if nbytes is None:
            nbytes = _WORKSPACE_BYTES[("s", self.M)] = lib.pigs_samples_workspace_bytes(self.M)
        if nbytes == 0:
            raise _lib.PigsError(f"binned path does not support M={self.M}")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=samples.device)
        # what this plan was built from: the caller's tensor (kept alive, so its address cannot be
        # handed to another tensor) and its version counter at build time
        self.source = source if source is not None else samples
        # the contiguous array the build reads: in index-tiled order (include/pigs_amd.h, ABI 7) the workspace holds no
        # copy of the points -- the sampling kernels read THIS array, so it lives as long as the workspace
        self.points = samples
        self.version = self.source._version
        self.built = False

    def matches(self, source):
        return (source is self.source or (
            source.data_ptr() == self.source.data_ptr() and source.shape == self.source.shape
            and source.stride() == self.source.stride() and source.dtype == self.source.dtype
            and source.device == self.source.device)) and source._version == self.version

    def scan_took_slow_path(self):
        """Diagnostic (synchronises): a workgroup of the build's scan recomputed a predecessor's total
        itself instead of receiving it (include/pigs_amd.h: the result is valid either way)."""
        return bool(_error_flag(self.workspace, _lib.load().pigs_samples_error_offset()))


class _PlanPool:
    """Plan workspaces whose plan has died, kept for the next ``preprocess`` of the same sizes on the
    same stream: a build leaves its workspace's counters zeroed, so a build INTO such a workspace
    skips the zeroing launch (PIGS_BUILD_PLAN_WS_CLEAN).  A workspace is only ever handed out again
    after its plan object is gone (no autograd node can still read it) and only to the stream its
    last build ran on (stream order then covers kernels that may still be in flight)."""

    KEEP = 2           # per key (sizes, device, stream)
    KEEP_TOTAL = 4     # over all keys: problem sizes that change from step to step must not pile up workspaces

    def __init__(self):
        self.free = {}             # key -> [workspace, ...]; dict order = least recently given first
        # plans die wherever their last reference is dropped -- the autograd engine's worker threads and
        # the garbage collector included -- while the main thread may be inside take()
        # (re-entrant: give() allocates while it holds the lock, a collector pass triggered there can finalise a
        # Plan in a reference cycle, whose __del__ comes back into give() on the same thread)
        self.lock = threading.RLock()

    def take(self, key):
        with self.lock:
            lst = self.free.get(key)
            if not lst:
                return None
            ws = lst.pop()
            if not lst:
                self.free.pop(key, None)
            return ws

    def give(self, key, workspace):
        with self.lock:
            lst = self.free.pop(key, [])
            if len(lst) < self.KEEP:
                lst.append(workspace)
            self.free[key] = lst       # most recently given last
            while sum(len(v) for v in self.free.values()) > self.KEEP_TOTAL:
                oldest = next(iter(self.free))
                self.free[oldest].pop(0)
                if not self.free[oldest]:
                    del self.free[oldest]


class Plan:
    """The Gaussian half of what ``preprocess`` builds (C ABI: pigs_plan_*): the Gaussians binned
    into the multi-level grid and the per-tile lists, on top of a :class:`SamplePlan`.  Immutable
    once built; autograd nodes keep a reference, so later ``preprocess`` calls never disturb a
    pending backward."""

    __slots__ = ("workspace", "samples", "N", "M", "c", "q_max", "q_max_backward", "_pool", "_pool_key",
                 "build_stream", "other_stream_used", "recorded_only", "forward_only", "_full")

    # pigs_amd.h: PIGS_BUILD_SAMPLES, _PLAN_WS_CLEAN, _DEFER_LISTS, _FORWARD_ONLY
    BUILD_SAMPLES, WS_CLEAN, DEFER_LISTS, FORWARD_ONLY = 1, 2, 32, 64

    def __init__(self, means, values, conics, samples, q_max, sample_plan=None, source=None, pool=None,
                 recorded_only=False, q_max_backward=None, defer_lists=False, forward_only=False):
        lib = _lib.load()
        self.N, self.M, self.c, self.q_max = means.shape[0], samples.shape[0], values.shape[1], float(q_max)
        self.q_max_backward = max(self.q_max, float(q_max_backward if q_max_backward is not None else q_max))
        self._pool = None
        self.other_stream_used = False
        self.recorded_only = bool(recorded_only)      # built inside a capture: has run only if that graph was replayed
        # no backward can follow (PIGS_BUILD_FORWARD_ONLY): group lists under the one cut-off q_max, no tile lists
        self.forward_only = bool(forward_only) and not defer_lists
        self._full = None
        key = (self.N, self.M, self.c)
        nbytes = _WORKSPACE_BYTES.get(key)
        if nbytes is None:
            nbytes = _WORKSPACE_BYTES[key] = lib.pigs_plan_workspace_bytes(self.N, self.M, self.c)
        if nbytes == 0:
            raise _lib.PigsError(f"binned path does not support N={self.N} M={self.M} c={self.c}")
        if sample_plan is None:
            sample_plan = SamplePlan(samples, source)
        self.samples = sample_plan
        with _on_device(means.device):
            stream = _stream(means.device)
            self.build_stream = stream.value
            self._pool_key = (self.N, self.M, self.c, means.device, stream.value)
            self.workspace = pool.take(self._pool_key) if pool is not None else None
            flags = 0 if sample_plan.built else self.BUILD_SAMPLES
            if defer_lists:       # the tile lists are built by the plan's first sampling call, a forward in the same launch
                flags |= self.DEFER_LISTS
            if self.forward_only:
                flags |= self.FORWARD_ONLY
            if self.workspace is not None:
                flags |= self.WS_CLEAN
            else:
                self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=means.device)
            sws = sample_plan.workspace
            rc = lib.pigs_plan_build(_ptr(self.workspace), nbytes, _ptr(sws), sws.numel(),
                                     flags, self.N, self.M, self.c, self.q_max, self.q_max_backward,
                                     _ptr(means), _ptr(conics), _ptr(values), _ptr(samples), stream)
        _lib.check(rc, "pigs_plan_build")
        # a build that was only RECORDED into a hipGraph has not run: nothing eager may rely on it -- and a
        # SamplePlan that WAS built eagerly stays built whatever is recorded on top of it (lowering the flag
        # would make the next eager preprocess re-sort a workspace older plans still hold tile lists for)
        sample_plan.built = sample_plan.built or not recorded_only
        self._pool = pool            # only a workspace whose build was launched completely goes back

    def note_stream(self, stream_value):
        """A launch on another stream than the build's reads the workspace: stream order no longer
        covers its reuse, so it does not go back to the pool -- and the caching allocator, which hands a freed
        block out again in the order of its allocation stream, is told about the other stream."""
        if stream_value != self.build_stream:
            self.other_stream_used = True
            st = torch.cuda.current_stream(self.workspace.device)
            if st.cuda_stream == stream_value:
                self.workspace.record_stream(st)
                self.samples.workspace.record_stream(st)

    def __del__(self):
        try:
            if self._pool is not None and not self.other_stream_used:
                self._pool.give(self._pool_key, self.workspace)
        except Exception:            # interpreter shutdown: nothing to keep
            pass

    def full_for_backward(self, means, values, conics, samples):
        """A raw backward (:func:`backward_raw`: tools, bench) on a forward-only plan runs on a full plan of the same
        inputs and samples half, built on the first such call and kept with this one."""
        if not self.forward_only:
            return self
        if self._full is None:
            with torch.no_grad():
                self._full = Plan(means.detach(), values.detach(), conics.detach(), samples, self.q_max, self.samples,
                                  q_max_backward=self.q_max_backward)
        return self._full

    def scan_took_slow_path(self):
        """Diagnostic (synchronises): see :meth:`SamplePlan.scan_took_slow_path`."""
        return self.samples.scan_took_slow_path() or bool(
            _error_flag(self.workspace, _lib.load().pigs_plan_error_offset()))

    @staticmethod
    def supported(means, values, samples):
        return (means.dtype == torch.float32 and means.shape[1] == 2 and 1 <= values.shape[1] <= 2
                and means.shape[0] >= 1 and samples.shape[0] >= 1)


def forward_raw(means, values, conics, samples, mask, plan=None):
    """Launch the forward for the orders in ``mask`` on contiguous device tensors (through the
    plan when given, else dense).  Returns a list of 5 entries (tensor or None): orders 0..3 and the
    Hessian's trace."""
    lib = _lib.load()
    N, d = means.shape
    c = values.shape[1]
    M = samples.shape[0]
    outs = [None] * 5
    for k in _mask_orders(mask):
        outs[k] = torch.empty(_out_shape(k, M, d, c), dtype=means.dtype, device=means.device)
    if M > 0:
        with _on_device(means.device):
            if plan is not None:
                sws = plan.samples.workspace
                if hasattr(plan, "note_stream"):
                    plan.note_stream(_stream(means.device).value)
                rc = lib.pigs_plan_forward(_ptr(plan.workspace), plan.workspace.numel(), _ptr(sws), sws.numel(),
                                           N, M, c, plan.q_max, mask,
                                           _ptr(outs[0]), _ptr(outs[1]), _ptr(_slot2(outs)), _ptr(outs[3]),
                                           _stream(means.device))
                _lib.check(rc, "pigs_plan_forward")
            else:
                rc = lib.pigs_sample_forward(_DTYPES[means.dtype], d, c, mask, N, M, _ptr(means), _ptr(conics),
                                             _ptr(values), _ptr(samples), _ptr(outs[0]), _ptr(outs[1]),
                                             _ptr(_slot2(outs)), _ptr(outs[3]), _stream(means.device))
                _lib.check(rc, "pigs_sample_forward")
    return outs


def _gradient_views(means, values, conics):
    """The three parameter gradients as views of ONE flat allocation [means | values | conics]: the multi-GPU path
    (pigs_amd/distributed.py) all-reduces that buffer in place -- no packing copy in front of the collective, no
    slicing behind it."""
    nm, nv, nc = means.numel(), values.numel(), conics.numel()
    flat = torch.empty(nm + nv + nc, dtype=means.dtype, device=means.device)
    return flat[:nm].view(means.shape), flat[nm:nm + nv].view(values.shape), flat[nm + nv:].view(conics.shape)


def periodic_images_raw(means, values, conics, lo, period, q_cut, flag=None):
    """pigs_periodic_images on contiguous device tensors [N, 2], [N, c], [N, 3]: the image arrays [9N, 2], [9N, c],
    [9N, 3] (image j of Gaussian n in row j*N + n; include/pigs_amd.h, ABI 10).  ``flag``: None or a zeroed int32
    tensor of one element that the launch sets when a Gaussian's cut-off ellipse reaches one period."""
    lib = _lib.load()
    N, c = means.shape[0], values.shape[1]
    img_m = torch.empty((9 * N, 2), dtype=means.dtype, device=means.device)
    img_v = torch.empty((9 * N, c), dtype=means.dtype, device=means.device)
    img_c = torch.empty((9 * N, 3), dtype=means.dtype, device=means.device)
    with _on_device(means.device):
        rc = lib.pigs_periodic_images(_DTYPES[means.dtype], c, N, lo, period, q_cut, _ptr(means), _ptr(conics),
                                      _ptr(values), _ptr(img_m), _ptr(img_c), _ptr(img_v), _ptr(flag),
                                      _stream(means.device))
    _lib.check(rc, "pigs_periodic_images")
    return img_m, img_v, img_c


def periodic_fold_raw(g_img_means, g_img_values, g_img_conics, N, c, dtype, device):
    """pigs_periodic_images_backward: the gradients [N, 2], [N, c], [N, 3] of the originals, g[n] = sum over the nine
    images (None reads as zero), as views of ONE flat allocation like every gradient of the sampler
    (:func:`_gradient_views`)."""
    lib = _lib.load()
    flat = torch.empty(N * (5 + c), dtype=dtype, device=device)
    g_means, g_values, g_conics = flat[:2 * N].view(N, 2), flat[2 * N:(2 + c) * N].view(N, c), flat[(2 + c) * N:].view(N, 3)
    with _on_device(device):
        rc = lib.pigs_periodic_images_backward(_DTYPES[dtype], c, N, _ptr(g_img_means), _ptr(g_img_conics),
                                               _ptr(g_img_values), _ptr(g_means), _ptr(g_conics), _ptr(g_values),
                                               _stream(device))
    _lib.check(rc, "pigs_periodic_images_backward")
    return g_means, g_values, g_conics


class _PeriodicImages(torch.autograd.Function):
    """The 3 x 3 images of every Gaussian on the torus (one launch); the backward folds the image gradients back onto
    the originals (one launch, no atomics).  The fold reads nothing but the incoming gradients: the node keeps no
    tensors."""

    @staticmethod
    def forward(ctx, means, values, conics, lo, period, q_cut, flag):
        ctx.sizes = (means.shape[0], values.shape[1], means.dtype, means.device)
        ctx.set_materialize_grads(False)
        return periodic_images_raw(means, values, conics, lo, period, q_cut, flag)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_means, g_values, g_conics):
        if g_means is None and g_values is None and g_conics is None:
            return None, None, None, None, None, None, None
        gs = [None if g is None else g.contiguous() for g in (g_means, g_values, g_conics)]
        gm, gv, gc = periodic_fold_raw(*gs, *ctx.sizes)
        return gm, gv, gc, None, None, None, None


def backward_raw(means, values, conics, samples, gouts, mask, plan=None):
    """Launch the backward; ``gouts`` has 5 entries (contiguous tensor or None: orders 0..3 and the
    trace), ``mask`` marks the non-None ones.  Returns (g_means, g_values, g_conics)."""
    lib = _lib.load()
    N, d = means.shape
    c = values.shape[1]
    M = samples.shape[0]
    g_means, g_values, g_conics = _gradient_views(means, values, conics)
    if plan is not None and M > 0 and getattr(plan, "forward_only", False):
        plan = plan.full_for_backward(means, values, conics, samples)
    if N > 0:
        with _on_device(means.device):
            if plan is not None and M > 0:
                sws = plan.samples.workspace
                if hasattr(plan, "note_stream"):
                    plan.note_stream(_stream(means.device).value)
                rc = lib.pigs_plan_backward(_ptr(plan.workspace), plan.workspace.numel(), _ptr(sws), sws.numel(),
                                            N, M, c, plan.q_max, mask,
                                            _ptr(gouts[0]), _ptr(gouts[1]), _ptr(_slot2(gouts)),
                                            _ptr(gouts[3]), _ptr(g_means), _ptr(g_conics), _ptr(g_values),
                                            _stream(means.device))
                _lib.check(rc, "pigs_plan_backward")
            else:
                rc = lib.pigs_sample_backward(_DTYPES[means.dtype], d, c, mask, N, M, _ptr(means), _ptr(conics),
                                              _ptr(values), _ptr(samples), _ptr(gouts[0]), _ptr(gouts[1]),
                                              _ptr(_slot2(gouts)), _ptr(gouts[3]), _ptr(g_means), _ptr(g_conics),
                                              _ptr(g_values), _stream(means.device))
                _lib.check(rc, "pigs_sample_backward")
    return g_means, g_values, g_conics


class _FusedOp:
    """What tells the fused outputs -- residual() in its three forms, vorticity_terms(), vorticity_residual() -- apart
    between the Python call and their pair of C entry points: ``label`` names the call in messages, ``entry`` the pair
    (``<entry>_forward`` / ``<entry>_backward``), ``width`` the output's columns (None: the channels), ``dims`` whether
    the entry points take d and c, ``has_params`` a coefficient block (an object with ``struct()``), ``has_side`` the
    forward's constant input (a residual's target, the previous level of the vorticity residual), ``has_target`` that
    this input is a target (differentiable: its gradient is ``-gout``), ``aux_shape`` the record that the forward
    leaves for the backward, a function of (params, M, d, c) that returns None where these parameters need none."""

    def __init__(self, label, entry, width=None, dims=True, has_params=True, has_side=True, has_target=True, aux_shape=None):
        self.label, self.width, self.dims = label, width, dims
        self.forward_name, self.backward_name = entry + "_forward", entry + "_backward"
        self.has_params, self.has_side, self.has_target, self.aux_shape = has_params, has_side, has_target, aux_shape


def _fused_call(op, backward, means, values, conics, samples, params, plan, side=None, gout=None, aux=None):
    """The forward or backward entry point of the fused output ``op`` on contiguous device tensors (through the plan
    when given).  Returns the output, or (g_means, g_values, g_conics)."""
    lib = _lib.load()
    N, d = means.shape
    c = values.shape[1]
    M = samples.shape[0]
    if backward and plan is not None and M > 0 and getattr(plan, "forward_only", False):
        plan = plan.full_for_backward(means, values, conics, samples)
    pw = (_ptr(plan.workspace), plan.workspace.numel(), _ptr(plan.samples.workspace), plan.samples.workspace.numel()) \
        if plan is not None else (ctypes.c_void_p(0), 0, ctypes.c_void_p(0), 0)
    args = [_DTYPES[means.dtype], d, c, N, M] if op.dims else [_DTYPES[means.dtype], N, M]
    args += [_ptr(means), _ptr(conics), _ptr(values), _ptr(samples)]
    if op.has_params:
        args.append(params.struct())
    with _on_device(means.device):
        stream = _stream(means.device)
        if plan is not None and hasattr(plan, "note_stream"):
            plan.note_stream(stream.value)
        if not backward:
            out = torch.empty((M, c if op.width is None else op.width), dtype=means.dtype, device=means.device)
            if M > 0:
                if op.has_side:
                    args.append(_ptr(side))
                args.append(_ptr(out))
                if op.aux_shape is not None:
                    args.append(_ptr(aux))
                _lib.check(getattr(lib, op.forward_name)(*args, *pw, stream), op.forward_name)
            return out
        g_means, g_values, g_conics = _gradient_views(means, values, conics)
        if N > 0:
            if M > 0:
                args.append(_ptr(gout))
                if op.aux_shape is not None:
                    args.append(_ptr(aux))
                rc = getattr(lib, op.backward_name)(*args, _ptr(g_means), _ptr(g_conics), _ptr(g_values), *pw, stream)
                _lib.check(rc, op.backward_name)
            else:
                for g in (g_means, g_values, g_conics):
                    g.zero_()
        return g_means, g_values, g_conics


class _FusedFunction(torch.autograd.Function):
    """One fused output in one launch; its backward is one launch too.  The node owns its inputs and plan like
    :class:`_SampleFunction`, and with them the coefficient block ``params`` (its fields), the constant ``side`` and the
    record ``aux`` of the forward where the backward reads one.  The subclasses carry their :class:`_FusedOp` alone."""
    op = None

    @classmethod
    def forward(cls, ctx, means, values, conics, samples, side, params, debug, plan, want_aux):
        op = cls.op
        target_dtype = side.dtype if op.has_target and side is not None else None
        if target_dtype is not None:
            side = side.detach().to(means.dtype).contiguous()
        M = samples.shape[0]
        shape = op.aux_shape(params, M, means.shape[1], values.shape[1]) if want_aux and M > 0 else None
        aux = None if shape is None else torch.empty(shape, dtype=means.dtype, device=means.device)
        out = _fused_call(op, False, means, values, conics, samples, params, plan, side=side, aux=aux)
        if debug:
            torch.cuda.synchronize(means.device)
        ctx.inputs = (means, values, conics, samples)
        ctx.versions = (means._version, values._version, conics._version, samples._version)
        ctx.params, ctx.aux, ctx.debug, ctx.plan, ctx.target_dtype = params, aux, debug, plan, target_dtype
        ctx.side = None if op.has_target else side
        return out

    @classmethod
    @torch.autograd.function.once_differentiable
    def backward(cls, ctx, gout):
        op = cls.op
        means, values, conics, samples = ctx.inputs
        if (means._version, values._version, conics._version, samples._version) != ctx.versions:
            raise RuntimeError("one of the tensors handed to GaussianSampler.preprocess() has been modified in place "
                               f"before the backward of a {op.label} output that was computed from it")
        M = samples.shape[0]
        if (op.aux_shape is not None and ctx.aux is None and M > 0
                and op.aux_shape(ctx.params, M, means.shape[1], values.shape[1]) is not None):
            raise RuntimeError(f"this {op.label} output was computed without the record its backward needs "
                               "(no input required grad when it ran)")
        gout = gout.contiguous()
        if ctx.debug:
            assert ctx.plan is None or not ctx.plan.forward_only, f"a {op.label} node holds a forward-only plan"
        g_means, g_values, g_conics = _fused_call(op, True, means, values, conics, samples, ctx.params, ctx.plan,
                                                  gout=gout, aux=ctx.aux)
        if ctx.debug:
            torch.cuda.synchronize(means.device)
        g_target = None if ctx.target_dtype is None or not ctx.needs_input_grad[4] else (-gout).to(ctx.target_dtype)
        return g_means, g_values, g_conics, None, g_target, None, None, None, None


class ResidualCoeffs:
    """The coefficients of a linear residual() call: the four floats a0, a1x, a1y, aL."""

    def __init__(self, coeffs):
        self.coeffs = coeffs

    def struct(self):
        return (ctypes.c_double * 4)(*self.coeffs)


class ResidualTerms:
    """The coefficients of a general residual() call as the cores take them: ``fields`` = a0 [M], a1 [M, d], aL [M],
    adv [M] as detached device tensors or None, ``consts`` = a0, a1x, a1y, aL, adv where there is no field, and the
    constants ``advect_by`` flat as [2][4].  ``advects``: the advection term is active."""

    def __init__(self, fields, consts, advect_by):
        self.fields, self.consts, self.advect_by = fields, consts, advect_by
        self.advects = fields[3] is not None or consts[4] != 0.0

    def struct(self):
        a0, a1x, a1y, aL, adv = self.consts
        by = tuple(tuple(self.advect_by[4 * i:4 * i + 4]) for i in range(2))
        return _lib.PigsResidualTerms(a0, (a1x, a1y), aL, adv, by, *(v if v is None else v.data_ptr() for v in self.fields))


class ResidualCoupling:
    """The coefficients of a coupled residual() call as the cores take them: ``fields`` = a0, aL, cw [M] as detached
    device tensors or None, ``consts`` = the same three where there is no field, and the two constant matrices flat as
    [4][4] (row = output channel, column = input channel)."""

    def __init__(self, fields, consts, couple0, couple_lap):
        self.fields, self.consts, self.couple0, self.couple_lap = fields, consts, couple0, couple_lap

    def struct(self):
        q0, qL = (tuple(tuple(q[4 * i:4 * i + 4]) for i in range(4)) for q in (self.couple0, self.couple_lap))
        return _lib.PigsResidualCoupling(*self.consts, q0, qL, *(v if v is None else v.data_ptr() for v in self.fields))


class VorticityResidual:
    """The coefficients of a vorticity_residual() call: three floats and ``tau``, a float or a detached device field
    [M, 1]."""

    def __init__(self, nu, dt, time_term, tau):
        self.nu, self.dt, self.time_term, self.tau = nu, dt, time_term, tau

    def struct(self):
        field = isinstance(self.tau, torch.Tensor)
        return _lib.PigsVorticityResidual(self.nu, self.dt, self.time_term, 0.0 if field else self.tau,
                                          self.tau.data_ptr() if field else None)


class VorticityFit(VorticityResidual):
    """The coefficients of a vorticity_residual(data=...) call: those of :class:`VorticityResidual`, the detached device
    array ``data`` [M] (which the node so keeps alive; only the forward reads it) and its weight."""

    def __init__(self, nu, dt, time_term, tau, data, data_weight):
        super().__init__(nu, dt, time_term, tau)
        self.data, self.data_weight = data, data_weight

    def struct(self):
        field = isinstance(self.tau, torch.Tensor)
        return _lib.PigsVorticityFit(self.nu, self.dt, self.time_term, 0.0 if field else self.tau, self.data_weight,
                                     self.tau.data_ptr() if field else None, self.data.data_ptr())


class _ResidualFunction(_FusedFunction):
    """r = a0 u + a1 . grad u + aL lap u - target."""
    op = _FusedOp("residual()", "pigs_residual")


class _ResidualTermsFunction(_FusedFunction):
    """The general residual (per-point coefficients, advection term); ``aux`` = u and grad u of the forward, which the
    backward of the advection term reads (kept only when that term is active)."""
    op = _FusedOp("residual()", "pigs_residual_terms",
                  aux_shape=lambda terms, M, d, c: (M, 1 + d, c) if terms.advects else None)


class _ResidualCoupledFunction(_FusedFunction):
    """The coupled residual (two constant matrices mix the channels under a per-point weight): linear in the field, so
    no record of the forward is kept."""
    op = _FusedOp("residual()", "pigs_residual_coupled")


class _VorticityFunction(_FusedFunction):
    """(u_x, u_y, div, w, w_x, w_y, lap w) as [M, 7]."""
    op = _FusedOp("vorticity_terms()", "pigs_vorticity", width=len(VORTICITY_COLUMNS), dims=False, has_params=False,
                  has_side=False, has_target=False)


class _VorticityResidualFunction(_FusedFunction):
    """(div_b, r) of the Navier-Stokes residual as [M, 2]; ``side`` = the previous level's vorticity terms (a constant),
    ``aux`` = the blended u and grad w of the forward, which the backward of the advection term reads."""
    op = _FusedOp("vorticity_residual()", "pigs_vorticity_residual", width=len(VORTICITY_RESIDUAL_COLUMNS), dims=False,
                  has_target=False, aux_shape=lambda params, M, d, c: (M, 4))


class _VorticityFitFunction(_FusedFunction):
    """(div_b, r, data_weight (w - data)) as [M, 3]: the vorticity residual with the data term from the same sums;
    ``side`` and ``aux`` as there, the data travels in ``params``."""
    op = _FusedOp("vorticity_residual()", "pigs_vorticity_fit", width=len(VORTICITY_FIT_COLUMNS), dims=False,
                  has_target=False, aux_shape=lambda params, M, d, c: (M, 4))


class _SampleFunction(torch.autograd.Function):
    """One fused launch producing the outputs of every order in ``mask``; its backward is one
    fused launch over the outputs that received a gradient.

    The reference's scripts treat the outputs of the separate ``sample_*`` calls as independent graphs:
    they differentiate one component after the other, some calls with ``retain_graph=True`` and the
    last one on an output without (test_derivatives.py:214-215), and come back to another output of
    the same ``preprocess`` later (test_derivatives.py:349-352).  Outputs that were computed by ONE
    fused launch share this node, so the node must survive a backward that does not retain the graph:
    the inputs are therefore kept on the node itself rather than through ``save_for_backward`` (whose
    storage autograd releases after the first such backward), with the version check that
    ``save_for_backward`` would have done repeated by hand."""

    @staticmethod
    def forward(ctx, means, values, conics, samples, mask, debug, plan):
        outs = forward_raw(means, values, conics, samples, mask, plan)
        if debug:
            torch.cuda.synchronize(means.device)
        ctx.inputs = (means, values, conics, samples)
        ctx.versions = (means._version, values._version, conics._version, samples._version)
        ctx.mask = mask
        ctx.debug = debug
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        return tuple(outs[k] for k in _mask_orders(mask))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_outputs):
        means, values, conics, samples = ctx.inputs
        if (means._version, values._version, conics._version, samples._version) != ctx.versions:
            raise RuntimeError("one of the tensors handed to GaussianSampler.preprocess() has been modified in place "
                               "before the backward of a sample_*() output that was computed from it")
        gouts = [None] * 5
        mask = 0
        for k, g in zip(_mask_orders(ctx.mask), grad_outputs):
            if g is not None:
                gouts[k] = g.contiguous()
                mask |= 1 << k
        if mask == 0:
            return None, None, None, None, None, None, None
        if ctx.debug:
            assert ctx.plan is None or not ctx.plan.forward_only, "a sample_*() node holds a forward-only plan"
        g_means, g_values, g_conics = backward_raw(means, values, conics, samples, gouts, mask, ctx.plan)
        if ctx.debug:
            torch.cuda.synchronize(means.device)
        return g_means, g_values, g_conics, None, None, None, None


def _check_periodic_flag(flag, box, q_cut):
    if flag:
        lo, hi = box
        raise ValueError(f"periodic=({lo}, {hi}): a Gaussian's cut-off ellipse (q <= {q_cut}) spans one period "
                         f"L = {hi - lo} or more on an axis (sqrt(q_cut Sigma_ii) >= L), or its conic is not positive "
                         "definite, or its mean is not finite: the 3 x 3 images do not give the periodic field")


_AUTO, _FUSE_ALL, _BACKEND_BINNED = 0, 1, 2      # sampler.py: _FUSE_CODES, _BACKEND_CODES


class SamplerCore:
    """The state and the policy of one sampler on the ctypes host: constructor, methods and public attributes are those
    of ``_pigs_host.SamplerCore``, name for name (tests/test_host_cpu.py); everything else carries an underscore."""

    _warned_samples_grad = False

    def __init__(self, debug, fuse, backend, q_max, q_max_order3, q_max_backward, reuse_samples):
        from .sampler import GaussianSampler as public      # the two thresholds of the ``auto`` rules live there
        self._fuse_auto_max_points, self._binned_auto_min_pairs = public.FUSE_AUTO_MAX_POINTS, public.BINNED_AUTO_MIN_PAIRS
        self._debug, self._fuse, self._backend, self._reuse_samples = debug, fuse, backend, reuse_samples
        self._q_max, self._q_max_order3, self._q_max_backward = q_max, q_max_order3, q_max_backward
        self._q_cut = max(q_max, q_max_backward, q_max_order3)      # the widest cut-off any launch samples with
        self.defer_lists = self.static_samples = self.periodic_aggregate = False
        self.periodic = None                 # the box (lo, hi), or None; the next preprocess uses it
        self.neighbors = self.plan = self.plan3 = None
        self.sample_plans = []               # most recently used first, at most ``reuse_samples``
        self._inputs = self._samples_source = None
        self._caller = self._box = None      # the caller's N Gaussians and the box that the bound images were made with
        self._pool = _PlanPool()
        self._cache = {}
        self._vorticity = None               # the cached vorticity_terms() of the bound inputs

    @property
    def pool_size(self):
        with self._pool.lock:
            return sum(len(v) for v in self._pool.free.values())

    def inputs(self):
        return self._inputs

    def cached_orders(self):
        return sorted(self._cache)

    # ------------------------------------------------------------------ preprocess
    def preprocess(self, means, values, covariances, conics, samples):
        if means.dim() != 2:
            raise ValueError(f"means must be [N, d], got {tuple(means.shape)}")
        N, d = means.shape
        if d not in (1, 2):
            raise NotImplementedError(f"d = {d} is not supported (d in {{1, 2}})")
        nf = d * (d + 1) // 2
        for name, t in (("means", means), ("values", values), ("conics", conics), ("samples", samples)):
            if not t.is_cuda:
                raise RuntimeError(f"{name} is on {t.device}: GaussianSampler runs on the GPU only (no CPU fallback)")
            if t.device != means.device:
                raise RuntimeError(f"{name} is on {t.device}, means on {means.device}")
            if t.dtype != means.dtype:
                raise TypeError(f"{name} has dtype {t.dtype}, means {means.dtype}")
        if means.dtype not in _DTYPES:
            raise TypeError(f"dtype {means.dtype} is not supported (float32 / float64)")
        if values.dim() == 1:
            values = values.reshape(N, 1)
        if values.dim() != 2 or values.shape[0] != N:
            raise ValueError(f"values must be [N, c], got {tuple(values.shape)}")
        c = values.shape[1]
        if not 1 <= c <= 4:
            raise NotImplementedError(f"c = {c} channels is not supported (1..4)")
        if conics.numel() != N * nf:
            raise ValueError(f"conics must hold N*{nf} elements (flat upper triangle), got {tuple(conics.shape)}")
        conics = conics.reshape(N, nf)
        if covariances is not None and isinstance(covariances, torch.Tensor) and covariances.numel() != N * nf:
            raise ValueError(f"covariances must hold N*{nf} elements, got {tuple(covariances.shape)}")
        if samples.dim() == 1 and d == 1:
            samples = samples.reshape(-1, 1)
        if samples.dim() != 2 or samples.shape[1] != d:
            raise ValueError(f"samples must be [M, {d}], got {tuple(samples.shape)}")
        # no gradient flows to the sample points (the reference requests none from the sampler:
        # test_derivatives.py:123 asks for (means, values, conics) only)
        if samples.requires_grad and torch.is_grad_enabled() and not SamplerCore._warned_samples_grad:
            SamplerCore._warned_samples_grad = True
            import warnings
            warnings.warn("GaussianSampler: samples.requires_grad is set, but the sampler returns no gradient "
                          "with respect to the sample points (as the reference, whose tests ask for the gradients "
                          "of means, values and conics only); use the derivative outputs instead", stacklevel=3)
        means, values, conics = means.contiguous(), values.contiguous(), conics.contiguous()
        self._caller = (means, conics)
        self._box = self.periodic
        if self.periodic is not None:
            self._inputs = None          # a preprocess that raises leaves nothing bound
            if d != 2:
                raise NotImplementedError("periodic=(lo, hi) is implemented for d = 2")
            means, values, conics = self._periodic_images(means, values, conics)
        self._inputs = (means, values, conics, samples.detach().contiguous())
        self._samples_source = samples
        self._cache = {}
        self._vorticity = None
        self.plan = self.plan3 = self.neighbors = None
        mc, vc, cc, sc = self._inputs
        # the pairs the launches will evaluate: with periodic=... the bound rows are the 9N images
        use_plan = self._backend == _BACKEND_BINNED or (
            self._backend == _AUTO and mc.shape[0] * sc.shape[0] >= self._binned_auto_min_pairs)
        if use_plan and Plan.supported(mc, vc, sc):
            self.plan = self._build_plan(self._q_max)
        elif self._backend == _BACKEND_BINNED and N > 0 and sc.shape[0] > 0:
            raise NotImplementedError("backend='binned' needs float32, d = 2, c <= 2")

    def _periodic_images(self, means, values, conics):
        """The 9N images, an autograd-tracked launch (also when preprocess runs under no_grad: the outputs of a later
        differentiable sample_*() call must reach the caller's tensors, as without periodic).  Debug mode reads the
        extent flag back (one synchronisation); otherwise it is never read and not even allocated."""
        lo, hi = self.periodic
        check = self._debug and means.shape[0] > 0 and not torch.cuda.is_current_stream_capturing()
        flag = torch.zeros(1, dtype=torch.int32, device=means.device) if check else None
        with torch.enable_grad():
            imgs = _PeriodicImages.apply(means, values, conics, lo, hi - lo, self._q_cut, flag)
        if check:
            _check_periodic_flag(int(flag.item()), self.periodic, self._q_cut)
        return imgs

    def _needs_backward(self, target=None):
        """Can a backward follow a launch made now (grad mode on and an input that requires grad)?  Plans built when
        it cannot are forward-only (PIGS_BUILD_FORWARD_ONLY)."""
        if not torch.is_grad_enabled() or self._inputs is None:
            return False
        mc, vc, cc, _ = self._inputs
        return mc.requires_grad or vc.requires_grad or cc.requires_grad or (target is not None and target.requires_grad)

    def _build_plan(self, q_max, sample_plan=None, forward_only=None):
        """A plan for the bound inputs; the samples half is reused when ``preprocess`` was handed an
        unmodified samples tensor it remembers (``reuse_samples``).  While a hipGraph is being captured
        nothing is looked up and nothing is remembered: the capture has to record the samples build
        itself (a replay after an in-place update of the static samples input must re-sort them), its
        workspaces belong to the graph (they neither come from the pool nor go back to it), and a
        SamplePlan that was only recorded has not been built as far as later eager calls go."""
        mc, vc, cc, sc = self._inputs
        capturing = torch.cuda.is_current_stream_capturing()
        sp = sample_plan
        if sp is None and (not capturing or self.static_samples):
            sp = next((p for p in self.sample_plans if p.built and p.matches(self._samples_source)), None)
        pool = None if capturing else self._pool
        if forward_only is None:
            forward_only = not self._needs_backward()
        with torch.no_grad():
            plan = Plan(mc.detach(), vc.detach(), cc.detach(), sc, q_max, sp, self._samples_source, pool,
                        recorded_only=capturing, q_max_backward=max(q_max, self._q_max_backward),
                        defer_lists=self.defer_lists, forward_only=forward_only)
        if self._reuse_samples and not capturing:
            self.sample_plans = [plan.samples] + [p for p in self.sample_plans if p is not plan.samples]
            del self.sample_plans[self._reuse_samples:]
        if self._debug and not capturing:
            torch.cuda.synchronize(mc.device)
        return plan

    # ------------------------------------------------------------------ sampling
    def _require_inputs(self):
        if self._inputs is None:
            raise RuntimeError("preprocess() must be called before sampling")
        return self._inputs

    def _plan_for(self, mask, target=None):
        """The plan a launch with this order mask runs on: third derivatives get the wider cut-off."""
        if self.plan is None:
            return None
        capturing = torch.cuda.is_current_stream_capturing()
        # an eager call behind a capture (no preprocess in between) must not sample what the capture only
        # RECORDED: the plan is rebuilt eagerly, on a samples half of its own (the recorded one belongs to the
        # graph, whose replays re-sort it)
        if self.plan.recorded_only and not capturing:
            self.plan = self._build_plan(self._q_max)
            self.plan3 = None
        # a differentiable call on a plan preprocess built for the forward alone (no_grad): the plan is rebuilt in
        # full first, on the same samples half; an autograd node never holds a forward-only plan
        needs_backward = self._needs_backward(target)
        if needs_backward and self.plan.forward_only:
            self.plan = self._build_plan(self._q_max, self.plan.samples, forward_only=False)
            self.plan3 = None
        if not mask & 8 or self._q_max_order3 == self._q_max:
            return self.plan
        if self.plan3 is not None and self.plan3.recorded_only and not capturing:
            self.plan3 = None
        if self.plan3 is not None and needs_backward and self.plan3.forward_only:
            self.plan3 = None
        if self.plan3 is None:
            self.plan3 = self._build_plan(self._q_max_order3, self.plan.samples)     # same points: the sorted samples are shared
        return self.plan3

    def _compute(self, mask):
        means, values, conics, samples = self._require_inputs()
        outs = _SampleFunction.apply(means, values, conics, samples, mask, self._debug, self._plan_for(mask))
        for k, o in zip(_mask_orders(mask), outs):
            self._cache[k] = o

    def get(self, order):
        if order not in self._cache:
            means, _, _, samples = self._require_inputs()
            mask = 1 << order
            if order <= 2 and (self._fuse == _FUSE_ALL or (
                    self._fuse == _AUTO and samples.shape[0] <= self._fuse_auto_max_points)):
                mask |= 7 & ~sum(1 << k for k in self._cache)
            self._compute(mask)
        return self._cache[order]

    def sample(self, orders):
        """orders: 0..3 and TRACE (the facade maps "lap")."""
        self._require_inputs()
        want = set(o for o in orders if o not in self._cache)
        if TRACE in want and (2 in want or 2 in self._cache):
            want.discard(TRACE)                    # the Hessian is (being) computed: take its diagonal
        if TRACE in want and 3 in want:            # no fused kernel for trace + order 3: two launches
            self._compute(1 << 3)
            want.discard(3)
        mask = sum(1 << o for o in want)
        if mask:
            self._compute(mask)
        if TRACE in orders and TRACE not in self._cache:
            self._cache[TRACE] = self._cache[2].diagonal(dim1=1, dim2=2).sum(-1)
        return tuple(self._cache[o] for o in orders)

    # ------------------------------------------------------------------ fused outputs
    # (the arguments arrive checked, detached and contiguous -- the facade does it -- and flat, as the native core takes them)
    def _fused(self, function, mask, side, params, target=None, want_aux=False):
        means, values, conics, samples = self._require_inputs()
        return function.apply(means, values, conics, samples, side, params, self._debug, self._plan_for(mask, target), want_aux)

    def residual(self, coeffs, target=None):
        return self._fused(_ResidualFunction, 0, target, ResidualCoeffs(coeffs), target)

    def residual_terms(self, fields, consts, advect_by, target=None):
        terms = ResidualTerms(fields, consts, advect_by)
        return self._fused(_ResidualTermsFunction, 0, target, terms, target, terms.advects and self._needs_backward(target))

    def residual_coupled(self, fields, consts, couple0, couple_lap, target=None):
        return self._fused(_ResidualCoupledFunction, 0, target, ResidualCoupling(fields, consts, couple0, couple_lap), target)

    def vorticity_terms(self):
        means, values, _, _ = self._require_inputs()
        d, c = means.shape[1], values.shape[1]
        if d != 2 or c != 2:
            raise NotImplementedError(f"vorticity_terms() needs a two-channel field in two dimensions, got d = {d}, c = {c}")
        # (a result computed where no backward could follow is not handed to a later differentiable call)
        if self._vorticity is None or (self._needs_backward() and not self._vorticity.requires_grad):
            self._vorticity = self._fused(_VorticityFunction, 8, None, None)
        return self._vorticity

    def vorticity_residual(self, nu, dt, time_term, tau, tau_field=None, prev=None):
        params = VorticityResidual(nu, dt, time_term, tau if tau_field is None else tau_field)
        return self._fused(_VorticityResidualFunction, 8, prev, params, want_aux=self._needs_backward())

    def _vorticity_fit(self, nu, dt, time_term, tau, tau_field, prev, data, data_weight):
        params = VorticityFit(nu, dt, time_term, tau if tau_field is None else tau_field, data, data_weight)
        return self._fused(_VorticityFitFunction, 8, prev, params, want_aux=self._needs_backward())

    def _network_inputs(self, kind, nu, wave0, wave1):
        """sample_u, sample_ux, sample_uxx, sample_pde as views of one allocation; forward only, no autograd node."""
        means, values, conics, samples = self._require_inputs()
        N, d = means.shape
        c, M = values.shape[1], samples.shape[0]
        widths = (c, 2 * c, 2 * c, network_pde_width(kind, c))
        with torch.no_grad():
            launch = N > 0 and M > 0
            buf = (torch.empty if launch else torch.zeros)(M * sum(widths), dtype=means.dtype, device=means.device)
            outs, at = [], 0
            for w in widths:
                outs.append(buf[at:at + M * w].view(M, w))
                at += M * w
            if launch:
                # the plan of the bound inputs as it stands (a forward-only one serves: no backward follows); the
                # vorticity's third derivatives take the order-3 plan
                plan = self._plan_for(8 if kind == _NET_NAVIER_STOKES else 0)
                pw = (_ptr(plan.workspace), plan.workspace.numel(), _ptr(plan.samples.workspace), plan.samples.workspace.numel()) \
                    if plan is not None else (ctypes.c_void_p(0), 0, ctypes.c_void_p(0), 0)
                with _on_device(means.device):
                    stream = _stream(means.device)
                    if plan is not None and hasattr(plan, "note_stream"):
                        plan.note_stream(stream.value)
                    params = _lib.PigsNetworkInputs(kind, nu, (wave0, wave1))
                    rc = _lib.load().pigs_network_inputs_forward(
                        _DTYPES[means.dtype], d, c, N, M, _ptr(means), _ptr(conics), _ptr(values), _ptr(samples),
                        ctypes.byref(params), *(_ptr(o) for o in outs), *pw, stream)
                    _lib.check(rc, "pigs_network_inputs_forward")
            if self._debug:
                torch.cuda.synchronize(means.device)
        return tuple(outs)

    # ------------------------------------------------------------------ neighbour aggregation
    def preprocess_aggregate(self, cap=-1):
        self._require_inputs()
        means, conics = self._caller          # the caller's N Gaussians, not the periodic images
        if means.shape[1] != 2:
            raise NotImplementedError("aggregate_neighbors is implemented for d = 2")
        box = None
        if self.periodic_aggregate:
            if self._box is None:
                raise RuntimeError("periodic_aggregate=True: preprocess() must have run with periodic=(lo, hi)")
            # block 0 of the bound images: the wrapped centres and their conics
            N = means.shape[0]
            means, conics = self._inputs[0][:N], self._inputs[2][:N]
            box = (self._box[0], self._box[1] - self._box[0])
        self.neighbors = aggregate.NeighborLists(means, conics, self._q_max, cap=None if cap < 0 else cap, periodic=box)
        if self._debug:
            self.neighbors.check()

    def aggregate_neighbors(self, features, transform, queries, keys, frequencies, distance_transform):
        if self.neighbors is None:
            raise RuntimeError("preprocess_aggregate() must be called before aggregate_neighbors()")
        return aggregate.aggregate(self.neighbors, features, transform, queries, keys, frequencies, distance_transform)

    def aggregate_neighbors_heads(self, features, transforms, queries, keys, frequencies, distance_transforms):
        if self.neighbors is None:
            raise RuntimeError("preprocess_aggregate() must be called before aggregate_neighbors_heads()")
        return aggregate.aggregate_heads(self.neighbors, features, transforms, queries, keys, frequencies, distance_transforms)
