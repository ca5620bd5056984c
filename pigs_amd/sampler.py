"""Host side of the sampler: the reference's ``GaussianSampler`` operator surface on MI355X.

Mirrors the Python-visible interface of the reference's native extension
(``from diff_gaussian_sampling import GaussianSampler``), known from its call sites:

* ``GaussianSampler(flag)``                       model_pn.py:423 (False), tests (True)
* ``preprocess(means, values, covariances, conics, samples)``
                                                  model_pn.py:648,768,784; test_gaussian_sampling.py:56;
                                                  test_derivatives.py:82; test_1d.py:30
* ``sample_gaussians()            -> [M, c]``      model_pn.py:650
* ``sample_gaussians_derivative() -> [M, d, c]``   model_pn.py:651
* ``sample_gaussians_laplacian()  -> [M, d, d, c]`` (the full Hessian) model_pn.py:652
* ``sample_gaussians_third_derivative() -> [M, d, d, d, c]``  model_pn.py:654

Outputs are differentiable wrt the ``means``, ``values`` and ``conics`` passed to the preceding
``preprocess`` (test_derivatives.py:123, 214-215, 349-352), also after later ``preprocess`` calls
(model_pn.py:766-788 then main_pn.py:220): every autograd node owns the tensors it needs.

All arithmetic runs in the HIP library behind the C ABI of include/pigs_amd.h; there is no CPU
or PyTorch fallback -- CPU tensors are rejected.
"""
import ctypes
import math
import os
import threading

import torch

from . import _lib

_ORDER_NAMES = ("sample_gaussians", "sample_gaussians_derivative", "sample_gaussians_laplacian",
                "sample_gaussians_third_derivative")
_DTYPES = {torch.float32: _lib.PIGS_F32, torch.float64: _lib.PIGS_F64}


TRACE = 4       # order index of the Hessian's trace (mask bit 16); it travels in pointer slot 2
# the columns of GaussianSampler.vorticity_terms(): the field, its divergence, the vorticity w = d_x u_y - d_y u_x,
# its gradient and its Laplacian
VORTICITY_COLUMNS = ("u_x", "u_y", "div", "w", "w_x", "w_y", "lap_w")
# the columns of GaussianSampler.vorticity_residual(): the blended divergence and the vorticity equation's residual
VORTICITY_RESIDUAL_COLUMNS = ("div", "r")


def _out_shape(order, M, d, c):
    return (M, c) if order == TRACE else (M,) + (d,) * order + (c,)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
    # the current stream's handle: the raw getter skips building a torch.cuda.Stream object (5 us a call)
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


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
    """The coefficients of a general residual() call: floats or detached device fields (a0, aL, adv: [M]; a1: d floats
    or [M, d]) and the d x c constants ``advect_by``.  ``advects``: the advection term is active."""

    def __init__(self, a0, a1, aL, adv, advect_by):
        self.a0, self.a1, self.aL, self.adv, self.advect_by = a0, a1, aL, adv, advect_by
        self.advects = isinstance(adv, torch.Tensor) or adv != 0.0

    def struct(self):
        t = _lib.PigsResidualTerms()
        for name, v in (("a0", self.a0), ("aL", self.aL), ("adv", self.adv)):
            if isinstance(v, torch.Tensor):
                setattr(t, name + "_pt", v.data_ptr())
            else:
                setattr(t, name, v)
        if isinstance(self.a1, torch.Tensor):
            t.a1_pt = self.a1.data_ptr()
        else:
            for i, v in enumerate(self.a1):
                t.a1[i] = v
        for i, row in enumerate(self.advect_by):
            for k, v in enumerate(row):
                t.advect_by[i][k] = v
        return t


class ResidualCoupling:
    """The coefficients of a coupled residual() call: a0, aL, cw as floats or detached device fields [M], and the two
    c x c constant matrices (row = output channel, column = input channel)."""

    def __init__(self, a0, aL, cw, couple0, couple_lap):
        self.a0, self.aL, self.cw, self.couple0, self.couple_lap = a0, aL, cw, couple0, couple_lap

    def struct(self):
        t = _lib.PigsResidualCoupling()
        for name, v in (("a0", self.a0), ("aL", self.aL), ("cw", self.cw)):
            if isinstance(v, torch.Tensor):
                setattr(t, name + "_pt", v.data_ptr())
            else:
                setattr(t, name, v)
        for dst, src in ((t.couple0, self.couple0), (t.couple_lap, self.couple_lap)):
            for i, row in enumerate(src):
                for k, v in enumerate(row):
                    dst[i][k] = v
        return t


class VorticityResidual:
    """The coefficients of a vorticity_residual() call: three floats and ``tau``, a float or a detached device field
    [M, 1]."""

    def __init__(self, nu, dt, time_term, tau):
        self.nu, self.dt, self.time_term, self.tau = nu, dt, time_term, tau

    def struct(self):
        t = _lib.PigsVorticityResidual()
        t.nu, t.dt, t.time_term = self.nu, self.dt, self.time_term
        if isinstance(self.tau, torch.Tensor):
            t.tau_pt = self.tau.data_ptr()
        else:
            t.tau = self.tau
        return t


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


def _periodic_box(periodic):
    """None, or the box (lo, hi) as two finite floats with hi > lo."""
    if periodic is None:
        return None
    try:
        lo, hi = periodic
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"periodic must be None or (lo, hi), got {periodic!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(hi - lo) and hi > lo):
        raise ValueError(f"periodic=(lo, hi) needs finite lo < hi, got {periodic!r}")
    return lo, hi


def _check_periodic_flag(flag, box, q_cut):
    if flag:
        lo, hi = box
        raise ValueError(f"periodic=({lo}, {hi}): a Gaussian's cut-off ellipse (q <= {q_cut}) spans one period "
                         f"L = {hi - lo} or more on an axis (sqrt(q_cut Sigma_ii) >= L), or its conic is not positive "
                         "definite, or its mean is not finite: the 3 x 3 images do not give the periodic field")


_FUSE_CODES = {"auto": 0, "all": 1, "none": 2}
_BACKEND_CODES = {"auto": 0, "dense": 1, "binned": 2}


def _load_native_host():
    """The native host extension (pigs_amd/_pigs_host.so, csrc_host/pigs_host.cpp); there is no silent
    fallback to the ctypes host: a missing extension raises."""
    _lib.load()
    variant = os.environ.get("PIGS_AMD_LIB")
    if variant and os.path.realpath(variant) != os.path.realpath(os.path.join(_lib.HERE, "libpigs_amd.so")):
        # _pigs_host.so resolves libpigs_amd.so through its $ORIGIN rpath: the launches would run the in-tree
        # library while the ctypes calls ran the variant -- two instances with separate state, an A/B run
        # timing the wrong kernels without noticing
        raise ImportError(f"PIGS_AMD_LIB={variant} selects a variant library, which only the ctypes host can drive: "
                          "construct GaussianSampler(..., host='ctypes') or set PIGS_AMD_HOST=ctypes")
    try:
        from . import _pigs_host
    except ImportError as e:
        raise ImportError(
            "pigs_amd/_pigs_host.so (the native host side of GaussianSampler) is missing or does not load: "
            f"{e}.  Build it first (python -m pigs_amd.build), or ask for the ctypes host explicitly "
            "(GaussianSampler(..., host='ctypes') / PIGS_AMD_HOST=ctypes).") from e
    if _pigs_host.ABI_VERSION != _lib.ABI_VERSION:
        raise ImportError(f"_pigs_host.so was built against ABI {_pigs_host.ABI_VERSION}, expected {_lib.ABI_VERSION}; rebuild")
    return _pigs_host


class GaussianSampler:
    """MI355X-native replacement of ``diff_gaussian_sampling.GaussianSampler``.

    ``flag`` is the single positional bool of the reference constructor (True in its tests,
    False in model_pn.py:423; meaning not visible in the reference).  Here it is a debug switch:
    when set, every launch is followed by a device synchronise so that errors surface at the call.

    ``backend`` (extension, keyword only): ``"dense"`` evaluates every (point, Gaussian) pair --
    the reference's dense semantics exactly; ``"binned"`` builds the culling plan in ``preprocess``
    and drops pairs with q > ``q_max`` (relative truncation below exp(-q_max/2); launches that
    compute third derivatives use the wider ``q_max_order3``, default q_max + 8, through a second
    plan built on first use: dropped terms carry a q^1.5 prefactor there, q^2.5 in its conic
    gradient -- tools/fuzz_stats.py: 2 of 300 adversarial cases left the 1e-5 bar at 36, none at
    40; the backward of gradients that arrive at second derivatives (or the trace) uses
    ``q_max_backward``, default q_max + 4, through wider group masks kept in the SAME plan: the conic
    gradient of such a term carries q^2 and its sum nearly cancels -- tools/fuzz_diag.py, worst of the four
    worst fuzz cases: 2.5e-5 of the largest entry at 36, 3.5e-6 at 40 -- the dense kernel's own float32
    error on those cases is 3.3e-6 -- 3.4e-6 at 44); ``"auto"`` picks
    binned for float32, d = 2, c <= 2 once N*M >= 2**26 pairs, where the plan pays for itself.

    ``reuse_samples`` (extension, keyword only; binned path): when ``preprocess`` is called again with a
    samples tensor it has seen recently (same storage, shape and version counter, i.e. not written
    to in between) the sorted sample structure built for it is reused and only the Gaussian half
    of the plan is rebuilt -- the reference's roll-out binds new Gaussians to a fixed grid every
    step (main_pn.py:317-324), its training step alternates between the collocation points and
    the boundary points (model_pn.py:766-785).  ``True`` remembers the last 4 sample tensors, an
    integer that many, ``False`` rebuilds everything every time.  While a hipGraph is being captured
    nothing is looked up or remembered: the capture records the samples build itself, so a replay
    after an in-place update of the samples re-sorts them.

    ``unpinned_aggregate`` (extension, keyword only): ``preprocess_aggregate`` / ``aggregate_neighbors``
    follow this repository's own definition (the reference's is not visible: parity unpinned) and
    warn once per process unless this is set.

    ``aggregate_cap`` (extension, keyword only): slots per Gaussian of the neighbour lists of
    ``preprocess_aggregate``.  Default ``None``: sized by a counting pass whose result is read back once per
    call (a host synchronisation); an integer skips that (lists that do not fit are truncated and flagged:
    debug mode raises).

    ``fuse`` (extension, keyword only) controls how many derivative orders one launch computes:
    ``"auto"`` -- the first ``sample_*`` call after a ``preprocess`` computes orders 0..2 in one
    launch when the problem is small enough to be launch-bound (M <= 65536), otherwise only the
    order asked for; ``"all"`` / ``"none"`` force either behaviour.  :meth:`sample` is the
    explicit fused entry point.

    ``defer_lists`` (extension, keyword only; binned path; default False): with True ``preprocess`` stops in front
    of the tile lists and the first ``sample_*`` call builds them in the same launch as its own evaluation
    (PIGS_BUILD_DEFER_LISTS, include/pigs_amd.h).  Built in round 4 to hide the latency-bound list build behind the
    forward's arithmetic; measured at C3 it does not (49.8 us against 21.8 + 26.5 in two launches: every wave builds
    first and evaluates afterwards, in step with all the others -- DESIGN.md section 3.3), so it is an option, not
    the default.

    ``periodic`` (extension, keyword only; default None; settable, the next ``preprocess`` uses it): ``(lo, hi)`` declares the periodic box [lo, hi)^2 with period
    L = hi - lo on both axes -- the reference's Navier-Stokes problem, whose model wraps its means back into the box
    after every update (model_pn.py:689-693).  ``preprocess`` then wraps every mean into the box (the gradient flows to
    the caller's mean unchanged) and binds the 3 x 3 images of every Gaussian, shifted by -L, 0, +L on each axis, in
    place of the N originals: every ``sample_*`` output, ``residual()`` and every gradient is that of the periodic
    field.  Sample points are not wrapped; for points in the closed box the sum is the periodic field exactly (up to
    the cut-off) when every Gaussian's q <= q_cut ellipse spans less than one period on each axis, sqrt(q_cut
    Sigma_ii) < L with q_cut = max(q_max, q_max_backward, q_max_order3) -- debug mode (``flag``) checks this and
    raises ``ValueError``.  d = 2 only (d = 1 raises ``NotImplementedError``); dense and binned alike, the ``auto``
    rule counting the 9N images.  ``preprocess_aggregate`` / ``aggregate_neighbors`` keep working on the caller's N
    Gaussians with the non-periodic neighbour definition unless ``periodic_aggregate`` is set.  ``lo`` and ``hi - lo``
    reach the kernels as doubles and are cast to the tensors' dtype there: a float32 sampler lives on the torus of
    float32(hi - lo) from float32(lo).  For (0, 2 pi) that period is 1.7e-7 away from 2 pi -- for narrow Gaussians a
    visible change of q next to the seam, and no error: wrap means and points with the same float32 period.  The
    wrapped means lie in the closed box [lo, lo + L] (a mean just below lo lands on hi, the same point of the torus).

    ``periodic_aggregate`` (extension, keyword only; default False; settable like ``periodic``; True without
    ``periodic`` raises ``ValueError``): ``preprocess_aggregate`` builds the neighbour lists of the torus from the
    wrapped centres (block 0 of the bound images) and ``aggregate_neighbors`` runs on them: the neighbours of i are
    the pairs (j, image k) whose shifted ellipse reaches the wrapped centre of i, each with its own offset
    mu'_j + s_k L - mu'_i, density and softmax entry -- the non-periodic definition on the 9N images, rows of the
    originals; the result is invariant under a translation of all means round the torus.  A Gaussian can be met
    through several images, so a list can be longer than N: the list size always comes from the counting pass (one
    read-back) unless ``aggregate_cap`` is given or a capture is running (slab min(4N, 8192 / 4096 in float64)).

    ``host`` (extension, keyword only): ``"native"`` (default; environment override PIGS_AMD_HOST) keeps
    the sampler's state and its autograd node in the C++ torch extension ``pigs_amd/_pigs_host.so``
    (csrc_host/pigs_host.cpp) -- what the reference's own boundary is (a compiled torch extension,
    model_pn.py:11); ``"ctypes"`` is the same logic in Python over ``ctypes`` (this file).  Both call
    the same C ABI; neither has a CPU fallback.

    Memory: the autograd node of a launch owns the tensors bound by ``preprocess`` and the plan (160 B
    per sample point at N > 512), and keeps them until every output of that launch is gone -- not just
    until the first backward (the reference's scripts come back to another output of the same launch
    after a non-retaining backward, test_derivatives.py:214-215, 349-352); saved-tensor hooks
    (``save_on_cpu``, checkpointing) do not see them.  Roll-outs that keep every step's outputs keep
    every step's plan.
    """

    FUSE_AUTO_MAX_POINTS = 1 << 16
    BINNED_AUTO_MIN_PAIRS = 1 << 26     # dense: ~1.2e12 pairs/s; the plan costs ~32 us to build

    _warned_samples_grad = False
    _warned_aggregate = False

    def __init__(self, flag=False, *, fuse="auto", backend="auto", q_max=36.0, q_max_order3=None,
                 q_max_backward=None, reuse_samples=True, unpinned_aggregate=False, aggregate_cap=None, host=None,
                 defer_lists=False, periodic=None, periodic_aggregate=False):
        if fuse not in ("auto", "all", "none"):
            raise ValueError("fuse must be 'auto', 'all' or 'none'")
        if backend not in ("auto", "dense", "binned"):
            raise ValueError("backend must be 'auto', 'dense' or 'binned'")
        if not q_max > 0:
            raise ValueError("q_max must be positive")
        if host is None:
            host = os.environ.get("PIGS_AMD_HOST") or "native"
        if host not in ("native", "ctypes"):
            raise ValueError("host must be 'native' or 'ctypes'")
        self.debug = bool(flag)
        self.fuse = fuse
        self.backend = backend
        self.host = host
        self.q_max = float(q_max)
        self.q_max_order3 = float(q_max_order3) if q_max_order3 is not None else self.q_max + 8.0
        if self.q_max_order3 < self.q_max:
            raise ValueError("q_max_order3 must not be below q_max")
        self.q_max_backward = float(q_max_backward) if q_max_backward is not None else self.q_max + 4.0
        if self.q_max_backward < self.q_max:
            raise ValueError("q_max_backward must not be below q_max")
        self.reuse_samples = 4 if reuse_samples is True else max(0, int(reuse_samples))
        self.defer_lists = bool(defer_lists)
        self._periodic = _periodic_box(periodic)
        self._periodic_aggregate = bool(periodic_aggregate)
        if self._periodic_aggregate and self._periodic is None:
            raise ValueError("periodic_aggregate=True needs periodic=(lo, hi)")
        self._st_caller = None
        self._st_box = None
        self._static_samples = False
        self.unpinned_aggregate = bool(unpinned_aggregate)
        self.aggregate_cap = None if aggregate_cap is None else int(aggregate_cap)
        self._neighbors = None
        self._st_plan3 = None
        self._st_inputs = None
        self._st_plan = None
        self._st_sample_plans = []       # most recently used first, at most ``reuse_samples``
        self._plan_pool = _PlanPool()
        self._samples_source = None
        self._cache = {}
        self._vorticity = None           # the cached vorticity_terms() of the bound inputs
        _lib.load()  # fail at construction, not at first use, if the HIP library is missing
        self._core = None
        if host == "native":
            self._core = _load_native_host().SamplerCore(self.debug, _FUSE_CODES[fuse], _BACKEND_CODES[backend],
                                                         self.q_max, self.q_max_order3, self.q_max_backward,
                                                         self.reuse_samples)
            self._core.defer_lists = self.defer_lists
            self._core.periodic = self._periodic
            self._core.periodic_aggregate = self._periodic_aggregate

    @property
    def periodic_aggregate(self):
        """Settable: whether ``preprocess_aggregate`` builds the neighbour lists of the torus (class docstring); takes
        effect at the next ``preprocess_aggregate``, on both hosts."""
        return self._periodic_aggregate

    @periodic_aggregate.setter
    def periodic_aggregate(self, value):
        if value and self._periodic is None:
            raise ValueError("periodic_aggregate=True needs periodic=(lo, hi)")
        self._periodic_aggregate = bool(value)
        if self._core is not None:
            self._core.periodic_aggregate = self._periodic_aggregate

    @property
    def periodic(self):
        """Settable: None or the box (lo, hi) (class docstring); a new value takes effect at the next ``preprocess``,
        on both hosts."""
        return self._periodic

    @periodic.setter
    def periodic(self, value):
        box = _periodic_box(value)
        if box is None and self._periodic_aggregate:
            raise ValueError("periodic_aggregate=True needs periodic=(lo, hi): clear periodic_aggregate first")
        self._periodic = box
        if self._core is not None:
            self._core.periodic = self._periodic

    @property
    def q_cut(self):
        """The widest cut-off any launch samples with: the extent condition of the periodic images is checked against
        it."""
        return max(self.q_max, self.q_max_backward, self.q_max_order3)

    @property
    def static_samples(self):
        """Settable.  While a hipGraph is being captured ``preprocess`` normally records the samples build too (a
        replay after an in-place update of the static samples input re-sorts them), so a replay is a COLD step.
        With ``static_samples = True`` a capture reuses the sorted sample structure that an eager ``preprocess``
        (the capture's warm-up runs) built for the same, unmodified samples tensor: the graph holds the Gaussian
        half only and a replay is a warm step.  The caller promises not to write to that samples tensor between
        replays (``pigs_amd.graphs.GraphedStep(..., samplers=[...], static_samples=True)`` sets this and keeps the
        reused structure alive)."""
        return self._static_samples

    @static_samples.setter
    def static_samples(self, value):
        self._static_samples = bool(value)
        if self._core is not None:
            self._core.static_samples = self._static_samples

    # state lives in the native core when there is one
    @property
    def _plan(self):
        return self._core.plan if self._core is not None else self._st_plan

    @property
    def _plan3(self):
        return self._core.plan3 if self._core is not None else self._st_plan3

    @property
    def _inputs(self):
        return self._core.inputs() if self._core is not None else self._st_inputs

    @property
    def _sample_plans(self):
        return self._core.sample_plans if self._core is not None else self._st_sample_plans

    # ------------------------------------------------------------------ preprocess
    def preprocess(self, means, values, covariances, conics, samples):
        """Bind the Gaussians and the sample points for the following ``sample_*`` calls.

        means [N,d]; values [N,c] (or [N]); covariances and conics flat [N, d(d+1)/2]
        (d=1: anything with N elements, e.g. [N,1] or [N,1,1]); samples [M,d] (d=1: also [M]).
        ``covariances`` does not enter the sampled values (the reference's dense twin,
        gaussians.py:48-58, never reads it); it is accepted for interface parity.
        """
        for name, t in (("means", means), ("values", values), ("conics", conics), ("samples", samples)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor")
        if self._core is not None:
            self._neighbors = None
            self._core.preprocess(means, values, covariances, conics, samples)
            return
        if means.dim() != 2:
            raise ValueError(f"means must be [N, d], got {tuple(means.shape)}")
        N, d = means.shape
        if d not in (1, 2):
            raise NotImplementedError(f"d = {d} is not supported (d in {{1, 2}})")
        nf = d * (d + 1) // 2
        for name, t in (("means", means), ("values", values), ("conics", conics), ("samples", samples)):
            if not t.is_cuda:
                raise RuntimeError(f"{name} is on {t.device}: GaussianSampler runs on the GPU only "
                                   "(no CPU fallback)")
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
        if samples.requires_grad and torch.is_grad_enabled() and not GaussianSampler._warned_samples_grad:
            GaussianSampler._warned_samples_grad = True
            import warnings
            warnings.warn("GaussianSampler: samples.requires_grad is set, but the sampler returns no gradient "
                          "with respect to the sample points (as the reference, whose tests ask for the gradients "
                          "of means, values and conics only); use the derivative outputs instead", stacklevel=2)
        means, values, conics = means.contiguous(), values.contiguous(), conics.contiguous()
        self._st_caller = (means, conics)
        self._st_box = self.periodic             # the box the bound images were made with
        if self.periodic is not None:
            self._st_inputs = None          # a preprocess that raises leaves nothing bound
            if d != 2:
                raise NotImplementedError("periodic=(lo, hi) is implemented for d = 2")
            means, values, conics = self._periodic_images(means, values, conics)
        self._st_inputs = (means, values, conics, samples.detach().contiguous())
        self._samples_source = samples
        self._cache = {}
        self._vorticity = None
        self._st_plan = None
        self._st_plan3 = None
        self._neighbors = None
        mc, vc, cc, sc = self._st_inputs
        # the pairs the launches will evaluate: with periodic=... the bound rows are the 9N images
        use_plan = self.backend == "binned" or (
            self.backend == "auto" and mc.shape[0] * sc.shape[0] >= self.BINNED_AUTO_MIN_PAIRS)
        if use_plan and Plan.supported(mc, vc, sc):
            self._st_plan = self._build_plan(self.q_max)
        elif self.backend == "binned" and N > 0 and sc.shape[0] > 0:
            raise NotImplementedError("backend='binned' needs float32, d = 2, c <= 2")

    def _periodic_images(self, means, values, conics):
        """The 9N images, an autograd-tracked launch (also when preprocess runs under no_grad: the outputs of a later
        differentiable sample_*() call must reach the caller's tensors, as without periodic).  Debug mode reads the
        extent flag back (one synchronisation); otherwise it is never read and not even allocated."""
        lo, hi = self.periodic
        check = self.debug and means.shape[0] > 0 and not torch.cuda.is_current_stream_capturing()
        flag = torch.zeros(1, dtype=torch.int32, device=means.device) if check else None
        with torch.enable_grad():
            imgs = _PeriodicImages.apply(means, values, conics, lo, hi - lo, self.q_cut, flag)
        if check:
            _check_periodic_flag(int(flag.item()), self.periodic, self.q_cut)
        return imgs

    def _needs_backward(self, target=None):
        """Can a backward follow a launch made now (grad mode on and an input that requires grad)?  Plans built when
        it cannot are forward-only (PIGS_BUILD_FORWARD_ONLY)."""
        if not torch.is_grad_enabled() or self._st_inputs is None:
            return False
        mc, vc, cc, _ = self._st_inputs
        return mc.requires_grad or vc.requires_grad or cc.requires_grad or (target is not None and target.requires_grad)

    def _build_plan(self, q_max, sample_plan=None, forward_only=None):
        """A plan for the bound inputs; the samples half is reused when ``preprocess`` was handed an
        unmodified samples tensor it remembers (``reuse_samples``).  While a hipGraph is being captured
        nothing is looked up and nothing is remembered: the capture has to record the samples build
        itself (a replay after an in-place update of the static samples input must re-sort them), its
        workspaces belong to the graph (they neither come from the pool nor go back to it), and a
        SamplePlan that was only recorded has not been built as far as later eager calls go."""
        mc, vc, cc, sc = self._st_inputs
        capturing = torch.cuda.is_current_stream_capturing()
        sp = sample_plan
        if sp is None and (not capturing or self.static_samples):
            sp = next((p for p in self._st_sample_plans if p.built and p.matches(self._samples_source)), None)
        pool = None if capturing else self._plan_pool
        if forward_only is None:
            forward_only = not self._needs_backward()
        with torch.no_grad():
            plan = Plan(mc.detach(), vc.detach(), cc.detach(), sc, q_max, sp, self._samples_source, pool,
                        recorded_only=capturing, q_max_backward=max(q_max, self.q_max_backward),
                        defer_lists=self.defer_lists, forward_only=forward_only)
        if self.reuse_samples and not capturing:
            self._st_sample_plans = [plan.samples] + [p for p in self._st_sample_plans if p is not plan.samples]
            del self._st_sample_plans[self.reuse_samples:]
        if self.debug and not capturing:
            torch.cuda.synchronize(mc.device)
        return plan

    # ------------------------------------------------------------------ sampling
    def _require_inputs(self):
        inputs = self._inputs
        if inputs is None:
            raise RuntimeError("preprocess() must be called before sampling")
        return inputs

    def _plan_for(self, mask, target=None):
        """The plan a launch with this order mask runs on: third derivatives get the wider cut-off."""
        if self._st_plan is None:
            return None
        capturing = torch.cuda.is_current_stream_capturing()
        # an eager call behind a capture (no preprocess in between) must not sample what the capture only
        # RECORDED: the plan is rebuilt eagerly, on a samples half of its own (the recorded one belongs to the
        # graph, whose replays re-sort it)
        if self._st_plan.recorded_only and not capturing:
            self._st_plan = self._build_plan(self.q_max)
            self._st_plan3 = None
        # a differentiable call on a plan preprocess built for the forward alone (no_grad): the plan is rebuilt in
        # full first, on the same samples half; an autograd node never holds a forward-only plan
        needs_backward = self._needs_backward(target)
        if needs_backward and self._st_plan.forward_only:
            self._st_plan = self._build_plan(self.q_max, self._st_plan.samples, forward_only=False)
            self._st_plan3 = None
        if not mask & 8 or self.q_max_order3 == self.q_max:
            return self._st_plan
        if self._st_plan3 is not None and self._st_plan3.recorded_only and not capturing:
            self._st_plan3 = None
        if self._st_plan3 is not None and needs_backward and self._st_plan3.forward_only:
            self._st_plan3 = None
        if self._st_plan3 is None:
            self._st_plan3 = self._build_plan(self.q_max_order3, self._st_plan.samples)     # same points: the sorted samples are shared
        return self._st_plan3

    def _compute(self, mask):
        means, values, conics, samples = self._require_inputs()
        outs = _SampleFunction.apply(means, values, conics, samples, mask, self.debug, self._plan_for(mask))
        for k, o in zip(_mask_orders(mask), outs):
            self._cache[k] = o

    def _get(self, order):
        if self._core is not None:
            return self._core.get(order)
        if order not in self._cache:
            means, _, _, samples = self._require_inputs()
            mask = 1 << order
            if order <= 2 and (self.fuse == "all" or (
                    self.fuse == "auto" and samples.shape[0] <= self.FUSE_AUTO_MAX_POINTS)):
                mask = 7 & ~sum(1 << k for k in self._cache)
                mask |= 1 << order
            self._compute(mask)
        return self._cache[order]

    def sample(self, orders=(0, 1, 2)):
        """Fused entry point: one launch for all ``orders`` (extension of the reference API).
        ``orders`` holds derivative orders 0..3 and / or ``"lap"`` -- the trace of the Hessian
        u_xx + u_yy as [M, c], what the PDE residuals consume (model_pn.py:614-617) -- e.g.
        ``sample((0, 1, "lap"))``.  Returns a tuple of outputs in the order given."""
        orders = tuple(TRACE if o == "lap" else int(o) for o in orders)
        if any(o < 0 or o > TRACE for o in orders):
            raise ValueError('orders must be in 0..3 or "lap"')
        if self._core is not None:
            return self._core.sample(list(orders))
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

    def _residual_field(self, name, v, cols):
        """A coefficient of residual(): a float (or ``cols`` floats) stays a host constant, a tensor becomes a detached
        contiguous device field [M] / [M, cols] in the means' dtype."""
        means, _, _, samples = self._require_inputs()
        M = samples.shape[0]
        if isinstance(v, torch.Tensor):
            if v.requires_grad:
                raise ValueError(f"{name}: the coefficients of residual() are constants; detach() the tensor "
                                 "(there are no gradients with respect to coefficient fields)")
            if v.device != means.device:
                raise RuntimeError(f"{name} must be a tensor on the sampler's device (no CPU fallback)")
            ok = tuple(v.shape) in ((M, cols),) + (((M,),) if cols == 1 else ())
            if not ok:
                raise ValueError(f"{name} must have shape [{M}, {cols}]" + (f" or [{M}]" if cols == 1 else "")
                                 + f", got {tuple(v.shape)}")
            return v.detach().to(means.dtype).reshape(M, cols).contiguous()
        if cols == 1 and not hasattr(v, "__len__"):
            return float(v)
        v = tuple(float(x) for x in (v if hasattr(v, "__len__") else (v,)))
        if len(v) != cols:
            raise ValueError(f"{name} must hold d = {cols} coefficients")
        return v

    def _coupling_matrix(self, name, q, c):
        """couple0 / couple_lap of residual(): c x c constants as a tuple of tuples (None: the zero matrix)."""
        if q is None:
            return tuple((0.0,) * c for _ in range(c))
        if isinstance(q, torch.Tensor) and q.requires_grad:
            raise ValueError(f"{name}: the coupling matrices of residual() are constants; detach() the tensor")
        try:
            q = tuple(tuple(float(x) for x in row) for row in q)
        except TypeError:
            raise ValueError(f"{name} must be c x c = {c} x {c} floats") from None
        if len(q) != c or any(len(row) != c for row in q):
            raise ValueError(f"{name} must be c x c = {c} x {c} floats")
        return q

    def _residual_coupled(self, a0, a1, lap, target, advect, advect_by, couple0, couple_lap, couple_weight):
        """The coupled form of residual(): every refusal, then one launch."""
        means, values, conics, samples = self._require_inputs()
        d, c, M = means.shape[1], values.shape[1], samples.shape[0]
        if couple0 is None and couple_lap is None:
            raise ValueError("couple_weight weighs couple0 / couple_lap: give at least one of the two matrices")
        if c == 1:
            raise ValueError("a one-channel field has nothing to couple: use a0 / lap")
        Q0 = self._coupling_matrix("couple0", couple0, c)
        QL = self._coupling_matrix("couple_lap", couple_lap, c)
        a1_zero = a1 is None or (not isinstance(a1, torch.Tensor)
                                 and all(float(x) == 0.0 for x in (a1 if hasattr(a1, "__len__") else (a1,))))
        if not a1_zero or advect is not None or advect_by is not None:
            raise NotImplementedError("a coupled residual() with a first-derivative (a1) or advection term is not built: "
                                      "compose it from sample((0, 1, \"lap\"))")
        f0 = self._residual_field("a0", a0, 1)
        fL = self._residual_field("lap", lap, 1)
        fW = self._residual_field("couple_weight", 1.0 if couple_weight is None else couple_weight, 1)
        if target is not None:
            if not isinstance(target, torch.Tensor) or not target.is_cuda:
                raise RuntimeError("target must be a tensor on the GPU (no CPU fallback)")
            if target.numel() != M * c:
                raise ValueError(f"target must hold M*c = {M * c} elements, got {tuple(target.shape)}")
            target = target.reshape(M, c)
        if self._core is not None:
            flat0, flatL = [0.0] * 16, [0.0] * 16          # the matrices as [4][4]
            for i in range(c):
                flat0[4 * i:4 * i + c] = Q0[i]
                flatL[4 * i:4 * i + c] = QL[i]
            fields = [v if isinstance(v, torch.Tensor) else None for v in (f0, fL, fW)]
            consts = [0.0 if isinstance(v, torch.Tensor) else v for v in (f0, fL, fW)]
            return self._core.residual_coupled(fields, consts, flat0, flatL, target)
        return _ResidualCoupledFunction.apply(means, values, conics, samples, target, ResidualCoupling(f0, fL, fW, Q0, QL),
                                              self.debug, self._plan_for(0, target), False)

    def residual(self, a0=0.0, a1=None, lap=0.0, target=None, *, advect=None, advect_by=None,
                 couple0=None, couple_lap=None, couple_weight=None):
        """Extension of the reference API: the linear residual
        ``r = a0 u + a1 . grad u + lap (u_xx + u_yy) - target`` as [M, c] in ONE launch (4 bytes per point and
        channel instead of the 28 of u, grad u and the Hessian), differentiable wrt means, values, conics (one
        launch) and ``target``.  ``a0``, ``lap``: floats; ``a1``: d floats (default zero); ``target``: [M, c]
        (or [M] for c = 1) or None.  The reference's diffusion loss in the form of test_no_mlp.py:127-144,
        ``(u - u_prev) / dt - D lap u``, is
        ``sampler.residual(a0=1 / dt, lap=-D, target=u_prev / dt).pow(2).mean()``; the model's own form
        (model_pn.py:612-617, 794-849: ``ut - dt * rhs``, the blend weighing the CURRENT level with ``time_samples``) is
        in INTEGRATION.md 4, "compute_loss with the one-launch residuals", for every problem.  Binned plans evaluate
        the backward with the wide cut-off ``q_max_backward``.

        THE GENERAL FORM (per-point coefficients and an advection term; still one launch each way):
        ``r = a0 u + a1 . grad u + lap (u_xx + u_yy) + advect (w . grad) u - target`` with
        ``w_i = sum_c' advect_by[i][c'] u_c'``.  ``a0``, ``lap``, ``advect`` also accept a tensor of M elements
        ([M] or [M, 1]) and ``a1`` a tensor [M, d]: fields per point, shared by the channels -- the reference's blend
        of two time levels with a random weight per point (model_pn.py:794-805, test_no_mlp.py:122-144).
        ``advect_by``: d x c floats; default the identity when c == d, i.e. (u . grad) u, the Burgers term.  The
        coefficients are constants (a tensor that requires grad raises ValueError); they are cast to the means' dtype
        and detached, and a field must not be modified in place between the call and its backward.  A call with
        floats only and ``advect=None`` is the linear residual above, on its own kernel.  INTEGRATION.md has the
        Burgers and trapezoid-diffusion recipes; DESIGN.md 12 the measured times against the same loss composed from
        ``sample((0, 1, "lap"))``: a training step is 19-25 % shorter, the forward alone (``no_grad``) is SLOWER
        (1.30x - 1.35x) when the coefficient fields are rebuilt in torch every step.

        THE COUPLED FORM (the channels mixed by constants; one launch each way; c >= 2):
        ``r = a0 u + lap (u_xx + u_yy) + couple_weight * (u @ couple0.T + lap_u @ couple_lap.T) - target``.
        ``couple0``, ``couple_lap``: c x c floats (nested sequences or arrays; row = output channel, column = input
        channel; a missing one is zero; constants -- a tensor that requires grad raises ValueError).  ``couple_weight``:
        a float (default 1.0) or a field of M elements, treated like ``a0`` and ``lap``, which keep their meaning.  Only
        u and the Laplacian are accumulated (2 c sums per point).  ``a1``, ``advect`` and ``advect_by`` cannot be
        combined with it (NotImplementedError: compose from ``sample()``).  The reference's wave system
        (test_no_mlp.py:127-139: ``res0 = u_t[0] - ub[1]``, ``res1 = u_t[1] - (10 lap ub[0] - 0.1 ub[1])``, ``ub`` blended
        by a random weight ``tau`` per point) is two launches::

            Q0, QL = np.array(((0, -1), (0, 0.1))), np.array(((0, 0), (-10, 0)))
            with torch.no_grad():      # the previous step's Gaussians bound to `prev`
                T = prev.residual(a0=1 / dt, couple_weight=tau, couple0=-Q0, couple_lap=-QL)
            r = cur.residual(a0=1 / dt, couple_weight=1 - tau, couple0=Q0, couple_lap=QL, target=T)
            loss = r[:, 0].pow(2).mean() + 0.01 * r[:, 1].pow(2).mean()

        INTEGRATION.md 1 has the recipe in full; DESIGN.md 14 the kernel and the measured times."""
        if couple0 is not None or couple_lap is not None or couple_weight is not None:
            return self._residual_coupled(a0, a1, lap, target, advect, advect_by, couple0, couple_lap, couple_weight)
        means, values, conics, samples = self._require_inputs()
        d, c, M = means.shape[1], values.shape[1], samples.shape[0]
        general = advect is not None or advect_by is not None or any(isinstance(v, torch.Tensor) for v in (a0, a1, lap))
        if general:
            f0 = self._residual_field("a0", a0, 1)
            f1 = self._residual_field("a1", (0.0,) * d if a1 is None else a1, d)
            fL = self._residual_field("lap", lap, 1)
            fA = self._residual_field("advect", 0.0 if advect is None else advect, 1)
            if advect_by is None:
                if advect is not None and c != d:
                    raise ValueError(f"advect with c = {c} channels in d = {d} dimensions needs advect_by (d x c floats): "
                                     "the default, the field advecting itself, exists for c == d only")
                B = tuple(tuple(1.0 if i == k else 0.0 for k in range(c)) for i in range(d))
            else:
                B = tuple(tuple(float(x) for x in row) for row in advect_by)
                if len(B) != d or any(len(row) != c for row in B):
                    raise ValueError(f"advect_by must be d x c = {d} x {c} floats")
            terms = ResidualTerms(f0, f1, fL, fA, B)
        if not general:
            a1 = (0.0,) * d if a1 is None else tuple(float(x) for x in (a1 if hasattr(a1, "__len__") else (a1,)))
            if len(a1) != d:
                raise ValueError(f"a1 must hold d = {d} coefficients")
            coeffs = (float(a0), a1[0], a1[1] if d == 2 else 0.0, float(lap))
        if target is not None:
            if not isinstance(target, torch.Tensor) or not target.is_cuda:
                raise RuntimeError("target must be a tensor on the GPU (no CPU fallback)")
            if target.numel() != M * c:
                raise ValueError(f"target must hold M*c = {M * c} elements, got {tuple(target.shape)}")
            target = target.reshape(M, c)
        if general:
            if self._core is not None:
                consts = [0.0 if isinstance(f0, torch.Tensor) else f0, 0.0, 0.0, 0.0 if isinstance(fL, torch.Tensor) else fL,
                          0.0 if isinstance(fA, torch.Tensor) else fA]
                if not isinstance(f1, torch.Tensor):
                    consts[1:1 + d] = f1
                flat = [0.0] * 8                  # advect_by as [2][4]
                for i, row in enumerate(B):
                    flat[4 * i:4 * i + c] = row
                return self._core.residual_terms([v if isinstance(v, torch.Tensor) else None for v in (f0, f1, fL, fA)],
                                                 consts, flat, target)
            want_aux = terms.advects and self._needs_backward(target)
            return _ResidualTermsFunction.apply(means, values, conics, samples, target, terms, self.debug,
                                                self._plan_for(0, target), want_aux)
        if self._core is not None:
            return self._core.residual(coeffs, target)
        return _ResidualFunction.apply(means, values, conics, samples, target, ResidualCoeffs(coeffs), self.debug,
                                       self._plan_for(0, target), False)

    def vorticity_terms(self):
        """Extension of the reference API: the seven numbers per point that the reference's Navier-Stokes problem keeps
        of orders 0..3 of its two-channel field (model_pn.py:650-659, 770-781, 848), as ONE tensor [M, 7] with the
        columns ``pigs_amd.VORTICITY_COLUMNS`` = ``(u_x, u_y, div, w, w_x, w_y, lap_w)``: the field, its divergence
        ``d_x u_x + d_y u_y``, the vorticity ``w = d_x u_y - d_y u_x``, its gradient and its Laplacian.  One launch with
        7 accumulators and 28 bytes per point, where ``sample((0, 1, 2, 3))`` carries 30 and stores 120 and a dozen
        slicing kernels follow; differentiable wrt means, values and conics in one launch.  d = 2 and c = 2 only
        (anything else raises ``NotImplementedError``).  Binned plans run it on the order-3 plan (``q_max_order3``),
        the backward with the wide cut-off.  The result is cached until the next ``preprocess`` (a result computed
        where no backward could follow -- ``no_grad`` -- is not handed to a later differentiable call: that call
        launches again).

        Take the columns with ``u_x, u_y, div, w, w_x, w_y, lap_w = t.unbind(1)``: the backward of ``unbind`` is one
        ``stack``, where seven slices ``t[:, k]`` would each scatter into a zeroed [M, 7] of their own.
        INTEGRATION.md has the Navier-Stokes recipe; DESIGN.md 13 the measured times."""
        means, values, conics, samples = self._require_inputs()
        d, c = means.shape[1], values.shape[1]
        if d != 2 or c != 2:
            raise NotImplementedError(f"vorticity_terms() needs a two-channel field in two dimensions, got d = {d}, c = {c}")
        if self._core is not None:
            return self._core.vorticity_terms()
        if self._vorticity is None or (self._needs_backward() and not self._vorticity.requires_grad):
            self._vorticity = _VorticityFunction.apply(means, values, conics, samples, None, None, self.debug,
                                                       self._plan_for(8), False)
        return self._vorticity

    def vorticity_residual(self, nu, dt, prev=None, tau=1.0, *, time_term=1.0):
        """Extension of the reference API: the Navier-Stokes residual of the reference's flagship problem (a periodic
        box in the vorticity formulation, ``compute_loss`` for ``Problem.NAVIER_STOKES``: model_pn.py:794-818, 629-631,
        830, 848-849) as ONE tensor [M, 2] with the columns ``pigs_amd.VORTICITY_RESIDUAL_COLUMNS`` = ``(div, r)``, in one
        launch forward and one backward.  With ``now`` the seven ``vorticity_terms()`` of the bound Gaussians, ``prev``
        [M, 7] the same seven of the previous time level (``None`` reads as zeros) and ``tau`` a float or a field of M
        elements ([M] or [M, 1])::

            X_b  = tau * X_now + (1 - tau) * X_prev          # X in u_x, u_y, div, w_x, w_y, lap_w
            div  = div_b
            r    = time_term * (w_now - w_prev) - dt * (nu * lap_w_b - (u_x_b * w_x_b + u_y_b * w_y_b))

        ``tau`` per point is the reference's ``TRAPEZOID`` rule, ``tau=1`` ``BACKWARD``, ``tau=0`` ``FORWARD``; the loss
        is ``out.pow(2).mean(0).sum()``.  ``time_term=0, dt=-1`` without ``prev`` gives ``r = nu lap_w - u . grad w``, the
        ``sample_pde`` of ``Model.forward`` (:655-659).  ``nu``, ``dt``, ``time_term``: floats.  ``tau`` as a tensor is
        treated like the coefficient fields of ``residual()`` (detached, cast to the means' dtype; ``requires_grad``
        raises ValueError).  ``prev`` is a constant on the device.  Differentiable wrt means, values and conics; d = 2
        and c = 2 only.  Binned plans run it on the order-3 plan (``q_max_order3``), the backward with the wide cut-off.
        The result is not cached: its arguments vary from call to call.  INTEGRATION.md 3 has the recipe (two calls
        and one line of loss); DESIGN.md 15 the kernels (the step's time against the same loss composed from
        ``vorticity_terms()`` has not been measured yet: ``tools/bench_vorticity.py`` times the two side by side)."""
        means, values, conics, samples = self._require_inputs()
        d, c, M = means.shape[1], values.shape[1], samples.shape[0]
        if d != 2 or c != 2:
            raise NotImplementedError(f"vorticity_residual() needs a two-channel field in two dimensions, got d = {d}, c = {c}")
        f_tau = self._residual_field("tau", tau, 1)
        if prev is not None:
            if not isinstance(prev, torch.Tensor) or prev.device != means.device:
                raise RuntimeError("prev must be a tensor on the sampler's device (no CPU fallback)")
            if prev.requires_grad:
                raise ValueError("prev: the previous time level of vorticity_residual() is a constant; detach() the tensor. "
                                 "When the previous level must receive a gradient, compose the residual from "
                                 "vorticity_terms() of both levels instead")
            if tuple(prev.shape) != (M, len(VORTICITY_COLUMNS)):
                raise ValueError(f"prev must have shape [{M}, {len(VORTICITY_COLUMNS)}] (the vorticity_terms() of the "
                                 f"previous time level), got {tuple(prev.shape)}")
            prev = prev.detach().to(means.dtype).contiguous()
        nu, dt, time_term = float(nu), float(dt), float(time_term)
        if self._core is not None:
            field = f_tau if isinstance(f_tau, torch.Tensor) else None
            return self._core.vorticity_residual(nu, dt, time_term, 0.0 if field is not None else f_tau, field, prev)
        return _VorticityResidualFunction.apply(means, values, conics, samples, prev, VorticityResidual(nu, dt, time_term, f_tau),
                                                self.debug, self._plan_for(8), self._needs_backward())

    def sample_gaussians(self):
        """u [M, c]"""
        return self._get(0)

    def sample_gaussians_derivative(self):
        """du/dx [M, d, c]"""
        return self._get(1)

    def sample_gaussians_laplacian(self):
        """full Hessian [M, d, d, c] (the reference's name is a misnomer: model_pn.py:614,652)"""
        return self._get(2)

    def sample_gaussians_laplacian_trace(self):
        """u_xx + u_yy [M, c]: the trace of the Hessian in its own launch (extension; 4 floats per
        point with u and grad u instead of 7, and no slicing of [M, d, d, c] in the residual)"""
        return self.sample(("lap",))[0]

    def sample_gaussians_third_derivative(self):
        """third derivatives [M, d, d, d, c]"""
        return self._get(3)

    # ------------------------------------------------------------------ neighbour aggregation
    def preprocess_aggregate(self):
        """Build the Gaussian <-> Gaussian neighbour structure for :meth:`aggregate_neighbors`
        (model_pn.py:257).  Semantics are this repo's own (parity unpinned): pigs_amd/aggregate.py."""
        from . import aggregate
        if not self.unpinned_aggregate and not GaussianSampler._warned_aggregate:
            GaussianSampler._warned_aggregate = True
            import warnings
            warnings.warn("GaussianSampler.preprocess_aggregate / aggregate_neighbors: the arithmetic of these two "
                          "methods exists only in the reference's absent CUDA source; what runs here is this "
                          "repository's own definition (pigs_amd/aggregate.py, DESIGN.md) -- a model trained with "
                          "the reference will not reproduce through it.  Pass unpinned_aggregate=True to "
                          "GaussianSampler to acknowledge.", stacklevel=2)
        if self._core is not None:
            self._core.preprocess_aggregate(-1 if self.aggregate_cap is None else self.aggregate_cap)
            self._neighbors = self._core.neighbors
            return
        self._require_inputs()
        means, conics = self._st_caller          # the caller's N Gaussians, not the periodic images
        if means.shape[1] != 2:
            raise NotImplementedError("aggregate_neighbors is implemented for d = 2")
        box = None
        if self._periodic_aggregate:
            if self._st_box is None:
                raise RuntimeError("periodic_aggregate=True: preprocess() must have run with periodic=(lo, hi)")
            # block 0 of the bound images: the wrapped centres and their conics
            N = means.shape[0]
            means, conics = self._st_inputs[0][:N], self._st_inputs[2][:N]
            box = (self._st_box[0], self._st_box[1] - self._st_box[0])
        self._neighbors = aggregate.NeighborLists(means, conics, self.q_max, cap=self.aggregate_cap, periodic=box)
        if self.debug:
            self._neighbors.check()

    def aggregate_neighbors(self, features, transform, queries, keys, frequencies, distance_transform):
        """[N, L] attention-weighted neighbour messages (model_pn.py:262-264); differentiable wrt all
        six arguments (test_neighbor_aggregation.py:89-98).  Parity unpinned: pigs_amd/aggregate.py."""
        if self._core is not None:
            return self._core.aggregate_neighbors(features, transform, queries, keys, frequencies, distance_transform)
        from . import aggregate
        if self._neighbors is None:
            raise RuntimeError("preprocess_aggregate() must be called before aggregate_neighbors()")
        return aggregate.aggregate(self._neighbors, features, transform, queries, keys, frequencies, distance_transform)

    def aggregate_neighbors_heads(self, features, transforms, queries, keys, frequencies, distance_transforms):
        """All H attention heads of a layer in one call (extension): ``out[:, h] = aggregate_neighbors(features,
        transforms[h], queries[:, h], keys[:, h], frequencies, distance_transforms[h])``.  features [N, L] and
        frequencies [F] are the heads' common part; transforms [H, L, L], queries / keys [N, H, K] (``torch.stack(...,
        dim=1)``), distance_transforms [H, L, 2E] -> [N, H, L]; ``out.reshape(N, H * L)`` is the ``torch.cat`` of the
        heads' results.  Differentiable once wrt all six arguments.  1 <= H <= 4; a shape the kernels do not admit
        raises ``NotImplementedError`` (H separate calls remain available).  pigs_amd/aggregate.py."""
        if self._core is not None:
            return self._core.aggregate_neighbors_heads(features, transforms, queries, keys, frequencies, distance_transforms)
        from . import aggregate
        if self._neighbors is None:
            raise RuntimeError("preprocess_aggregate() must be called before aggregate_neighbors_heads()")
        return aggregate.aggregate_heads(self._neighbors, features, transforms, queries, keys, frequencies,
                                         distance_transforms)
