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

This file is the facade: the public class, its documentation and the argument checks that both hosts share.  The
state and the policy live in a core -- ``_pigs_host.SamplerCore`` (csrc_host/pigs_host.cpp, the default) or
``host_ctypes.SamplerCore`` -- with one interface ("hosts").
"""
import collections
import math
import os

import torch

from . import _lib, host_ctypes
from .host_ctypes import (NETWORK_PDES, TRACE, VORTICITY_COLUMNS, VORTICITY_FIT_COLUMNS,  # noqa: F401
                          VORTICITY_RESIDUAL_COLUMNS, backward_raw, forward_raw, network_pde_width)

# what GaussianSampler.network_inputs() returns: the four arrays of the reference's Model.forward (model_pn.py:650-664)
NetworkInputs = collections.namedtuple("NetworkInputs", ("sample_u", "sample_ux", "sample_uxx", "sample_pde"))


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
    model_pn.py:11); ``"ctypes"`` is the same logic in Python over ``ctypes`` (pigs_amd/host_ctypes.py).  Both call
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
        self.unpinned_aggregate = bool(unpinned_aggregate)
        self.aggregate_cap = None if aggregate_cap is None else int(aggregate_cap)
        _lib.load()  # fail at construction, not at first use, if the HIP library is missing
        module = _load_native_host() if host == "native" else host_ctypes
        self._core = module.SamplerCore(self.debug, _FUSE_CODES[fuse], _BACKEND_CODES[backend], self.q_max,
                                        self.q_max_order3, self.q_max_backward, self.reuse_samples)
        self._core.defer_lists = self.defer_lists
        self.periodic = periodic
        self.periodic_aggregate = periodic_aggregate

    @property
    def periodic_aggregate(self):
        """Settable: whether ``preprocess_aggregate`` builds the neighbour lists of the torus (class docstring); takes
        effect at the next ``preprocess_aggregate``, on both hosts."""
        return self._core.periodic_aggregate

    @periodic_aggregate.setter
    def periodic_aggregate(self, value):
        if value and self._core.periodic is None:
            raise ValueError("periodic_aggregate=True needs periodic=(lo, hi)")
        self._core.periodic_aggregate = bool(value)

    @property
    def periodic(self):
        """Settable: None or the box (lo, hi) (class docstring); a new value takes effect at the next ``preprocess``,
        on both hosts."""
        return self._core.periodic

    @periodic.setter
    def periodic(self, value):
        box = _periodic_box(value)
        if box is None and self._core.periodic_aggregate:
            raise ValueError("periodic_aggregate=True needs periodic=(lo, hi): clear periodic_aggregate first")
        self._core.periodic = box

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
        return self._core.static_samples

    @static_samples.setter
    def static_samples(self, value):
        self._core.static_samples = bool(value)

    # the state lives in the core
    _plan = property(lambda self: self._core.plan)
    _plan3 = property(lambda self: self._core.plan3)
    _inputs = property(lambda self: self._core.inputs())
    _sample_plans = property(lambda self: self._core.sample_plans)
    _neighbors = property(lambda self: self._core.neighbors)

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
        self._core.preprocess(means, values, covariances, conics, samples)

    # ------------------------------------------------------------------ sampling
    def _require_inputs(self):
        inputs = self._core.inputs()
        if inputs is None:
            raise RuntimeError("preprocess() must be called before sampling")
        return inputs

    def sample(self, orders=(0, 1, 2)):
        """Fused entry point: one launch for all ``orders`` (extension of the reference API).
        ``orders`` holds derivative orders 0..3 and / or ``"lap"`` -- the trace of the Hessian
        u_xx + u_yy as [M, c], what the PDE residuals consume (model_pn.py:614-617) -- e.g.
        ``sample((0, 1, "lap"))``.  Returns a tuple of outputs in the order given."""
        orders = [TRACE if o == "lap" else int(o) for o in orders]
        if any(o < 0 or o > TRACE for o in orders):
            raise ValueError('orders must be in 0..3 or "lap"')
        return self._core.sample(orders)

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

    @staticmethod
    def _residual_target(target, M, c):
        """The target of residual(): None, or a device tensor of M*c elements as [M, c]."""
        if target is None:
            return None
        if not isinstance(target, torch.Tensor) or not target.is_cuda:
            raise RuntimeError("target must be a tensor on the GPU (no CPU fallback)")
        if target.numel() != M * c:
            raise ValueError(f"target must hold M*c = {M * c} elements, got {tuple(target.shape)}")
        return target.reshape(M, c)

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
        target = self._residual_target(target, M, c)
        flat0, flatL = [0.0] * 16, [0.0] * 16          # the matrices as [4][4]
        for i in range(c):
            flat0[4 * i:4 * i + c] = Q0[i]
            flatL[4 * i:4 * i + c] = QL[i]
        fields = [v if isinstance(v, torch.Tensor) else None for v in (f0, fL, fW)]
        consts = [0.0 if isinstance(v, torch.Tensor) else v for v in (f0, fL, fW)]
        return self._core.residual_coupled(fields, consts, flat0, flatL, target)

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
        if not general:
            a1 = (0.0,) * d if a1 is None else tuple(float(x) for x in (a1 if hasattr(a1, "__len__") else (a1,)))
            if len(a1) != d:
                raise ValueError(f"a1 must hold d = {d} coefficients")
            coeffs = (float(a0), a1[0], a1[1] if d == 2 else 0.0, float(lap))
        target = self._residual_target(target, M, c)
        if not general:
            return self._core.residual(coeffs, target)
        consts = [0.0 if isinstance(f0, torch.Tensor) else f0, 0.0, 0.0, 0.0 if isinstance(fL, torch.Tensor) else fL,
                  0.0 if isinstance(fA, torch.Tensor) else fA]
        if not isinstance(f1, torch.Tensor):
            consts[1:1 + d] = f1
        flat = [0.0] * 8                  # advect_by as [2][4]
        for i, row in enumerate(B):
            flat[4 * i:4 * i + c] = row
        return self._core.residual_terms([v if isinstance(v, torch.Tensor) else None for v in (f0, f1, fL, fA)],
                                         consts, flat, target)

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
        return self._core.vorticity_terms()

    def vorticity_residual(self, nu, dt, prev=None, tau=1.0, *, time_term=1.0, data=None, data_weight=1.0):
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
        ``vorticity_terms()`` has not been measured yet: ``tools/bench_vorticity.py`` times the two side by side).

        ``data`` ([M] or [M, 1] on the device; a constant, treated as ``tau`` is) adds the data term of the reference's
        Navier-Stokes loop (main_pn.py:202-212) from the same sums in the same launch: the result is [M, 3] with the
        columns ``pigs_amd.VORTICITY_FIT_COLUMNS`` = ``(div, r, fit)``, ``fit = data_weight * (w_now - data)`` with the
        vorticity of the CURRENT level.  With ``data_weight = sqrt(5)`` the step loss including ``recon_loss`` is
        ``out.pow(2).mean(0).sum()``; ``vorticity_residual(0.0, 0.0, None, 1.0, time_term=0.0, data=...)`` is the loss
        of the initialisation fit (test_initialize.py:135-136), its column 1 exact zeros.  ``pigs_amd.grid_lookup``
        makes ``data`` from an image in one launch.  There is no gradient with respect to ``data``, and the backward
        does not read it."""
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
        field = f_tau if isinstance(f_tau, torch.Tensor) else None
        if data is not None:
            if not isinstance(data, torch.Tensor):
                raise RuntimeError("data must be a tensor on the sampler's device (no CPU fallback)")
            data = self._residual_field("data", data, 1)
            return self._core._vorticity_fit(nu, dt, time_term, 0.0 if field is not None else f_tau, field, prev, data,
                                             float(data_weight))
        return self._core.vorticity_residual(nu, dt, time_term, 0.0 if field is not None else f_tau, field, prev)

    def network_inputs(self, pde, nu=0.0, wave=(10.0, 0.1)):
        """Extension of the reference API: the four arrays that the reference's ``Model.forward`` samples at its
        Gaussians' means under ``no_grad`` and hands to its dynamics network (model_pn.py:645-664), in ONE launch and
        in the layouts of those lines, as the named tuple ``(sample_u, sample_ux, sample_uxx, sample_pde)``::

            sample_u   [M, c]     u
            sample_ux  [M, 2c]    sample_ux[m, i*c + ch] = d_i u_ch      (sample_gaussians_derivative().reshape(M, -1))
            sample_uxx [M, 2c]    u_xx of every channel, then u_yy       (the cat of :664: planar, not interleaved)
            sample_pde [M, p]     pde_rhs (:612-631) by ``pde``

        ``pde`` is one of ``pigs_amd.NETWORK_PDES``: ``"zero"`` (Problem.TEST; p = c), ``"diffusion"`` (``u_xx + u_yy``;
        p = c), ``"burgers"`` (``nu (u_xx + u_yy) - u_ch d_x u_ch``, channel by channel as the reference's broadcast
        does; p = c), ``"wave"`` (``(u_1, wave[0] (u_xx + u_yy)_0 - wave[1] u_1)``; c = 2, p = 2) and
        ``"navier_stokes"`` (``nu lap w - (u_0 w_x + u_1 w_y)`` with ``w = d_x u_y - d_y u_x``; c = 2, p = 1).  The
        kernel accumulates only what these need -- 5 c sums per point, 13 for Navier-Stokes, where orders 0..3 carry
        30 at c = 2 -- and composes ``sample_pde`` once per point, so none of the reference's slicing, stacking and
        ``cat`` kernels follow.  The four tensors are contiguous views of one allocation and go straight into
        ``FusedInputTransform.forward`` / ``.transform_gaussians``.

        Forward only: the model calls it under ``no_grad``, and the outputs never require a gradient, whatever the
        bound tensors do.  No autograd node, no host wait, scratch from torch: it records into a ``GraphedStep``.
        d = 2 only; dense float32 / float64 with c = 1..4, binned float32 with c <= 2 (Navier-Stokes on the order-3
        plan, ``q_max_order3``); periodic samplers included.  M = 0 or N = 0 returns zeros of the right shapes without a
        launch.  Anything else raises ``NotImplementedError`` by name.  INTEGRATION.md 4 has the time step it belongs
        to; DESIGN.md 25 the kernels."""
        means, values, conics, samples = self._require_inputs()
        if pde not in NETWORK_PDES:
            raise ValueError(f"pde must be one of {NETWORK_PDES}, got {pde!r}")
        kind = NETWORK_PDES.index(pde)
        d, c = means.shape[1], values.shape[1]
        if d != 2:
            raise NotImplementedError(f"network_inputs() is implemented for d = 2 (the reference's model), got d = {d}")
        if pde in ("wave", "navier_stokes") and c != 2:
            raise NotImplementedError(f"network_inputs(pde={pde!r}) needs a two-channel field, got c = {c}")
        try:
            w0, w1 = (float(x) for x in wave)
        except (TypeError, ValueError):
            raise ValueError(f"wave must be two floats, got {wave!r}") from None
        return NetworkInputs(*self._core._network_inputs(kind, float(nu), w0, w1))

    def sample_gaussians(self):
        """u [M, c]"""
        return self._core.get(0)

    def sample_gaussians_derivative(self):
        """du/dx [M, d, c]"""
        return self._core.get(1)

    def sample_gaussians_laplacian(self):
        """full Hessian [M, d, d, c] (the reference's name is a misnomer: model_pn.py:614,652)"""
        return self._core.get(2)

    def sample_gaussians_laplacian_trace(self):
        """u_xx + u_yy [M, c]: the trace of the Hessian in its own launch (extension; 4 floats per
        point with u and grad u instead of 7, and no slicing of [M, d, d, c] in the residual)"""
        return self.sample(("lap",))[0]

    def sample_gaussians_third_derivative(self):
        """third derivatives [M, d, d, d, c]"""
        return self._core.get(3)

    # ------------------------------------------------------------------ neighbour aggregation
    def preprocess_aggregate(self):
        """Build the Gaussian <-> Gaussian neighbour structure for :meth:`aggregate_neighbors`
        (model_pn.py:257).  Semantics are this repo's own (parity unpinned): pigs_amd/aggregate.py."""
        if not self.unpinned_aggregate and not GaussianSampler._warned_aggregate:
            GaussianSampler._warned_aggregate = True
            import warnings
            warnings.warn("GaussianSampler.preprocess_aggregate / aggregate_neighbors: the arithmetic of these two "
                          "methods exists only in the reference's absent CUDA source; what runs here is this "
                          "repository's own definition (pigs_amd/aggregate.py, DESIGN.md) -- a model trained with "
                          "the reference will not reproduce through it.  Pass unpinned_aggregate=True to "
                          "GaussianSampler to acknowledge.", stacklevel=2)
        self._core.preprocess_aggregate(-1 if self.aggregate_cap is None else self.aggregate_cap)

    def aggregate_neighbors(self, features, transform, queries, keys, frequencies, distance_transform):
        """[N, L] attention-weighted neighbour messages (model_pn.py:262-264); differentiable wrt all
        six arguments (test_neighbor_aggregation.py:89-98).  Parity unpinned: pigs_amd/aggregate.py."""
        return self._core.aggregate_neighbors(features, transform, queries, keys, frequencies, distance_transform)

    def aggregate_neighbors_heads(self, features, transforms, queries, keys, frequencies, distance_transforms):
        """All H attention heads of a layer in one call (extension): ``out[:, h] = aggregate_neighbors(features,
        transforms[h], queries[:, h], keys[:, h], frequencies, distance_transforms[h])``.  features [N, L] and
        frequencies [F] are the heads' common part; transforms [H, L, L], queries / keys [N, H, K] (``torch.stack(...,
        dim=1)``), distance_transforms [H, L, 2E] -> [N, H, L]; ``out.reshape(N, H * L)`` is the ``torch.cat`` of the
        heads' results.  Differentiable once wrt all six arguments.  1 <= H <= 4; a shape the kernels do not admit
        raises ``NotImplementedError`` (H separate calls remain available).  pigs_amd/aggregate.py."""
        return self._core.aggregate_neighbors_heads(features, transforms, queries, keys, frequencies, distance_transforms)
