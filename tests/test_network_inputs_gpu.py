"""GPU: GaussianSampler.network_inputs() (pair_math.h ORDI / ORDJ, pigs_network_inputs_forward) -- the four arrays of the
reference's Model.forward (model_pn.py:645-664) in one launch -- against the float64 recipe of
tests/test_network_inputs.py (oracle/dense_numpy.forward orders 0..3 plus the five pde_rhs lines).

The bars, per array, both errors against that float64 recipe on the inputs as the kernel sees them:
    float64   err <= 1e-11 x scale                              (tests/test_model_loss_gpu.py)
    float32   err <= 4 err_torch32 + 1e-5 x scale               (tests/test_step_gpu.py for sampler outputs)
err_torch32 is the error of the same recipe in float32 torch on the CPU (oracle/dense_torch.py); ``scale`` is the largest
entry of the sum of the absolute terms of a composed value over the oracle's absolute=True pair sums
(test_network_inputs.scales), so that a sum that cancels is not measured against its own smallness.  The binned scenes of
tests/test_binned_matrix_gpu.py are held as that file holds them: within TOL = 1e-5 of the term scale built from the
largest entry of every order (their pairs beyond the cut-off are below that), because the pair sums of 18 M pairs at
order 3 do not fit a test.  Every case prints its worst err / allowance.
"""
import ctypes

import numpy as np
import pytest
import torch

import host_program as hp
import test_network_inputs as tn
from test_network_inputs import NAMES, ORDI, ORDJ, PDES, WAVE, flat_conics, full_conics, recipe, scales

pytestmark = pytest.mark.gpu
BAR64, FLOOR32 = 1e-11, tn.FLOOR32
HOSTS = ("native", "ctypes")


def round32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def sampler_of(backend="dense", host_="native", debug=True, **kw):
    from diff_gaussian_sampling import GaussianSampler
    return GaussianSampler(debug, backend=backend, host=host_, **kw)


class Reference:
    """One scene (means, full conics, values, points; float64) as a float32 or a float64 kernel sees it: the float64
    recipe per right-hand side, the float32 torch recipe and the scales, each computed once and never changed."""

    def __init__(self, means, conics_full, values, points, f32):
        rnd = round32 if f32 else (lambda a: np.asarray(a, dtype=np.float64))
        self.f32 = f32
        self.means, self.flat, self.values, self.points = rnd(means), rnd(flat_conics(conics_full)), rnd(values), rnd(points)
        full = full_conics(self.flat)
        self.out = tn.oracle_outputs(self.means, full, self.values, self.points)
        self.mag = tn.oracle_outputs(self.means, full, self.values, self.points, absolute=True)
        self.out32 = None
        self._want, self._ref32 = {}, {}

    def want(self, pde, nu):
        if (pde, nu) not in self._want:
            self._want[pde, nu] = recipe(self.out, pde, nu=nu, wave=WAVE)
        return self._want[pde, nu]

    def ref32(self, pde, nu):
        from oracle import dense_torch
        if self.out32 is None:
            t = [torch.as_tensor(a, dtype=torch.float32) for a in (self.means, self.flat, self.values, self.points)]
            self.out32 = dense_torch.forward(*t, orders=(0, 1, 2, 3))
        if (pde, nu) not in self._ref32:
            self._ref32[pde, nu] = {k: v.double().numpy() for k, v in recipe(self.out32, pde, nu=nu, wave=WAVE).items()}
        return self._ref32[pde, nu]

    def scale(self, pde, nu):
        return {k: float(v.max()) if v.size else 0.0 for k, v in scales(self.mag, pde, nu=nu, wave=WAVE).items()}

    def tensors(self, grad=False):
        dt = torch.float32 if self.f32 else torch.float64
        means, values, flat, points = (dev(a, dt) for a in (self.means, self.values, self.flat, self.points))
        for t in (means, values, flat):
            t.requires_grad_(grad)
        return means, values, flat, points

    def hold(self, what, got, pde, nu):
        """the bar of the module text; returns the worst err / allowance"""
        want, sc = self.want(pde, nu), self.scale(pde, nu)
        ref32 = self.ref32(pde, nu) if self.f32 else None
        worst, bad = 0.0, []
        for k, g in zip(NAMES, got):
            assert g.is_contiguous() and not g.requires_grad and tuple(g.shape) == want[k].shape, (what, k, tuple(g.shape))
            g = host(g)
            assert np.isfinite(g).all(), (what, k)
            err = float(np.abs(g - want[k]).max()) if g.size else 0.0
            allow = 4.0 * float(np.abs(ref32[k] - want[k]).max()) + FLOOR32 * sc[k] if self.f32 else BAR64 * sc[k]
            ratio = err / allow if allow > 0 else (0.0 if err == 0 else float("inf"))
            worst = max(worst, ratio)
            if not err <= allow:
                bad.append(f"{k}: err {err:.3g}, allowance {allow:.3g}, scale {sc[k]:.3g}")
        print(f"[figure] {what}: worst err / allowance = {worst:.3g}")
        assert not bad, f"{what}: " + "; ".join(bad)
        return worst


_references = {}


def recorded(name, f32):
    """the Reference of a recorded fixture or of the first M = N record of a trace; (reference, pde, nu)"""
    if (name, f32) not in _references:
        if name in tn.FIXTURES:
            means, conics, values, _ = tn.load_recorded(name)
        else:
            means, conics, values, _ = tn.load_trace_records(name)[0]
        _references[name, f32] = Reference(means, conics, values, means, f32)
    pde, nu = tn.FIXTURES.get(name) or tn.TRACES[name]
    return _references[name, f32], pde, nu


def seeded(c, f32, N=97, M=None, seed=5):
    key = ("seeded", c, f32, N, M, seed)
    if key not in _references:
        means, conics, values = tn.seeded_scene(c, N=N, seed=seed)
        points = means if M is None else np.random.default_rng(seed + 1).uniform(-1, 1, (M, 2))
        _references[key] = Reference(means, conics, values, points, f32)
    return _references[key]


def run(s, ref, pde, nu):
    means, values, flat, points = ref.tensors()
    s.preprocess(means, values, None, flat, points)
    return s.network_inputs(pde, nu=nu, wave=WAVE)


# ---- the recordings -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_", HOSTS)
@pytest.mark.parametrize("variant", ["dense float64", "dense float32", "binned float32"])
@pytest.mark.parametrize("name", sorted(tn.FIXTURES) + sorted(tn.TRACES))
def test_the_recorded_forwards(hip_lib, name, variant, host_):
    f32 = variant != "dense float64"
    ref, pde, nu = recorded(name, f32)
    s = sampler_of("binned" if variant.startswith("binned") else "dense", host_)
    got = run(s, ref, pde, nu)
    assert (s._plan is not None) == variant.startswith("binned")
    assert type(got).__name__ == "NetworkInputs" and got._fields == NAMES
    ref.hold(f"{name}, {variant}, {host_}", got, pde, nu)


# ---- every dense instantiation through every launch variant it can take -------------------------------------
def dense_cases():
    """(dtype, c, mask, variant, N, M): the smallest shapes on the edges that choose_dense_forward reports -- rows with
    more than one chunk of Gaussians and a ragged last block of 16 points; w16 just past the 256 blocks that rows takes,
    with a ragged last block; w4 below the 64 Gaussians that w16 asks for, N no multiple of the four-record step, M
    three blocks with a ragged last one (the direct store of the four-wave kernel)."""
    return [(dtype, c, mask, variant) for (dtype, c, mask), variants in tn.VARIANTS.items() for variant in variants]


@pytest.mark.parametrize("dtype,c,mask,variant", dense_cases(), ids=[f"{dt}-c{c}-{mask}-{v}" for dt, c, mask, v in dense_cases()])
def test_every_dense_instantiation_in_every_variant(hip_lib, dtype, c, mask, variant):
    if variant == "rows":
        N, M = hp.dense(dtype, 2, c, mask, 1600, 1600).rows_chunk + 37, 37
    elif variant == "w16":
        N, M = 70, 64 * 256 + 65
    else:
        N, M = 37, 130
    assert hp.dense(dtype, 2, c, mask, N, M).forward == variant
    ref = seeded(c, dtype == "float32", N=N, M=M, seed=N + M)
    s = sampler_of("dense")
    for pde, nu in ((("navier_stokes", 0.05),) if mask == ORDJ else (("burgers", 0.05),) + ((("wave", 0.0),) if c == 2 else ())):
        ref.hold(f"{dtype} c={c} mask {mask} {variant} {N} x {M} {pde}", run(s, ref, pde, nu), pde, nu)


# ---- every binned instantiation in every tile mode ----------------------------------------------------------
def binned_cases():
    from test_binned_matrix_gpu import SCENES
    cases = []
    for name in SCENES:
        for c, pde in ((1, "burgers"), (2, "burgers"), (2, "navier_stokes")):
            if name == "P-stride" and (c, pde) == (2, "burgers"):
                continue                  # the trip through the helper waves does not depend on the template
            cases.append((name, c, pde))
    return cases


@pytest.mark.parametrize("name,c,pde", binned_cases(), ids=[f"{n}-c{c}-{p}" for n, c, p in binned_cases()])
def test_every_binned_instantiation_in_every_tile_mode(hip_lib, name, c, pde):
    from test_binned_matrix_gpu import TOL, assert_mode, scene
    cs = scene(name, c).on_device((name, c, "network inputs", pde))
    nu = 0.05
    s = cs.sampler()
    if pde == "navier_stokes":
        # the order-3 plan in full, as a differentiable call builds it: network_inputs() alone would build it for the
        # forward only, without the backward's tile lists that assert_mode reads for L-sorted
        s.vorticity_terms()
    with torch.no_grad():
        got = s.network_inputs(pde, nu=nu, wave=WAVE)
    counts = assert_mode(cs, s._plan3 if pde == "navier_stokes" else s._plan, hip_lib, s)
    want = recipe(cs.exp, pde, nu=nu, wave=WAVE)
    # the term scale from the largest entry of every order, as that file's check_output / check_columns take it
    top = {o: np.full_like(cs.exp[o], np.abs(cs.exp[o]).max()) for o in range(4)}
    sc = {k: float(v.max()) for k, v in scales(top, pde, nu=nu, wave=WAVE).items()}
    worst = 0.0
    for k, g in zip(NAMES, got):
        assert tuple(g.shape) == want[k].shape and np.isfinite(host(g)).all(), k
        worst = max(worst, float(np.abs(host(g) - want[k]).max()) / (TOL * sc[k]))
    print(f"[figure] binned {name} c={c} {pde}: tiles in LIST / RANGES / GROUPS / POINTS {counts}: worst err / (1e-5 x scale) = {worst:.3f}")
    assert worst <= 1.0


# ---- equal to the composition -------------------------------------------------------------------------------
@pytest.mark.parametrize("pde,c", [(p, c) for p in PDES for c in ((2,) if p in ("wave", "navier_stokes") else (1, 2, 3, 4))])
def test_equal_to_the_composition_of_the_sampled_orders(hip_lib, pde, c):
    """sample((0, 1, 2, 3)) and the reference's torch lines on the GPU, the best composition before this operator, stand
    where err_torch32 stands in the bar"""
    ref, nu = seeded(c, True), 0.05
    s = sampler_of("dense")
    means, values, flat, points = ref.tensors()
    with torch.no_grad():
        s.preprocess(means, values, None, flat, points)
        composed = recipe(dict(enumerate(s.sample((0, 1, 2, 3)))), pde, nu=nu, wave=WAVE)
        got = s.network_inputs(pde, nu=nu, wave=WAVE)
    want, sc = ref.want(pde, nu), ref.scale(pde, nu)
    worst = 0.0
    for k, g in zip(NAMES, got):
        assert tuple(g.shape) == tuple(composed[k].shape), k
        allow = 4.0 * float(np.abs(host(composed[k]) - want[k]).max()) + FLOOR32 * sc[k]
        err = float(np.abs(host(g) - want[k]).max())
        worst = max(worst, err / allow if allow > 0 else float(err > 0))
        assert err <= allow, (pde, c, k, err, allow)
    print(f"[figure] {pde} c={c}: against the composition, worst err / allowance = {worst:.3g}")


# ---- a periodic sampler -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["dense float64", "dense float32", "binned float32"])
def test_a_periodic_sampler_on_another_box(hip_lib, variant):
    """the box (0.5, 2.5): the float64 recipe over the nine images of every Gaussian, sampled at the wrapped means"""
    f32 = variant != "dense float64"
    lo, hi, N = 0.5, 2.5, 83
    L = hi - lo
    key = ("periodic", f32)
    rng = np.random.default_rng(11)
    means = rng.uniform(lo, hi, (N, 2))
    sig = 0.09 * np.exp(rng.normal(0, 0.2, (N, 2)))
    rho = rng.uniform(-0.6, 0.6, N)
    det = (sig[:, 0] * sig[:, 1]) ** 2 * (1 - rho ** 2)
    flat = np.stack((sig[:, 1] ** 2 / det, -rho * sig[:, 0] * sig[:, 1] / det, sig[:, 0] ** 2 / det), -1)
    values = rng.uniform(-1, 1, (N, 2))
    rnd = round32 if f32 else np.asarray
    means, flat, values = rnd(means), rnd(flat), rnd(values)
    if key not in _references:
        shifts = np.array([(i * rnd(L), j * rnd(L)) for i in (-1, 0, 1) for j in (-1, 0, 1)])
        img_means = (means[None] + shifts[:, None]).reshape(-1, 2)
        ref = Reference(img_means, full_conics(np.tile(flat, (9, 1))), np.tile(values, (9, 1)), means, False)
        ref.f32 = f32
        _references[key] = ref
    ref = _references[key]
    dt = torch.float32 if f32 else torch.float64
    s = sampler_of("binned" if variant.startswith("binned") else "dense", periodic=(lo, hi))
    s.preprocess(dev(means, dt), dev(values, dt), None, dev(flat, dt), dev(means, dt))
    for pde, nu in (("navier_stokes", 0.05), ("burgers", 0.05)):
        ref.hold(f"periodic ({lo}, {hi}), {variant}, {pde}", s.network_inputs(pde, nu=nu), pde, nu)


# ---- canaries, degenerate shapes, no gradient ---------------------------------------------------------------
@pytest.mark.parametrize("pde,c,binned", [("burgers", 3, False), ("wave", 2, False), ("navier_stokes", 2, False),
                                          ("diffusion", 1, False), ("wave", 2, True), ("navier_stokes", 2, True),
                                          ("diffusion", 1, True)])
def test_nothing_is_written_behind_the_four_outputs(hip_lib, pde, c, binned):
    """through the C ABI, every output in the middle of a buffer of canaries (the binned kernels: c <= 2)"""
    from pigs_amd import _lib
    ref = seeded(c, True, N=97, M=203, seed=9)
    means, values, flat, points = ref.tensors()
    M, pad, canary = 203, 64, -777.0
    widths = (c, 2 * c, 2 * c, 2 if pde == "wave" else 1 if pde == "navier_stokes" else c)
    bufs = [torch.full((M * w + 2 * pad,), canary, device="cuda") for w in widths]
    outs = [ctypes.c_void_p(b.data_ptr() + 4 * pad) for b in bufs]
    pw = (ctypes.c_void_p(0), 0, ctypes.c_void_p(0), 0)
    if binned:
        s = sampler_of("binned")
        with torch.no_grad():
            s.preprocess(means, values, None, flat, points)
            s.network_inputs(pde, nu=0.05)           # builds the plan this right-hand side runs on
        plan = s._plan3 if pde == "navier_stokes" else s._plan
        pw = (ctypes.c_void_p(plan.workspace.data_ptr()), plan.workspace.numel(),
              ctypes.c_void_p(plan.samples.workspace.data_ptr()), plan.samples.workspace.numel())
    params = _lib.PigsNetworkInputs(PDES.index(pde), 0.05, WAVE)
    rc = hip_lib.pigs_network_inputs_forward(0, 2, c, 97, M, *(ctypes.c_void_p(t.data_ptr()) for t in (means, flat, values, points)),
                                             ctypes.byref(params), *outs, *pw, _lib.stream(means.device))
    assert rc == 0
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:pad] == canary).all()) and bool((b[-pad:] == canary).all())
    ref.hold(f"C ABI {pde} c={c} binned={binned}", [b[pad:-pad].view(M, w) for b, w in zip(bufs, widths)], pde, 0.05)


@pytest.mark.parametrize("host_", HOSTS)
def test_degenerate_shapes_and_no_gradient(hip_lib, host_):
    s = sampler_of("dense", host_)
    z = lambda *shape: torch.zeros(shape, device="cuda")      # noqa: E731
    for N, M in ((0, 5), (5, 0), (0, 0)):
        s.preprocess(z(N, 2), z(N, 2), None, torch.ones(N, 3, device="cuda"), z(M, 2))
        for pde, p in (("burgers", 2), ("wave", 2), ("navier_stokes", 1), ("zero", 2)):
            got = s.network_inputs(pde, nu=0.1)
            assert [tuple(t.shape) for t in got] == [(M, 2), (M, 4), (M, 4), (M, p)], (N, M, pde)
            assert all(not bool(t.any()) for t in got)
    ref = seeded(2, True)
    means, values, flat, points = ref.tensors(grad=True)
    s.preprocess(means, values, None, flat, points)
    got = s.network_inputs("navier_stokes", nu=0.05)                      # grad mode on, leaves that require grad
    assert all(not t.requires_grad and t.grad_fn is None for t in got)
    ref.hold(f"leaves that require grad, {host_}", got, "navier_stokes", 0.05)
    with pytest.raises(ValueError):
        s.network_inputs("poisson")
    s.preprocess(means[:, :1].detach().contiguous(), values.detach(), None, flat[:, :1].detach().contiguous(), points[:, :1].contiguous())
    with pytest.raises(NotImplementedError, match="d = 2"):
        s.network_inputs("diffusion")
    s.preprocess(means.detach(), values[:, :1].detach().contiguous(), None, flat.detach(), points)
    with pytest.raises(NotImplementedError, match="two-channel"):
        s.network_inputs("wave")


# ---- capture ------------------------------------------------------------------------------------------------
def _transform_of(name):
    import pigs_amd
    import test_input_transform as ti
    from test_input_transform_gpu import module_of
    rows, params, w, _ = ti.load_fixture(name)
    c, p = rows[2].shape[1], rows[7].shape[1]
    params = [round32(a) for a in params]
    return rows, params, pigs_amd.FusedInputTransform.from_module(module_of(params, c, p))


def test_preprocess_network_inputs_and_the_input_transform_in_one_graphed_step(hip_lib):
    """three replays after in-place changes of the Gaussians against the eager call on the same values"""
    from pigs_amd.graphs import GraphedStep
    rows, _, net = _transform_of("navier_stokes")
    ref, pde, nu = recorded("navier_stokes", True)
    s = sampler_of("dense", debug=False)

    def fn(means, u, flat, cov, bnd):
        with torch.no_grad():
            s.preprocess(means, u, None, flat, means)
            ni = s.network_inputs(pde, nu=nu)
            return (net(means, cov, u, bnd, *ni),) + tuple(ni)

    def make_inputs():
        means, values, flat, _ = ref.tensors()
        return means, values, flat, dev(rows[1]), dev(rows[3])
    step = GraphedStep(fn, make_inputs, warmup=2)
    rng = np.random.default_rng(3)
    equal = True
    for k in range(3):
        with torch.no_grad():
            step.inputs[0].add_(dev(rng.normal(0, 0.01, ref.means.shape)))
            step.inputs[1].mul_(1.0 + 0.1 * (k + 1))
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        eager = fn(*(t.clone() for t in step.inputs))
        for a, b in zip(got, eager):
            assert float((a - b).abs().max()) <= FLOOR32 * float(b.abs().max()), k
            equal = equal and torch.equal(a, b)
        assert float(got[0].abs().max()) > 0
    print(f"[figure] graphed step: three replays, bits equal to the eager call: {equal}")


@pytest.mark.parametrize("name", sorted(tn.FIXTURES))
def test_t_params_of_the_recorded_step_from_the_hip_inputs(hip_lib, name):
    """the recorded Gaussians through network_inputs() and FusedInputTransform: t_params against the float64 chain
    (recipe + tests/test_input_transform.py oracle) under err_hip <= 4 err_torch32 + 1e-6 scale, err_torch32 that of the
    same chain in float32 torch on the GPU"""
    import test_input_transform as ti
    from oracle import dense_torch
    rows, params, net = _transform_of(name)
    ref, pde, nu = recorded(name, True)
    rows = [round32(a) for a in rows]
    rows[0] = ref.means

    def chain(dtype, device):
        t = [torch.as_tensor(a, dtype=dtype, device=device) for a in (ref.means, ref.flat, ref.values, ref.points)]
        ni = recipe(dense_torch.forward(*t, orders=(0, 1, 2, 3)), pde, nu=nu, wave=WAVE)
        trows = [torch.as_tensor(a, dtype=dtype, device=device) for a in rows[:4]] + [ni[k] for k in NAMES]
        return host(ti.oracle(trows, [torch.as_tensor(a, dtype=dtype, device=device) for a in params])[2])
    want, ref32 = chain(torch.float64, "cpu"), chain(torch.float32, "cuda")
    s = sampler_of("dense")
    with torch.no_grad():
        got = host(net(*(dev(a) for a in rows[:4]), *run(s, ref, pde, nu))[0])
    assert got.shape == want.shape
    err_h, err_t, scale = np.abs(got - want).max(), np.abs(ref32 - want).max(), ti.scale_of(want)
    print(f"[figure] {name}: t_params hip {err_h:.3g}, torch32 {err_t:.3g}, scale {scale:.3g}: "
          f"ratio {err_h / (4.0 * err_t + 1e-6 * scale):.3f}")
    assert err_h <= 4.0 * err_t + 1e-6 * scale
