"""GPU: ``Model.compute_loss`` through the one-launch operators of ``GaussianSampler``, against the float64 recipe of
tests/test_model_loss.py on the recorded scenes of tests/golden/model_pn_loss/*.npz (fixtures only; the reference
is never read here).

``HipOps`` hands the arguments that ``test_model_loss.loss_recipe`` builds to the sampler: ``residual()`` with fields and
advection (DIFFUSION, BURGERS; under FORWARD / BACKWARD some coefficients are floats, DIFFUSION then runs the linear
kernel), the coupled ``residual()`` on both levels (WAVE), ``vorticity_terms()`` of the previous level and
``vorticity_residual()`` (NAVIER_STOKES, the plain sampler, as recorded; tau the floats 0.0 / 1.0 under FORWARD /
BACKWARD), ``sample_gaussians()`` on the boundary points, ``sample((0, 1, "lap"))`` for the previous level's fields.
One sampler serves both levels and both point sets, as the model's does.

The bar, in the form of tests/test_step_gpu.py, for the residual, the two losses and the three gradients:

    float32     err_hip <= 4 err_torch32 + 1e-5 x scale       both errors against the float64 recipe on the same
                                                              (float32-valued) inputs; err_torch32: the same recipe from
                                                              float32 torch ops on the GPU; 1e-5: the sampler's tolerance
    float64     err_hip <= 1e-11 x scale                      the float64 bar of tests/test_residual_terms_gpu.py

scale = the largest entry of the float64 result.  Every case prints its worst ratio.

  1. 12 scenes x {dense float32, dense float64, binned float32} x {native, ctypes};
  2. the seam: one whole training iteration on the two step fixtures -- ``HipOps.step`` of tests/test_step_gpu.py, the
     new state's free rows bound to M = 100 seeded points, the PDE loss of the recipe (TRAPEZOID, a seeded tau per
     point) against the INCOMING level as ``prev``, plus the weighted penalty, ``torch.autograd.grad`` to every network
     parameter, to t_params and to the state -- against ``test_step.step_oracle`` followed by the recipe in float64;
     both head routes, both hosts;
  3. capture: the same iteration in one ``GraphedStep``, replayed twice on new tau and new points copied into the static
     inputs, held to the bar against the oracle; against the eager iteration on the same inputs its forward outputs are
     bit-equal (the distance of the gradients, which come through atomics, is printed);
  4. determinism: the forward outputs of two runs on the dense path are bit-equal.

MEASURED (MI355X), worst err_hip / allowance per case (DESIGN.md section 23 has the table): the twelve scenes 0.015 -
0.060 dense float32, 0.024 - 0.083 binned float32, 4.8e-5 - 3.7e-4 dense float64 (the hosts agree to the digits shown);
one training iteration 0.30 - 0.47; the graphed iteration's replays 0.25 - 0.68, their gradients 0.29 - 0.87 of one
allowance from the eager iteration's.  No case found a defect in a kernel or a host.
"""
import numpy as np
import pytest
import torch

import test_model_loss as tl
import test_step as ts
from test_model_loss import CHECKED, FLOOR, OracleOps, RULES, SCENES, allowance, errors, loss_recipe, loss_oracle, run_recipe

pytestmark = pytest.mark.gpu

HOSTS = ("native", "ctypes")
PATHS = (("dense", torch.float32), ("dense", torch.float64), ("binned", torch.float32))
F64_BAR = 1e-11
FORWARD_OUTPUTS = ("residual", "pde_loss", "bc_loss")
SEAM = ("diffusion", "navier_stokes")      # the step fixtures; each takes the recipe of its name
SEAM_M, SEAM_DT = 100, 0.25
SEAM_FORWARD = ("deltas", "penalty", "residual", "pde_loss", "loss")


class HipOps:
    """The operators of test_model_loss.OracleOps through the library: bind the level to the points, one call."""

    def __init__(self, host="native", backend="dense", sampler=None):
        from diff_gaussian_sampling import GaussianSampler
        self.sampler = GaussianSampler(False, backend=backend, host=host) if sampler is None else sampler

    def bind(self, level, points):
        self.sampler.preprocess(level[0], level[1], None, level[2], points)
        return self.sampler

    def fields(self, level, points):
        return self.bind(level, points).sample((0, 1, "lap"))

    def u(self, level, points):
        return self.bind(level, points).sample_gaussians()

    def residual(self, level, points, **kw):
        return self.bind(level, points).residual(**kw)

    def vorticity_terms(self, level, points):
        return self.bind(level, points).vorticity_terms()

    def vorticity_residual(self, level, points, nu, dt, prev, tau, time_term=1.0):
        return self.bind(level, points).vorticity_residual(nu, dt, prev, tau, time_term=time_term)


def hold(what, got, want, single=None, keys=CHECKED):
    """the bar of the module text; ``single`` None: the float64 bar.  Returns the worst err_hip / allowance."""
    e_hip = errors(got, want, keys)
    e_t = None if single is None else errors(single, want, keys)
    worst, bad = 0.0, []
    for k in keys:
        assert tuple(got[k].shape) == tuple(want[k].shape), (what, k, tuple(got[k].shape), tuple(want[k].shape))
        allowed = F64_BAR * e_hip[k][1] if single is None else allowance(e_t[k][0], e_hip[k][1])
        ratio = e_hip[k][0] / allowed
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad.append(f"{k}: hip {e_hip[k][0]:.3g}, torch32 {'-' if single is None else format(e_t[k][0], '.3g')}, "
                       f"scale {e_hip[k][1]:.3g}, ratio {ratio:.3g}")
    print(f"[figure] {what}: worst err_hip / allowance = {worst:.3g}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return worst


_single = {}


def torch32(problem, rule):
    """the recipe from float32 torch ops on the GPU: computed once per scene, shared"""
    if (problem, rule) not in _single:
        _single[(problem, rule)] = run_recipe(loss_oracle(problem, rule)[0], OracleOps(), torch.float32, "cuda")
    return _single[(problem, rule)]


# ---- 1. the twelve scenes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend,dtype", PATHS, ids=["dense-f32", "dense-f64", "binned-f32"])
@pytest.mark.parametrize("problem,rule", SCENES)
def test_compute_loss_through_the_operators(hip_lib, problem, rule, backend, dtype, host):
    scene, want = loss_oracle(problem, rule)
    ops = HipOps(host, backend)
    got = run_recipe(scene, ops, dtype, "cuda")
    assert (ops.sampler._plan is not None) == (backend == "binned")
    assert all(got[k].dtype == dtype for k in CHECKED if k != "bc_loss" or problem != "navier_stokes")
    hold(f"{problem} {rule}, {backend} {str(dtype)[6:]}, host {host}", got, want,
         torch32(problem, rule) if dtype == torch.float32 else None)


# ---- 2. the seam: step, loss, one backward ------------------------------------------------------------------
def seam_inputs(name, k=0):
    """M = 100 collocation points and a tau per point, seeded per fixture and draw ``k``, float32-valued"""
    rng = np.random.default_rng(1000 + 10 * len(name) + k)
    return ts.as_float32(rng.uniform(-1.0, 1.0, (SEAM_M, 2))), ts.as_float32(rng.uniform(0.05, 0.95, SEAM_M))


def run_iteration(scene, step_ops, loss_ops, net, dtype=torch.float64, device="cpu", tensors=None, points=None, tau=None):
    """One training iteration on a step fixture: the step, the recipe's PDE loss (TRAPEZOID) of the new state's free rows
    against the incoming level, the weighted penalty, and the gradient of their sum with respect to every parameter of
    the network, to t_params and to the state."""
    x = ts.scene_tensors(scene, dtype, device) if tensors is None else tensors
    if points is None:
        points, tau = (torch.as_tensor(a, dtype=dtype, device=device) for a in seam_inputs(scene.name))
    fx = tl.load_fixture(scene.name)
    nb = scene.n_boundary
    s = step_ops.step(net, x.t_params[0], *x.state, x.mask, scene.wrap, 0)
    with torch.no_grad():
        conics_in = ts.flat_covariances(x.state[2], x.state[3])[1]
        prev = (x.state[0][nb:].clone(), x.state[1][nb:].clone(), conics_in[nb:])
    cur = (s["means"][nb:], s["u"][nb:], s["conics"][nb:])
    rec = loss_recipe(loss_ops, scene.name, prev, cur, points, None, tau, SEAM_DT, float(fx["nu"]),
                      (float(fx["pde_weight"]), float(fx["bc_weight"])))
    loss = rec["pde_loss"] + (s["penalty"] * x.weights).sum()
    out = {"deltas": s["deltas"], "penalty": s["penalty"], "residual": rec["residual"], "pde_loss": rec["pde_loss"], "loss": loss}
    leaves = [(n, p) for n, p in net.named_parameters() if p.requires_grad] + [("t_params0", x.t_params[0])]
    leaves += list(zip(ts.STATE, x.state))
    for (n, leaf), g in zip(leaves, torch.autograd.grad(loss, [t for _, t in leaves])):
        out["grad/" + n] = g
    return {k: v.detach() for k, v in out.items()}


def seam_allowance(name, err_torch32, scale):
    """every name floored at the sampler's 1e-5 but the two upstream of it (test_step.floor_of)"""
    return 4.0 * err_torch32 + (ts.FLOOR_UPSTREAM if name in ("deltas", "penalty") else FLOOR) * scale


def hold_seam(what, got, want, single):
    e_hip, e_t = ts.errors(got, want), ts.errors(single, want)
    worst, bad = 0.0, []
    for k in want:
        assert tuple(got[k].shape) == tuple(want[k].shape), (what, k)
        ratio = e_hip[k][0] / seam_allowance(k, *e_t[k])
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad.append(f"{k}: hip {e_hip[k][0]:.3g}, torch32 {e_t[k][0]:.3g}, scale {e_hip[k][1]:.3g}, ratio {ratio:.3g}")
    print(f"[figure] {what}: worst err_hip / (4 err_torch32 + floor x scale) = {worst:.3f}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return worst


_seam = {}


def seam_reference(name, k=0):
    """(scene, float64 oracle on the CPU, float32 torch composition on the GPU) for draw ``k`` of points and tau"""
    if (name, k) not in _seam:
        scene = ts.fixture_scene(name)
        p, t = seam_inputs(name, k)
        want = run_iteration(scene, ts.OracleOps(), OracleOps(), ts.Network(scene.sd), points=torch.as_tensor(p), tau=torch.as_tensor(t))
        single = run_iteration(scene, ts.OracleOps(), OracleOps(), ts.Network(scene.sd, torch.float32, "cuda"), torch.float32, "cuda",
                               points=torch.as_tensor(p, dtype=torch.float32, device="cuda"),
                               tau=torch.as_tensor(t, dtype=torch.float32, device="cuda"))
        _seam[(name, k)] = (scene, want, single)
    return _seam[(name, k)]


def hip_iteration(hip_lib, scene, host, route, **kw):
    from test_step_gpu import HipOps as StepOps, fused_network
    step_ops = StepOps(hip_lib, host, route)
    return run_iteration(scene, step_ops, HipOps(sampler=step_ops.sampler), fused_network(scene.sd), torch.float32, "cuda", **kw)


@pytest.mark.parametrize("route", ("one_launch", "separate"))
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name", SEAM)
def test_one_training_iteration(hip_lib, name, host, route):
    """the backward of residual() / vorticity_residual() feeding the backward of advance_gaussians, the aggregation and
    the fused MLPs, on the step's own sampler"""
    scene, want, single = seam_reference(name)
    got = hip_iteration(hip_lib, scene, host, route)
    assert float(want["residual"].abs().max()) > 0 and float(want["grad/t_params0"].abs().max()) > 0
    hold_seam(f"iteration on {name}, host {host}, heads {route}", got, want, single)


# ---- 3. capture ---------------------------------------------------------------------------------------------
def test_the_iteration_in_one_graphed_step(hip_lib):
    """GraphedStep over step + loss + backward on the Navier-Stokes fixture; two replays after new points and new tau were
    copied into the static inputs: each under the bar against the oracle, and within one allowance of the eager iteration"""
    from pigs_amd.graphs import GraphedStep
    from test_step_gpu import HipOps as StepOps, fused_network
    name = "navier_stokes"
    scene = seam_reference(name)[0]
    net = fused_network(scene.sd)
    holder = {}

    def make_inputs():
        holder["step"] = StepOps(hip_lib)
        holder["loss"] = HipOps(sampler=holder["step"].sampler)
        x = holder["x"] = ts.scene_tensors(scene, torch.float32, "cuda")
        p, t = seam_inputs(name)
        holder["points"], holder["tau"] = (torch.as_tensor(a, dtype=torch.float32, device="cuda") for a in (p, t))
        return x.t_params + x.state

    def fn(*leaves):
        rec = run_iteration(scene, holder["step"], holder["loss"], net, tensors=holder["x"], points=holder["points"], tau=holder["tau"])
        holder["names"] = list(rec)
        return tuple(rec.values())
    step = GraphedStep(fn, make_inputs, warmup=2)
    for k in (1, 2):
        _, want, single = seam_reference(name, k)
        p, t = (torch.as_tensor(a, dtype=torch.float32, device="cuda") for a in seam_inputs(name, k))
        with torch.no_grad():
            holder["points"].copy_(p)
            holder["tau"].copy_(t)
        got = dict(zip(holder["names"], [v.clone() for v in step()]))
        torch.cuda.synchronize()
        hold_seam(f"graphed iteration, replay {k}", got, want, single)
        eager = hip_iteration(hip_lib, scene, "native", "one_launch", points=p, tau=t)
        for n in SEAM_FORWARD:      # the same launches on the same inputs, every sum in a fixed order
            assert torch.equal(got[n], eager[n]), f"replay {k}: {n} differs from the eager iteration's"
        e_t, apart = ts.errors(single, want), ts.errors(got, eager)
        ratios = {n: apart[n][0] / seam_allowance(n, e_t[n][0], e_t[n][1]) for n in want}
        worst = max(ratios, key=ratios.get)      # the gradients come through atomics: both meet the bar, the distance is printed
        print(f"[figure] graphed iteration, replay {k}: gradients apart from the eager iteration's by {ratios[worst]:.3f} x the allowance ({worst})")


# ---- 4. determinism -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=["f32", "f64"])
@pytest.mark.parametrize("problem", tl.PROBLEMS)
def test_two_runs_give_the_same_forward_bits_on_the_dense_path(hip_lib, problem, dtype):
    """the dense forward sums the Gaussians in a fixed order: residual and losses of two runs are bit-equal (the
    gradients come through atomics and meet the bar: case 1)"""
    for rule in RULES:
        scene = loss_oracle(problem, rule)[0]
        a, b = (run_recipe(scene, HipOps("native", "dense"), dtype, "cuda") for _ in range(2))
        for k in FORWARD_OUTPUTS:
            assert torch.equal(a[k], b[k]), f"{problem} {rule} {k} differs between two runs on the same inputs"
