"""CPU: ``Model.compute_loss`` of the reference written in the terms of the one-launch operators, in float64 -- and pinned.

``loss_recipe`` is compute_loss (model_pn.py:790-849 with pde_rhs, :612-631) IN THE MODEL'S CONVENTIONS: the blend
weighs the CURRENT level with ``time_samples`` (``X_b = tau X_now + (1 - tau) X_prev``, :795-805), the residual is
``ut - dt * rhs`` (:830-849), the wave system carries its 0.01 on channel 0 (:844-845), and what compute_loss returns is
``pde_weight * pde_loss`` and ``bc_weight * bc_loss``.  It builds the ARGUMENTS of the operators -- the coefficient
fields a0, a1, lap, advect and target of ``residual()`` from the previous level's fields (DIFFUSION, BURGERS), the two
coupling matrices and couple_weight of the coupled ``residual()`` (WAVE), ``prev`` [M, 7], tau, nu and dt of
``vorticity_residual()`` (NAVIER_STOKES) -- and hands them to ``ops``.  ``OracleOps`` is a statement of each operator's
documented definition in torch over oracle/dense_torch.py (autograd supplies every gradient; dtype and device follow
the inputs); tests/test_model_loss_gpu.py hands the same arguments to ``GaussianSampler``.  INTEGRATION.md section 4
("compute_loss with the one-launch residuals") prints the recipes as they stand here.  With t = tau, s = 1 - tau:

    DIFFUSION   residual(a0=1, lap=-dt t, target=pu + dt s plap)
    BURGERS     residual(a0=1 + dt t s pux, a1=(dt t s pu, 0), lap=-dt nu t, advect=dt t^2, advect_by=((1,), (0,)),
                         target=pu + dt nu s plap - dt s^2 pu pux)
    WAVE        Q0 = dt ((0, -1), (0, 0.1)), QL = dt ((0, 0), (-10, 0))
                T = prev.residual(a0=1, couple_weight=-s, couple0=Q0, couple_lap=QL)           (no_grad)
                r = cur.residual(a0=1, couple_weight=t, couple0=Q0, couple_lap=QL, target=T)
                pde_loss = 0.01 mean(r[:, 0]^2) + mean(r[:, 1]^2)
    NAVIER_STOKES  vorticity_residual(nu, dt, prev=prev.vorticity_terms(), tau).pow(2).mean(0).sum()
    bc_loss = mean(sample_gaussians(bc points)^2)        (not for NAVIER_STOKES)

TRAPEZOID: tau = time_samples [M]; FORWARD: the float 0.0; BACKWARD: the float 1.0.

Here, without a GPU:
  * the operator statements equal the numpy checkers the suite already owns (test_residual_terms_gpu.compose,
    test_residual_coupled_gpu.compose, test_vorticity.combine + test_vorticity_residual.compose) to rounding, and the
    third derivatives added to oracle/dense_torch.py equal oracle/c_oracle's;
  * THE PIN: on the recorded inputs of the twelve scenes of tests/golden/model_pn_loss/*.npz (tools/gen_model_loss.py:
    4 problems x 3 rules, 121 free Gaussians, M = 100, 60 boundary points, dt = 0.25) the per-point residual, pde_loss,
    bc_loss and the gradients that left the two ``preprocess`` calls of the current level equal the recording to 1e-10
    of each tensor's largest entry.  The recording holds ``rhs`` and the two terms of ``ut`` (``wt``); the recorded
    residual is ``ut - dt * rhs``.  For NAVIER_STOKES that is column 1 of the operator's output; its column 0 (the
    blended divergence) is pinned through pde_loss and the gradients.  NAVIER_STOKES under FORWARD / BACKWARD is
    recorded under TRAPEZOID with time_samples all 0 / all 1: the reference defines wx / wxx under TRAPEZOID only;
  * DISCRIMINATION: each of eight deliberate mistakes planted in the recipe or the oracle moves some pinned quantity by
    at least 10 x the GPU allowance of tests/test_model_loss_gpu.py for it (4 err_torch32 + 1e-5 x scale, the float32
    composition's error measured here on the CPU), on the inputs rounded to float32 as the GPU file uses them.
    MEASURED smallest factor per mistake (over the scenes it applies to): tau_swapped 6.9e+04, dt_dropped 3.2e+05,
    dt_divides 1.3e+06, nu_dropped 3.5e+03, advection_sign 1.2e+05, blend_of_products 6.4e+03,
    wave_weight_other_channel 9.7e+04, wt_blended 3.5e+04;
  * scene conditions, so that the GPU file may rely on them: every conic of both levels is positive definite; the one
    limit the sampler documents for a Gaussian's extent is that of its periodic domain, sqrt(q Sigma_ii) < L, and the
    problem that lives on one (NAVIER_STOKES, L = 2; recorded and run here with the plain sampler) is held to it at
    q = 36 (the lattice problems carry wider Gaussians, DIFFUSION up to a half extent of 2.07: the plain sampler
    documents no limit for them); no collocation point is farther than q = 36 from every Gaussian of either level.
"""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import dense_torch
from test_advance import scale_of

PROBLEMS = ("diffusion", "burgers", "wave", "navier_stokes")
RULES = ("TRAPEZOID", "FORWARD", "BACKWARD")
SCENES = [(p, r) for p in PROBLEMS for r in RULES]
INPUTS = ("means", "values", "conics")
FLOOR, Q_MAX = 1e-5, 36.0
CHECKED = ("residual", "pde_loss", "bc_loss", "grad/means", "grad/values", "grad/conics")
WAVE_Q0, WAVE_QL = ((0.0, -1.0), (0.0, 0.1)), ((0.0, 0.0), (-10.0, 0.0))      # -rhs of :624-627 as u @ Q0.T + lap @ QL.T
# mistake -> the problems it can show on (every rule of them, where the rule leaves it visible)
MISTAKES = {"tau_swapped": PROBLEMS, "dt_dropped": PROBLEMS, "dt_divides": PROBLEMS, "nu_dropped": ("burgers", "navier_stokes"),
            "advection_sign": ("burgers", "navier_stokes"), "blend_of_products": ("burgers", "navier_stokes"),
            "wave_weight_other_channel": ("wave",), "wt_blended": ("navier_stokes",)}
ONLY_RULES = {"blend_of_products": ("TRAPEZOID",), "wt_blended": ("TRAPEZOID", "FORWARD")}      # elsewhere no change at all


def load_fixture(problem):
    with np.load(os.path.join(GOLDEN, "model_pn_loss", f"{problem}.npz")) as f:
        return {k: f[k] for k in f.files}


def as_float32(a):
    """the values a float32 path can hold, in float64: every path of a scene starts from the same numbers"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def tau_of(rule, time_samples):
    return {"TRAPEZOID": time_samples, "FORWARD": 0.0, "BACKWARD": 1.0}[rule]


def make_scene(problem, rule, rounded=True):
    """the recorded inputs of one scene; ``rounded``: to float32 values (the GPU file), else as recorded (the pin)"""
    fx = load_fixture(problem)
    r = as_float32 if rounded else np.asarray
    return types.SimpleNamespace(
        problem=problem, rule=rule, prev={k: r(fx["prev/" + k]) for k in INPUTS}, cur={k: r(fx["cur/" + k]) for k in INPUTS},
        samples=r(fx["samples"]), bc_samples=r(fx["bc_samples"]), tau=tau_of(rule, r(fx["time_samples"])),
        dt=float(fx["dt"]), nu=float(fx["nu"]), weights=(float(fx["pde_weight"]), float(fx["bc_weight"])))


# ---- the operators, as documented, in torch ------------------------------------------------------------------
def col(v):
    """a float, or a field [M] as a column"""
    return v[:, None] if isinstance(v, torch.Tensor) else v


def residual_terms(o, a0=0.0, a1=(0.0, 0.0), lap=0.0, target=None, advect=0.0, advect_by=None):
    """GaussianSampler.residual(), the general form: r = a0 u + a1 . grad u + lap (u_xx + u_yy) + advect (w . grad) u -
    target, w_i = sum_c' advect_by[i][c'] u_c'; ``o`` = {order: tensor} of orders 0, 1, 2"""
    u, du, trace = o[0], o[1], o[2][:, 0, 0] + o[2][:, 1, 1]
    r = col(a0) * u + col(lap) * trace - (0 if target is None else target.reshape(u.shape))
    B = None if advect_by is None else torch.as_tensor(advect_by, dtype=u.dtype, device=u.device)
    for i in range(du.shape[1]):
        coef = a1[:, i] if isinstance(a1, torch.Tensor) else a1[i]
        if B is not None:
            coef = coef + advect * (u @ B[i])
        r = r + col(coef) * du[:, i]
    return r


def residual_coupled(o, a0=0.0, lap=0.0, couple_weight=1.0, couple0=None, couple_lap=None, target=None):
    """GaussianSampler.residual(), the coupled form: r = a0 u + lap (u_xx + u_yy) + couple_weight (u @ couple0.T +
    lap_u @ couple_lap.T) - target"""
    u, trace = o[0], o[2][:, 0, 0] + o[2][:, 1, 1]
    Q0, QL = (torch.as_tensor(q, dtype=u.dtype, device=u.device) for q in (couple0, couple_lap))
    return col(a0) * u + col(lap) * trace + col(couple_weight) * (u @ Q0.T + trace @ QL.T) - (0 if target is None else target)


def vorticity_terms(o):
    """GaussianSampler.vorticity_terms(): (u_x, u_y, div, w, w_x, w_y, lap_w) [M, 7] from orders 0..3, w = d_x u_y - d_y u_x"""
    u, ux, uxx, uxxx = o[0], o[1], o[2], o[3]
    wx = uxx[..., 0, 1] - uxx[..., 1, 0]
    wxx = uxxx[..., 0, 1] - uxxx[..., 1, 0]
    return torch.stack((u[:, 0], u[:, 1], ux[:, 0, 0] + ux[:, 1, 1], ux[:, 0, 1] - ux[:, 1, 0], wx[:, 0], wx[:, 1],
                        wxx[:, 0, 0] + wxx[:, 1, 1]), -1)


def vorticity_residual(now, prev, tau, nu, dt, time_term=1.0, mistake=None):
    """GaussianSampler.vorticity_residual(): (div_b, time_term (w_now - w_prev) - dt (nu lap_w_b - u_b . grad w_b)) [M, 2],
    X_b = tau X_now + (1 - tau) X_prev.  ``mistake``: one of the three that live inside the operator."""
    t = col(tau)
    b = t * now + (1 - t) * prev
    advection = b[:, 0] * b[:, 4] + b[:, 1] * b[:, 5]
    if mistake == "blend_of_products":
        advection = (t * (now[:, 0:2] * now[:, 4:6]) + (1 - t) * (prev[:, 0:2] * prev[:, 4:6])).sum(-1)
    if mistake == "advection_sign":
        advection = -advection
    wt = (b[:, 3] if mistake == "wt_blended" else now[:, 3]) - prev[:, 3]
    return torch.stack((b[:, 2], time_term * wt - dt * (nu * b[:, 6] - advection)), -1)


class OracleOps:
    """The operators on a level = (means, values, conics) bound to points, from oracle/dense_torch.py."""

    def __init__(self, mistake=None):
        self.mistake = mistake

    def orders(self, level, points, orders):
        return dense_torch.forward(level[0], level[2], level[1], points, orders=orders)

    def fields(self, level, points):
        o = self.orders(level, points, (0, 1, 2))
        return o[0], o[1], o[2][:, 0, 0] + o[2][:, 1, 1]

    def u(self, level, points):
        return self.orders(level, points, (0,))[0]

    def residual(self, level, points, **kw):
        o = self.orders(level, points, (0, 1, 2))
        return residual_coupled(o, **kw) if "couple0" in kw else residual_terms(o, **kw)

    def vorticity_terms(self, level, points):
        return vorticity_terms(self.orders(level, points, (0, 1, 2, 3)))

    def vorticity_residual(self, level, points, nu, dt, prev, tau, time_term=1.0):
        return vorticity_residual(self.vorticity_terms(level, points), prev, tau, nu, dt, time_term, self.mistake)


# ---- the recipe ----------------------------------------------------------------------------------------------
def loss_recipe(ops, problem, prev, cur, points, bc_points, tau, dt, nu, weights, mistake=None):
    """compute_loss in the model's conventions through ``ops``: ``prev`` / ``cur`` = (means, values, conics) of the two
    levels (the previous one a constant), ``tau`` a float or [M]; ``bc_points`` None: no boundary term.  Returns the
    per-point residual and the two losses as compute_loss returns them.  ``mistake``: one of MISTAKES, planted on purpose (test_the_pin_discriminates)."""
    t, s = tau, 1 - tau                       # the weights of the current and of the previous level, :795-805
    if mistake == "tau_swapped":
        t, s = s, t
    k, h = {"dt_dropped": (1.0, 1.0), "dt_divides": (1.0 / dt, 1.0)}.get(mistake, (1.0, dt))      # r = k ut - h rhs, :830-849
    if mistake == "nu_dropped":
        nu = 0.0
    if problem == "diffusion":
        with torch.no_grad():
            pu, _, plap = ops.fields(prev, points)
        r = ops.residual(cur, points, a0=k, lap=-h * t, target=k * pu + col(h * s) * plap)
        pde = r.pow(2).mean()
    elif problem == "burgers":
        with torch.no_grad():
            pu, pdu, plap = ops.fields(prev, points)
            pu, pux, plap = pu[:, 0], pdu[:, 0, 0], plap[:, 0]
        g = -h if mistake == "advection_sign" else h
        if mistake == "blend_of_products":                      # t u ux + s pu pux in place of (t u + s pu) (t ux + s pux)
            a0, a1x, adv, target = k, 0.0 * pu, g * t, k * pu + h * nu * s * plap - g * s * pu * pux
        else:
            a0, a1x, adv, target = k + g * t * s * pux, g * t * s * pu, g * t * t, k * pu + h * nu * s * plap - g * s * s * pu * pux
        r = ops.residual(cur, points, a0=a0, a1=torch.stack((a1x, torch.zeros_like(a1x)), -1), lap=-h * nu * t, advect=adv,
                         advect_by=((1.0,), (0.0,)), target=target[:, None])
        pde = r.pow(2).mean()
    elif problem == "wave":
        Q0, QL = h * np.array(WAVE_Q0), h * np.array(WAVE_QL)
        with torch.no_grad():
            T = ops.residual(prev, points, a0=k, couple_weight=-s, couple0=Q0, couple_lap=QL)
        r = ops.residual(cur, points, a0=k, couple_weight=t, couple0=Q0, couple_lap=QL, target=T)
        small, full = (1, 0) if mistake == "wave_weight_other_channel" else (0, 1)
        pde = 0.01 * r[:, small].pow(2).mean() + r[:, full].pow(2).mean()
    elif problem == "navier_stokes":
        with torch.no_grad():
            prev7 = ops.vorticity_terms(prev, points)
        r = ops.vorticity_residual(cur, points, nu, h, prev7, t, time_term=k)
        pde = r.pow(2).mean(0).sum()
    else:
        raise ValueError(problem)
    bc = torch.zeros((), dtype=r.dtype, device=r.device)
    if problem != "navier_stokes" and bc_points is not None:
        bc = ops.u(cur, bc_points).pow(2).mean()
    return {"residual": r, "pde_loss": weights[0] * pde, "bc_loss": weights[1] * bc}


def level_tensors(arrays, dtype, device, grad):
    return [torch.as_tensor(arrays[k], dtype=dtype, device=device).requires_grad_(grad) for k in INPUTS]


def run_recipe(scene, ops, dtype=torch.float64, device="cpu", mistake=None, split=False):
    """The scene through ``ops``: the residual, the two losses and the gradient of their sum with respect to the current
    level's means, values and conics (one backward, as the training loop's); ``split``: also of each loss alone."""
    def tensor(a):
        return a if isinstance(a, float) else torch.as_tensor(a, dtype=dtype, device=device)
    prev, cur = level_tensors(scene.prev, dtype, device, False), level_tensors(scene.cur, dtype, device, True)
    rec = loss_recipe(ops, scene.problem, prev, cur, tensor(scene.samples), tensor(scene.bc_samples), tensor(scene.tau),
                      scene.dt, scene.nu, scene.weights, mistake)
    if split:
        for name in ("pde", "bc"):
            if rec[name + "_loss"].requires_grad:
                g = torch.autograd.grad(rec[name + "_loss"], cur, retain_graph=True, allow_unused=True)
                rec.update({f"grad_{name}/{k}": torch.zeros_like(x) if v is None else v for k, x, v in zip(INPUTS, cur, g)})
    rec.update({f"grad/{k}": v for k, v in zip(INPUTS, torch.autograd.grad(rec["pde_loss"] + rec["bc_loss"], cur))})
    return {k: v.detach() for k, v in rec.items()}


def host(t):
    return t.detach().cpu().double().numpy()


def errors(got, want, keys=CHECKED):
    """{name: (largest absolute error, the reference's largest entry)}"""
    return {k: (float(np.abs(host(got[k]) - host(want[k])).max()), scale_of(host(want[k]))) for k in keys}


def allowance(err_torch32, scale):
    return 4.0 * err_torch32 + FLOOR * scale


_runs = {}


def loss_oracle(problem, rule, dtype=torch.float64):
    """the unperturbed oracle on a scene of rounded inputs: computed once, shared, never changed.  (scene, results)"""
    if (problem, rule, dtype) not in _runs:
        scene = make_scene(problem, rule)
        _runs[(problem, rule, dtype)] = (scene, run_recipe(scene, OracleOps(), dtype))
    return _runs[(problem, rule, dtype)]


# ---- the statements against the checkers the suite owns -------------------------------------------------------
def test_third_derivatives_of_the_torch_oracle_equal_the_c_oracle():
    from oracle import c_oracle
    s = make_scene("navier_stokes", "TRAPEZOID", rounded=False)
    args = (s.cur["means"], s.cur["conics"], s.cur["values"], s.samples)
    want = c_oracle.forward(*args, orders=(0, 1, 2, 3))
    got = dense_torch.forward(*(torch.as_tensor(a) for a in args), orders=(0, 1, 2, 3))
    for o in range(4):
        assert np.abs(host(got[o]) - want[o]).max() <= 1e-12 * np.abs(want[o]).max(), o


def test_the_operator_statements_equal_the_numpy_checkers():
    """the torch statements above against test_residual_terms_gpu.compose, test_residual_coupled_gpu.compose and
    test_vorticity.combine + test_vorticity_residual.compose, on a recorded level with seeded fields"""
    from test_residual_coupled_gpu import compose as compose_coupled
    from test_residual_terms_gpu import compose as compose_terms
    from test_vorticity import combine
    from test_vorticity_residual import compose as compose_vorticity
    rng = np.random.default_rng(7)
    M = 100
    for problem in ("burgers", "wave"):
        s = make_scene(problem, "TRAPEZOID", rounded=False)
        c = s.cur["values"].shape[1]
        level = [torch.as_tensor(s.cur[k]) for k in INPUTS]
        o = OracleOps().orders(level, torch.as_tensor(s.samples), (0, 1, 2, 3))
        exp = {k: host(v) for k, v in o.items()}
        a0, a1, aL, adv, cw = rng.uniform(0.5, 2, M), rng.uniform(-1, 1, (M, 2)), rng.uniform(-0.1, 0.1, M), rng.uniform(0.2, 1, M), rng.uniform(0.2, 1, M)
        target = rng.uniform(-1, 1, (M, c))
        T = torch.as_tensor
        if c == 1:
            B = ((0.8,), (-0.5,))
            got = residual_terms(o, T(a0), T(a1), T(aL), T(target), T(adv), B)
            want = compose_terms(exp, (a0, a1, aL, adv), B, target, 2)
            floats = residual_terms(o, 1.5, (0.25, -0.5), -0.01, T(target), 0.75, B)
            ones = np.ones(M)
            want_floats = compose_terms(exp, (1.5 * ones, np.stack((0.25 * ones, -0.5 * ones), -1), -0.01 * ones, 0.75 * ones), B, target, 2)
            assert np.abs(host(floats) - want_floats).max() <= 1e-13 * np.abs(want_floats).max()
        else:
            Q0, QL = rng.uniform(-1, 1, (2, 2)), rng.uniform(-0.1, 0.1, (2, 2))
            got = residual_coupled(o, T(a0), T(aL), T(cw), Q0, QL, T(target))
            want = compose_coupled(exp, (a0, aL, cw, Q0, QL), target, 2)
            prev7, tau = rng.normal(size=(M, 7)), rng.uniform(0, 1, M)
            now7 = vorticity_terms(o)
            assert np.abs(host(now7) - combine(exp)).max() <= 1e-13 * np.abs(combine(exp)).max()
            for tt, k in ((tau, 1.0), (0.0, 1.0), (1.0, -2.5)):
                v = vorticity_residual(now7, T(prev7), T(tt) if isinstance(tt, np.ndarray) else tt, 0.05, 0.3, k)
                w = compose_vorticity(combine(exp), prev7, tt, 0.05, 0.3, k)
                assert np.abs(host(v) - w).max() <= 1e-13 * np.abs(w).max()
        assert np.abs(host(got) - want).max() <= 1e-13 * np.abs(want).max(), problem


# ---- the pin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,rule", SCENES)
def test_the_recipe_reproduces_the_recorded_compute_loss(problem, rule):
    """float64 against float64 on the inputs as recorded: 1e-10 of each tensor's largest entry"""
    fx = load_fixture(problem)
    assert tuple(fx["rules"]) == RULES
    got = run_recipe(make_scene(problem, rule, rounded=False), OracleOps(), split=True)
    ns = problem == "navier_stokes"
    ut = fx["w_now"] - fx["w_prev"] if ns else fx["u_now"] - fx["u_prev"]
    want = {"residual": ut - float(fx["dt"]) * fx[rule + "/rhs"].reshape(ut.shape), "pde_loss": fx[rule + "/pde_loss"],
            "bc_loss": fx[rule + "/bc_loss"]}
    want.update({k[len(rule) + 1:]: v for k, v in fx.items() if k.startswith(rule + "/grad_")})
    assert len(want) == (6 if ns else 9)
    got["residual"] = got["residual"][:, 1] if ns else got["residual"].reshape(ut.shape)
    worst = 0.0
    for name, w in want.items():
        assert tuple(got[name].shape) == w.shape, (name, tuple(got[name].shape), w.shape)
        err = np.abs(host(got[name]) - w).max() / scale_of(w)
        worst = max(worst, err)
        assert err <= 1e-10, f"{problem} {rule} {name}: {err:.3g} of its largest entry"
    if ns:
        assert float(got["bc_loss"]) == 0.0 == float(fx[rule + "/bc_loss"])
    print(f"[figure] {problem} {rule}: the recipe against the recorded compute_loss, worst {worst:.3g} of a tensor's largest entry")


def test_fixtures_hold_float64_data_within_the_size_of_the_largest_fixture():
    largest = os.path.getsize(os.path.join(GOLDEN, "model_pn_step", "navier_stokes.npz"))
    for problem in PROBLEMS:
        fx = load_fixture(problem)
        N, M = fx["cur/means"].shape[0], fx["samples"].shape[0]
        assert 100 <= N <= 150 and N % 16 and N % 64 and M == 100 and fx["bc_samples"].shape[0] == 60
        assert float(fx["dt"]) == 0.25
        assert all(v.dtype == np.float64 for k, v in fx.items() if k != "rules")
        assert os.path.getsize(os.path.join(GOLDEN, "model_pn_loss", f"{problem}.npz")) <= largest
        assert np.abs(fx["cur/means"] - fx["prev/means"]).max() > 0 and 0 < fx["time_samples"].min() and fx["time_samples"].max() < 1


# ---- scene conditions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", PROBLEMS)
def test_scene_conditions(problem):
    """on the inputs as the GPU file uses them (rounded to float32): positive definite conics, NAVIER_STOKES within the
    periodic sampler's extent limit sqrt(36 Sigma_ii) < 2, and every collocation point within q = 36 of some Gaussian of
    each level (its residual would be pure target otherwise)"""
    s = make_scene(problem, "TRAPEZOID")
    for level in (s.prev, s.cur):
        a, b, c = level["conics"].T
        det = a * c - b * b
        assert (det > 0).all() and (a > 0).all()
        half = np.sqrt(Q_MAX * np.stack((c / det, a / det), -1))          # half extents: sqrt(q Sigma_ii)
        assert np.isfinite(half).all()
        if problem == "navier_stokes":
            assert half.max() < 2.0, half.max()
        x = s.samples[:, None, :] - level["means"][None, :, :]
        q = a * x[..., 0] ** 2 + 2 * b * x[..., 0] * x[..., 1] + c * x[..., 1] ** 2
        nearest = q.min(1)
        assert nearest.max() < Q_MAX, f"{problem}: a collocation point has q >= {nearest.max():.3g} to every Gaussian"
        print(f"[figure] {problem}: widest half extent {half.max():.3g}, farthest collocation point at q = {nearest.max():.3g}")


# ---- the pin discriminates ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_the_pin_discriminates(mistake):
    """A mistake planted in the recipe (or, for the three that live inside vorticity_residual, in the oracle's statement
    of it) moves at least one checked quantity of every scene it applies to by 10 x what the GPU bar allows for it,
    4 err_torch32 + 1e-5 x scale with the float32 composition's error measured here on the CPU."""
    smallest = None
    for problem in MISTAKES[mistake]:
        for rule in ONLY_RULES.get(mistake, RULES):
            scene, want = loss_oracle(problem, rule)
            _, single = loss_oracle(problem, rule, torch.float32)
            wrong = run_recipe(scene, OracleOps(mistake), mistake=mistake)
            err32, moved = errors(single, want), errors(wrong, want)
            factors = {k: moved[k][0] / allowance(*err32[k]) for k in CHECKED}
            best = max(factors, key=factors.get)
            print(f"[figure] {mistake} on {problem} {rule}: {best} moves by {factors[best]:.3g} x its allowance")
            assert factors[best] >= 10.0, f"{mistake} on {problem} {rule}: nothing moves by more than {factors[best]:.3g} x its allowance"
            smallest = factors[best] if smallest is None else min(smallest, factors[best])
    print(f"[figure] {mistake}: smallest factor {smallest:.3g}")
