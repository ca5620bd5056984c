"""CPU: GaussianAdam1D (pigs_amd/optim.py, csrc/optim.hip: optim1d_*) -- its float64 checker against
torch.optim.Adam plus autograd through the reference's own lines (test_no_mlp_1d.py:109-111) plus the statistic lines
(:156-162), the presence patterns of its three groups, the C ABI's refusals, the class's refusals, and the recorded 1-D
loop of tests/golden/grad_stats/no_mlp_1d.npz.  No GPU call is made here.

Shared with tests/test_optim_1d_gpu.py:
    make_state_1d() / make_grads_1d()   a starting state and gradients of (means, values, covariances, conics), each [N,1]
    chain_rule_1d() / checker_step_1d() ONE step: d raw_means = d mu * scale * sech^2, d raw_scaling = d cov * s - d conic / s
    TorchChain1D, loop_1d()             the Burgers loop of test_no_mlp_1d.py:97-153 over GaussianAdam1D's interface
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_optim import BETAS, EPS, scale_of, sech2
from test_optim_stats import (STATS, Gaussians, assert_stats_agree, check_fixture, filled_stats, make_stats,
                              reference_lines, stats_step, torch_stats)

GROUPS = ("means", "values", "scaling")
RATES = {"means": 5e-3, "values": 1e-3, "scaling": 5e-2}


# ---- the checker --------------------------------------------------------------------------------------------
def make_state_1d(N, c, seed, steps=0, moments=False):
    """raw_means N(0, 0.8), values N(0, 1), raw_scaling U[-4, -1]; moments zero or random; per-group step counts"""
    rng = np.random.default_rng(seed)
    p = {"means": 0.8 * rng.standard_normal((N, 1)), "values": rng.standard_normal((N, c)),
         "scaling": rng.uniform(-4.0, -1.0, (N, 1))}
    if moments:
        m = {g: rng.standard_normal(p[g].shape) for g in GROUPS}
        v = {g: rng.standard_normal(p[g].shape) ** 2 for g in GROUPS}
    else:
        m = {g: np.zeros_like(p[g]) for g in GROUPS}
        v = {g: np.zeros_like(p[g]) for g in GROUPS}
    steps = dict(steps) if isinstance(steps, dict) else {g: int(steps) for g in GROUPS}
    return {"p": p, "m": m, "v": v, "steps": steps}


def make_grads_1d(N, c, seed, present=(True, True, False, True)):
    rng = np.random.default_rng(seed + 104729)
    shapes = ((N, 1), (N, c), (N, 1), (N, 1))
    return tuple(rng.standard_normal(s) if on else None for s, on in zip(shapes, present))


def as_dtype_1d(state, dtype):
    out = copy.deepcopy(state)
    for k in ("p", "m", "v"):
        out[k] = {g: a.astype(dtype).astype(np.float64) for g, a in state[k].items()}
    return out


def forward_1d(p, means_map="tanh", scale=1.0):
    means = np.tanh(p["means"]) * scale if means_map == "tanh" else p["means"].copy()
    s = np.exp(p["scaling"])
    return means, s, 1.0 / s


def chain_rule_1d(p, grads, means_map="tanh", scale=1.0):
    g_means, g_values, g_cov, g_con = grads
    out = {g: None for g in GROUPS}
    if g_means is not None:
        out["means"] = g_means * scale * sech2(p["means"]) if means_map == "tanh" else g_means.copy()
    if g_values is not None:
        out["values"] = g_values.copy()
    if g_cov is not None or g_con is not None:
        s = np.exp(p["scaling"])
        out["scaling"] = (0.0 if g_cov is None else g_cov * s) - (0.0 if g_con is None else g_con / s)
    return out


def checker_step_1d(state, grads, lr=RATES, betas=BETAS, eps=EPS, means_map="tanh", scale=1.0, wrap=None):
    new = copy.deepcopy(state)
    raw = chain_rule_1d(state["p"], grads, means_map, scale)
    b1, b2 = betas
    for g in GROUPS:
        if raw[g] is None:
            continue
        t = new["steps"][g] = state["steps"][g] + 1
        m = new["m"][g] = b1 * state["m"][g] + (1.0 - b1) * raw[g]
        v = new["v"][g] = b2 * state["v"][g] + (1.0 - b2) * raw[g] ** 2
        new["p"][g] = state["p"][g] - lr[g] / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    if wrap is not None and raw["means"] is not None:
        lo, hi = wrap
        x = new["p"]["means"]
        x = np.where(x > hi, x - (hi - lo), x)
        new["p"]["means"] = np.where(x < lo, x + (hi - lo), x)
    return new, forward_1d(new["p"], means_map, scale)


# ---- against torch.optim.Adam, autograd and the reference's lines -------------------------------------------
def torch_state_1d(state, dtype=torch.float64, device="cpu", lr=RATES):
    params = {g: torch.tensor(state["p"][g], dtype=dtype, device=device, requires_grad=True) for g in GROUPS}
    optim = torch.optim.Adam([{"params": [params[g]], "lr": lr[g]} for g in GROUPS], betas=BETAS, eps=EPS, foreach=False)
    for g in GROUPS:
        if state["steps"][g] > 0 or np.any(state["m"][g]) or np.any(state["v"][g]):
            optim.state[params[g]] = {"step": torch.tensor(float(state["steps"][g])),
                                      "exp_avg": torch.tensor(state["m"][g], dtype=dtype, device=device),
                                      "exp_avg_sq": torch.tensor(state["v"][g], dtype=dtype, device=device)}
    return params, optim


def torch_step_1d(params, optim, grads, means_map="tanh", scale=1.0, wrap=None):
    """test_no_mlp_1d.py:109-111 (tanh * scale, exp, 1 / covariances), autograd from the given gradients, Adam, the wrap;
    the gradients stay on the parameters"""
    ref = params["means"]
    means = torch.tanh(params["means"]) * scale if means_map == "tanh" else params["means"]
    covariances = torch.exp(params["scaling"]).reshape(-1, 1)
    conics = 1.0 / covariances
    loss = None
    for out, g in zip((means, params["values"], covariances, conics), grads):
        if g is not None:
            term = (out * torch.as_tensor(g, dtype=ref.dtype, device=ref.device)).sum()
            loss = term if loss is None else loss + term
    optim.zero_grad(set_to_none=True)
    loss.backward()
    optim.step()
    if wrap is not None and params["means"].grad is not None:
        lo, hi = wrap
        with torch.no_grad():
            raw_means = params["means"]
            oob = raw_means > hi
            raw_means[oob] -= hi - lo
            oob = raw_means < lo
            raw_means[oob] += hi - lo


def read_torch_1d(params, optim, like):
    out = copy.deepcopy(like)
    for g in GROUPS:
        out["p"][g] = params[g].detach().cpu().double().numpy().copy()
        st = optim.state.get(params[g])
        if st:
            out["m"][g] = st["exp_avg"].cpu().double().numpy().copy()
            out["v"][g] = st["exp_avg_sq"].cpu().double().numpy().copy()
            out["steps"][g] = int(st["step"])
        else:
            out["steps"][g] = 0
    return out


def assert_states_agree_1d(got, want, bar, what=""):
    worst = 0.0
    for k in ("p", "m", "v"):
        for g in GROUPS:
            err = float(np.abs(got[k][g] - want[k][g]).max()) / scale_of(want[k][g])
            worst = max(worst, err)
            assert err <= bar, f"{what} {k}[{g}]: {err:.3g} of its scale > {bar:.3g}"
    assert got["steps"] == want["steps"], (what, got["steps"], want["steps"])
    return worst


def test_checker_agrees_with_torch_adam_autograd_and_the_reference_lines():
    """float64 on the CPU, five consecutive steps each compared as ONE step from torch's state before it, statistics from
    non-zero sums: N = 257, c = 2, three distinct rates; 1e-12 of each tensor's scale"""
    N, c = 257, 2
    state, stats = make_state_1d(N, c, seed=1), make_stats(N, seed=1, d=1)
    params, optim = torch_state_1d(state)
    t = torch_stats(stats)
    worst = 0.0
    for it in range(5):
        grads = make_grads_1d(N, c, seed=10 + it, present=(True, True, it % 2 == 1, it != 3))
        before = read_torch_1d(params, optim, state)
        stats_before = dict({k: t[k].numpy().copy() for k in STATS}, counts=dict(stats["counts"]))
        torch_step_1d(params, optim, grads, "tanh", 2.5)
        reference_lines(t, params["means"], params["scaling"])
        want = read_torch_1d(params, optim, state)
        got, _ = checker_step_1d(before, grads, means_map="tanh", scale=2.5)
        worst = max(worst, assert_states_agree_1d(got, want, 1e-12, f"step {it}"))
        got_stats = stats_step(before["p"], stats_before, grads, "tanh", 2.5, chain=chain_rule_1d)
        worst = max(worst, assert_stats_agree(got_stats, t, 1e-12, f"step {it}"))
    assert want["steps"] == {g: 5 for g in GROUPS}
    print(f"1-D checker vs torch.optim.Adam + autograd + the reference's lines, float64: worst {worst:.3g}")


@pytest.mark.parametrize("mistake", ["step_norm", "norm_before", "d_mu"])
def test_checker_sees_a_planted_mistake(mistake):
    N, c = 257, 1
    state, stats = make_state_1d(N, c, seed=2), make_stats(N, seed=2, d=1)
    grads = make_grads_1d(N, c, seed=3, present=(True, True, True, True))
    want = stats_step(state["p"], stats, grads, "tanh", 2.5, chain=chain_rule_1d)
    wrong = stats_step(state["p"], stats, grads, "tanh", 2.5, chain=chain_rule_1d, mistake=mistake)
    moved = max(float(np.abs(wrong[k] - want[k]).max()) / scale_of(want[k]) for k in STATS)
    print(f"1-D planted mistake {mistake}: moves a statistic by {moved:.3g} of its scale, {moved / 1e-11:.3g} x the "
          f"float64 bar, {moved / 2e-3:.3g} x the loop bar")
    assert moved >= 1e-2


PATTERNS = [(a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)
            if a or b or c or d]


@pytest.mark.parametrize("present", PATTERNS, ids=["".join("mvcq"[i] if on else "-" for i, on in enumerate(p)) for p in PATTERNS])
def test_null_gradients_skip_their_group_as_torch_does(present):
    N, c = 65, 2
    state = make_state_1d(N, c, seed=3, moments=True, steps={"means": 3, "values": 5, "scaling": 2})
    stats = make_stats(N, seed=3, d=1)
    grads = make_grads_1d(N, c, seed=4, present=present)
    params, optim = torch_state_1d(state)
    t = torch_stats(stats)
    torch_step_1d(params, optim, grads, "identity", wrap=(-1.0, 1.0))
    reference_lines(t, params["means"], params["scaling"])
    want = read_torch_1d(params, optim, state)
    got, _ = checker_step_1d(state, grads, means_map="identity", wrap=(-1.0, 1.0))
    assert_states_agree_1d(got, want, 1e-12, str(present))
    got_stats = stats_step(state["p"], stats, grads, "identity", chain=chain_rule_1d)
    assert_stats_agree(got_stats, t, 1e-12, str(present))
    on = {"means": present[0], "values": present[1], "scaling": present[2] or present[3]}
    for g in GROUPS:
        assert got["steps"][g] == state["steps"][g] + int(on[g])
        if not on[g]:
            assert all(np.array_equal(got[k][g], state[k][g]) for k in ("p", "m", "v"))
    for g, names in (("means", ("mean_grad", "mean_grad_norm", "last_mean_grad")),
                     ("scaling", ("scale_grad", "scale_grad_norm", "last_scale_grad"))):
        assert got_stats["counts"][g] == 3 + int(on[g])
        if not on[g]:
            assert all(np.array_equal(got_stats[k], stats[k]) for k in names)


# ---- the C ABI ----------------------------------------------------------------------------------------------
def test_refusals_come_before_any_hip_call(hip_lib):
    """pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    from pigs_amd import _lib
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(1 << 12)
    mat, step = hip_lib.pigs_optim1d_materialize, hip_lib.pigs_optim1d_step
    assert mat(7, 0, 4, 1.0, *([some] * 5), null) == 2                        # dtype
    assert mat(0, 2, 4, 1.0, *([some] * 5), null) == 2                        # map
    assert mat(0, 0, 0, 1.0, *([some] * 5), null) == 1                        # N = 0
    assert mat(1, 1, -3, 1.0, *([some] * 5), null) == 1                       # N < 0
    for k in range(5):
        args = [some] * 5
        args[k] = null
        assert mat(0, 0, 4, 1.0, *args, null) == 1                            # a null array

    h = _lib.PigsAdamStep()
    h.means_map = 0
    ok = [some] * 16
    for stats in (None, ctypes.byref(filled_stats())):
        assert step(0, 1, 4, None, *ok, stats, null) == 1                     # null hyper
        assert step(7, 1, 4, ctypes.byref(h), *ok, stats, null) == 2          # dtype
        assert step(0, 0, 4, ctypes.byref(h), *ok, stats, null) == 2          # c outside 1..4
        assert step(0, 5, 4, ctypes.byref(h), *ok, stats, null) == 2
        assert step(0, 1, 0, ctypes.byref(h), *ok, stats, null) == 1          # N <= 0
        assert step(1, 4, -1, ctypes.byref(h), *ok, stats, null) == 1
        h.means_map = 3
        assert step(0, 1, 4, ctypes.byref(h), *ok, stats, null) == 2          # map
        h.means_map = 1
        for k in list(range(9)) + [13, 14, 15]:                               # parameters, moments, outputs
            args = list(ok)
            args[k] = null
            assert step(0, 1, 4, ctypes.byref(h), *args, stats, null) == 1, k
        args = list(ok)
        args[9:13] = [null] * 4
        assert step(0, 1, 4, ctypes.byref(h), *args, stats, null) == 1        # no gradient at all
    for name, _ in _lib.PigsGradStats._fields_[:6]:                           # a null statistics array
        bad = filled_stats()
        setattr(bad, name, None)
        assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1, name
    bad = filled_stats()
    bad.device_counts = 1 << 12                                               # device counts without a device state
    assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1


def test_gaussian_adam_1d_refuses_cpu_tensors_and_bad_arguments(hip_lib):
    from pigs_amd.optim import GaussianAdam1D
    rm, u, rs = torch.zeros(4, 1), torch.ones(4, 3), torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianAdam1D(rm, u, rs)
    with pytest.raises(NotImplementedError):
        GaussianAdam1D(torch.zeros(4, 2), u, torch.zeros(4, 2))                  # d = 2 rows
    with pytest.raises(NotImplementedError):
        GaussianAdam1D(rm, u, torch.zeros(4, 2))
    with pytest.raises(NotImplementedError):
        GaussianAdam1D(rm, torch.ones(4, 5), rs)                                 # c = 5
    with pytest.raises(ValueError):
        GaussianAdam1D(rm, torch.ones(5, 3), rs)                                 # row counts differ
    with pytest.raises(TypeError):
        GaussianAdam1D(rm, u.double(), rs)                                       # mixed dtypes
    with pytest.raises(ValueError):
        GaussianAdam1D(rm, u, rs, means_map="sigmoid")
    with pytest.raises(ValueError):
        GaussianAdam1D(rm, u, rs, means_map="tanh", wrap=(-1.0, 1.0))            # the wrap goes with the identity map
    with pytest.raises(ValueError):
        GaussianAdam1D(rm, u, rs, means_map="identity", wrap=(1.0, -1.0))
    with pytest.raises(ValueError):
        GaussianAdam1D(rm, u, rs, lr={"means": 1e-3, "values": 1e-3, "scaling": 1e-3, "transform": 1e-3})  # three groups
    for kw in ({"weight_decay": 1e-2}, {"amsgrad": True}, {"maximize": True}):
        with pytest.raises(NotImplementedError):
            GaussianAdam1D(rm, u, rs, **kw)


# ---- the recorded loop --------------------------------------------------------------------------------------
class TorchChain1D:
    """The reference's 1-D step behind GaussianAdam1D's interface, any device: test_no_mlp_1d.py:109-111 with autograd,
    then :156-162, torch.optim.Adam and zero_grad."""

    def __init__(self, raw_means, values, raw_scaling, lr, scale):
        self.p = [t.detach().clone().requires_grad_(True) for t in (raw_means, values, raw_scaling)]
        self.scale = scale
        self.optim = torch.optim.Adam(self.p, lr=lr)
        rm = self.p[0]
        self.stats = {"mean_grad": torch.zeros_like(rm), "mean_grad_norm": torch.zeros(rm.shape[0], dtype=rm.dtype, device=rm.device),
                      "scale_grad": torch.zeros_like(rm), "scale_grad_norm": torch.zeros(rm.shape[0], dtype=rm.dtype, device=rm.device)}

    def gaussians(self):
        raw_means, values, scaling = self.p
        means = torch.tanh(raw_means) * self.scale
        covariances = torch.exp(scaling).reshape(-1, 1)
        conics = 1.0 / covariances
        return Gaussians(means, values, covariances, conics)

    def step(self):
        reference_lines(self.stats, self.p[0], self.p[2])
        self.optim.step()
        self.optim.zero_grad()

    def read_stats(self):
        return {k: self.stats[k].detach().cpu().double().numpy() for k in STATS}


def init_1d(device, dtype, n=25):
    """test_no_mlp_1d.py:40-47 with values = 0.1 rand (CPU generator, seed 7, drawn in float64 and cast)"""
    g = torch.Generator(device="cpu").manual_seed(7)
    raw_means = torch.linspace(-1, 1, n, dtype=torch.float64).reshape(-1, 1).to(device=device, dtype=dtype)
    scaling = (torch.ones((n, 1), dtype=torch.float64) * -4.0).to(device=device, dtype=dtype)
    values = (0.1 * torch.rand((n, 1), generator=g, dtype=torch.float64)).to(device=device, dtype=dtype)
    return (raw_means, values, scaling), g


def loop_1d(opt, g, new_sampler, device, dtype, steps=30, n_samples=128, scale=2.5, dt=0.05):
    """test_no_mlp_1d.py:97-153, Burgers: 128 points in (-scale, scale) and a per-point tau per step (both drawn in float64
    and cast), 10 steps fitting exp(-2 x^2), the fitted state frozen at step 10, then the residual
    mean((u_t - (nu u_xx_b - u_b u_x_b))^2) with u, u_x, u_xx blended with the frozen level by tau (:138-142)."""
    nu = 1.0 / (100.0 * np.pi)
    sampler = new_sampler()
    losses, prev = [], None
    for it in range(steps):
        samples = ((torch.rand((n_samples, 1), generator=g, dtype=torch.float64) * 2.0 - 1.0) * scale).to(device=device, dtype=dtype)
        time_samples = torch.rand((n_samples,), generator=g, dtype=torch.float64).to(device=device, dtype=dtype)
        gs = opt.gaussians()
        if it == 10:
            prev = tuple(t.detach().clone() for t in gs)
        if it >= 10:
            with torch.no_grad():
                sampler2 = new_sampler()
                sampler2.preprocess(*prev, samples)
                prev_img = sampler2.sample_gaussians()
                prev_ux = sampler2.sample_gaussians_derivative()
                prev_uxx = sampler2.sample_gaussians_laplacian()
        sampler.preprocess(gs.means, gs.values, gs.covariances, gs.conics, samples)
        img = sampler.sample_gaussians()
        if it < 10:
            desired = torch.exp(-2.0 * samples ** 2).squeeze()
            loss = torch.mean((img[..., 0] - desired) ** 2)
        else:
            ux = sampler.sample_gaussians_derivative()
            uxx = sampler.sample_gaussians_laplacian()
            ut = (img - prev_img) / dt
            u = time_samples.reshape(-1, 1) * prev_img + (1 - time_samples.reshape(-1, 1)) * img
            ux = time_samples.reshape(-1, 1, 1) * prev_ux + (1 - time_samples.reshape(-1, 1, 1)) * ux
            uxx = time_samples.reshape(-1, 1, 1, 1) * prev_uxx + (1 - time_samples.reshape(-1, 1, 1, 1)) * uxx
            loss = torch.mean((ut[:, 0] - (nu * uxx[:, 0, 0, 0] - u[:, 0] * ux[:, 0, 0])) ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


def test_the_1d_fixture():
    """shapes, finiteness, the fit converges, and float32 against float64 as the generator measured them"""
    f = check_fixture(os.path.join(GOLDEN, "grad_stats", "no_mlp_1d.npz"), 25, 1)
    assert f["losses"][9] < f["losses"][0]
    worst = max(float(np.abs(f[k] - f[k + "_f64"]).max()) / scale_of(f[k + "_f64"]) for k in STATS)
    loss = float((np.abs(f["losses"] - f["losses_f64"]) / np.abs(f["losses_f64"])).max())
    print(f"1-D fixture, float32 vs float64: losses {loss:.3g}, statistics {worst:.3g} of an array's scale")
    assert loss < 2e-3 / 70 and worst < 2e-3 / 70                 # precision alone leaves the 2e-3 bar 70 x of room
