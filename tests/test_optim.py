"""CPU: the optimiser (pigs_amd/optim.py, csrc/optim.hip) -- its float64 checker against torch.optim.Adam plus autograd,
the wrap against the reference's lines, the refinement surgery against INTEGRATION.md's recipe, the C ABI's refusals.
No GPU call is made here.

The checker, shared with tests/test_optim_gpu.py:
    make_state()     a starting state: parameters, moments, per-group step counts (float64 numpy)
    make_grads()     gradients with respect to (means, values, covariances, conics), any of them None
    forward()        the parameterisation: means, covariances, conics
    checker_step()   ONE step from a given state: chain rule (sech^2 = 4e / (1 + e)^2, e = exp(-2|x|)), Adam as
                     torch.optim.Adam defines it, the wrap, the next Gaussians
Every comparison is one step from a given state; trajectories of parameters are never compared (a first Adam step is
lr * sign(g): a last-bit difference in a near-zero gradient flips an entry by 2 lr).
"""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_refine import random_masks, refine_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("means", "values", "scaling", "transform")
RATES = {"means": 5e-3, "values": 1e-3, "scaling": 5e-2, "transform": 2e-2}      # four distinct (test_initialize.py:80-85)
BETAS, EPS = (0.9, 0.999), 1e-8


# ---- the checker --------------------------------------------------------------------------------------------
def make_state(N, c, seed, t_max=3.0, steps=0, moments=False):
    """raw_means N(0, 0.8), values N(0, 1), raw_scaling U[-4, -1], transform U[-t_max, t_max]; moments zero or random
    (exp_avg N(0, 1), exp_avg_sq chi^2); ``steps``: an int or a dict per group."""
    rng = np.random.default_rng(seed)
    p = {"means": 0.8 * rng.standard_normal((N, 2)), "values": rng.standard_normal((N, c)),
         "scaling": rng.uniform(-4.0, -1.0, (N, 2)), "transform": rng.uniform(-t_max, t_max, (N, 1))}
    if moments:
        m = {g: rng.standard_normal(p[g].shape) for g in GROUPS}
        v = {g: rng.standard_normal(p[g].shape) ** 2 for g in GROUPS}
    else:
        m = {g: np.zeros_like(p[g]) for g in GROUPS}
        v = {g: np.zeros_like(p[g]) for g in GROUPS}
    steps = dict(steps) if isinstance(steps, dict) else {g: int(steps) for g in GROUPS}
    return {"p": p, "m": m, "v": v, "steps": steps}


def make_grads(N, c, seed, present=(True, True, False, True)):
    """(d means [N,2], d values [N,c], d covariances [N,3], d conics [N,3]); None where not present"""
    rng = np.random.default_rng(seed + 104729)
    shapes = ((N, 2), (N, c), (N, 3), (N, 3))
    return tuple(rng.standard_normal(s) if on else None for s, on in zip(shapes, present))


def as_dtype(state, dtype):
    """the state rounded to ``dtype`` and promoted back to float64: what a float32 run starts from"""
    out = copy.deepcopy(state)
    for k in ("p", "m", "v"):
        out[k] = {g: a.astype(dtype).astype(np.float64) for g, a in state[k].items()}
    return out


def sech2(x):
    e = np.exp(-2.0 * np.abs(x))
    return 4.0 * e / (1.0 + e) ** 2


def cov_terms(raw_scaling, t):
    s0, s1 = np.exp(raw_scaling[:, 0]), np.exp(raw_scaling[:, 1])
    h = np.tanh(t)
    k = 1.0 / sech2(t)                                            # 1 / (1 - h^2), no cancellation
    return s0, s1, h, np.sqrt(s0 * s1), k


def forward(p, means_map="tanh", scale=1.0):
    means = np.tanh(p["means"]) * scale if means_map == "tanh" else p["means"].copy()
    s0, s1, h, r, k = cov_terms(p["scaling"], p["transform"].reshape(-1))
    cov = np.stack((s0, h * r, s1), -1)
    con = np.stack((k / s0, -h * k / r, k / s1), -1)
    return means, cov, con


def chain_rule(p, grads, means_map="tanh", scale=1.0):
    """gradients of the raw parameters per group (None = group absent)"""
    g_means, g_values, g_cov, g_con = grads
    out = {g: None for g in GROUPS}
    if g_means is not None:
        out["means"] = g_means * scale * sech2(p["means"]) if means_map == "tanh" else g_means.copy()
    if g_values is not None:
        out["values"] = g_values.copy()
    if g_cov is not None or g_con is not None:
        s0, s1, h, r, k = cov_terms(p["scaling"], p["transform"].reshape(-1))
        g = np.zeros((len(s0), 3)) if g_cov is None else g_cov
        q = np.zeros((len(s0), 3)) if g_con is None else g_con
        # covariance (s0, h r, s1), conic (k / s0, -h k / r, k / s1): partials with respect to s0, s1, r, h, k
        d_r = g[:, 1] * h + q[:, 1] * h * k / r ** 2
        d_s0 = g[:, 0] - q[:, 0] * k / s0 ** 2 + d_r * r / (2.0 * s0)
        d_s1 = g[:, 2] - q[:, 2] * k / s1 ** 2 + d_r * r / (2.0 * s1)
        d_k = q[:, 0] / s0 + q[:, 2] / s1 - q[:, 1] * h / r
        d_h = g[:, 1] * r - q[:, 1] * k / r + d_k * 2.0 * h * k ** 2            # dk/dh = 2 h k^2
        out["scaling"] = np.stack((d_s0 * s0, d_s1 * s1), -1)                    # ds/d raw = s
        out["transform"] = (d_h / k).reshape(p["transform"].shape)              # dh/dt = sech^2 = 1 / k
    return out


def checker_step(state, grads, lr=RATES, betas=BETAS, eps=EPS, means_map="tanh", scale=1.0, wrap=None):
    """ONE step.  Returns (new state, (means, covariances, conics) of the new parameters)."""
    new = copy.deepcopy(state)
    raw = chain_rule(state["p"], grads, means_map, scale)
    b1, b2 = betas
    for g in GROUPS:
        if raw[g] is None:
            continue
        t = new["steps"][g] = state["steps"][g] + 1
        m = new["m"][g] = b1 * state["m"][g] + (1.0 - b1) * raw[g]
        v = new["v"][g] = b2 * state["v"][g] + (1.0 - b2) * raw[g] ** 2
        step_size = lr[g] / (1.0 - b1 ** t)
        new["p"][g] = state["p"][g] - step_size * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    if wrap is not None and raw["means"] is not None:
        lo, hi = wrap
        x = new["p"]["means"]
        x = np.where(x > hi, x - (hi - lo), x)
        new["p"]["means"] = np.where(x < lo, x + (hi - lo), x)
    return new, forward(new["p"], means_map, scale)


def scale_of(a):
    return max(float(np.abs(a).max()), 1e-300)


# ---- the checker against torch.optim.Adam and autograd ------------------------------------------------------
def torch_state(state, dtype=torch.float64, device="cpu"):
    """parameters as leaves and an Adam(foreach=False) over them carrying the state's moments and counts"""
    params = {g: torch.tensor(state["p"][g], dtype=dtype, device=device, requires_grad=True) for g in GROUPS}
    optim = torch.optim.Adam([{"params": [params[g]], "lr": RATES[g]} for g in GROUPS], betas=BETAS, eps=EPS, foreach=False)
    for g in GROUPS:
        if state["steps"][g] > 0 or np.any(state["m"][g]) or np.any(state["v"][g]):
            optim.state[params[g]] = {"step": torch.tensor(float(state["steps"][g])),
                                      "exp_avg": torch.tensor(state["m"][g], dtype=dtype, device=device),
                                      "exp_avg_sq": torch.tensor(state["v"][g], dtype=dtype, device=device)}
    return params, optim


def torch_step(params, optim, grads, means_map="tanh", scale=1.0, wrap=None):
    """tanh / exp / synthetic.covariances_from_raw, autograd from the given gradients, Adam, zero_grad, the wrap"""
    from pigs_amd import synthetic
    ref = params["means"]
    means = torch.tanh(params["means"]) * scale if means_map == "tanh" else params["means"]
    cov, con = synthetic.covariances_from_raw(torch.exp(params["scaling"]), params["transform"])
    loss = None
    for out, g in zip((means, params["values"], cov, con), grads):
        if g is not None:
            term = (out * torch.as_tensor(g, dtype=ref.dtype, device=ref.device)).sum()
            loss = term if loss is None else loss + term
    optim.zero_grad(set_to_none=True)
    loss.backward()
    optim.step()
    if wrap is not None and params["means"].grad is not None:
        lo, hi = wrap
        with torch.no_grad():                                     # test_initialize.py:175-180
            raw_means = params["means"]
            oob = raw_means > hi
            raw_means[oob] -= hi - lo
            oob = raw_means < lo
            raw_means[oob] += hi - lo


def read_torch(params, optim, like):
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


def assert_states_agree(got, want, bar, what=""):
    worst = 0.0
    for k in ("p", "m", "v"):
        for g in GROUPS:
            err = float(np.abs(got[k][g] - want[k][g]).max()) / scale_of(want[k][g])
            worst = max(worst, err)
            assert err <= bar, f"{what} {k}[{g}]: {err:.3g} of its scale > {bar:.3g}"
    assert got["steps"] == want["steps"], (what, got["steps"], want["steps"])
    return worst


def test_checker_agrees_with_torch_adam_and_autograd():
    """float64 on the CPU, five consecutive steps, each compared as ONE step from torch's state before it:
    N = 257, c = 2, |t| <= 3, four distinct rates; the project's float64 bar, 1e-12 of each tensor's scale"""
    N, c = 257, 2
    state = make_state(N, c, seed=1, t_max=3.0)
    params, optim = torch_state(state)
    worst = 0.0
    for it in range(5):
        grads = make_grads(N, c, seed=10 + it, present=(True, True, it % 2 == 1, True))
        before = read_torch(params, optim, state)
        torch_step(params, optim, grads, "tanh", 2.5)
        want = read_torch(params, optim, state)
        got, _ = checker_step(before, grads, means_map="tanh", scale=2.5)
        worst = max(worst, assert_states_agree(got, want, 1e-12, f"step {it}"))
        assert want["steps"] == {g: it + 1 for g in GROUPS}
    print(f"checker vs torch.optim.Adam + autograd, float64: worst {worst:.3g} of a tensor's scale")


def test_checker_forward_is_the_reference_composition():
    from pigs_amd import synthetic
    state = make_state(300, 1, seed=2)
    means, cov, con = forward(state["p"], "tanh", 2.5)
    p = {g: torch.tensor(a) for g, a in state["p"].items()}
    tcov, tcon = synthetic.covariances_from_raw(torch.exp(p["scaling"]), p["transform"])
    assert np.abs(means - (torch.tanh(p["means"]) * 2.5).numpy()).max() <= 1e-12 * scale_of(means)
    assert np.abs(cov - tcov.numpy()).max() <= 1e-12 * scale_of(cov)
    assert np.abs(con - tcon.numpy()).max() <= 1e-12 * scale_of(con)
    assert np.array_equal(forward(state["p"], "identity")[0], state["p"]["means"])


PATTERNS = [(a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)
            if a or b or c or d]


@pytest.mark.parametrize("present", PATTERNS, ids=["".join("mvcq"[i] if on else "-" for i, on in enumerate(p)) for p in PATTERNS])
def test_null_gradients_skip_their_group_as_torch_does(present):
    """a group without a gradient keeps parameters, moments and its own step count, here and in torch"""
    N, c = 65, 2
    state = make_state(N, c, seed=3, moments=True, steps={"means": 3, "values": 5, "scaling": 2, "transform": 2})
    grads = make_grads(N, c, seed=4, present=present)
    params, optim = torch_state(state)
    torch_step(params, optim, grads, "identity")
    want = read_torch(params, optim, state)
    got, _ = checker_step(state, grads, means_map="identity")
    assert_states_agree(got, want, 1e-12, str(present))
    on = {"means": present[0], "values": present[1], "scaling": present[2] or present[3],
          "transform": present[2] or present[3]}
    for g in GROUPS:
        assert got["steps"][g] == state["steps"][g] + int(on[g])
        if not on[g]:
            assert all(np.array_equal(got[k][g], state[k][g]) for k in ("p", "m", "v"))


def test_wrap_is_the_reference_four_lines():
    """identity map on (-1, 1) with a rate that throws rows over both edges; exact rows at the edges stay"""
    N, c = 129, 1
    state = make_state(N, c, seed=5)
    state["p"]["means"] = np.random.default_rng(5).uniform(-1.0, 1.0, (N, 2))
    state["p"]["means"][:4] = [[1.0, -1.0], [0.999, -0.999], [1.0 - 1e-12, -1.0 + 1e-12], [0.0, 0.0]]
    grads = make_grads(N, c, seed=6, present=(True, False, False, False))
    lr = dict(RATES, means=0.7)
    params, optim = torch_state(state)
    optim.param_groups[0]["lr"] = 0.7
    torch_step(params, optim, grads, "identity", wrap=(-1.0, 1.0))
    want = read_torch(params, optim, state)
    got, (means, _, _) = checker_step(state, grads, lr=lr, means_map="identity", wrap=(-1.0, 1.0))
    assert np.abs(got["p"]["means"] - want["p"]["means"]).max() <= 1e-12
    moved = np.abs(got["p"]["means"] - state["p"]["means"]) > 1.0
    assert moved.any() and (np.abs(got["p"]["means"]) <= 1.0).all() and np.array_equal(means, got["p"]["means"])
    # one shift, strict inequalities: a coordinate exactly on an edge is left alone
    x = np.array([[1.0, -1.0], [3.5, -3.5]])
    st = {"p": dict(state["p"], means=x), "m": {g: np.zeros((2, 2)) for g in GROUPS}, "v": {g: np.zeros((2, 2)) for g in GROUPS},
          "steps": {g: 0 for g in GROUPS}}
    for g in ("values", "scaling", "transform"):
        st["p"][g] = state["p"][g][:2]
    out, _ = checker_step(st, (np.zeros((2, 2)), None, None, None), means_map="identity", wrap=(-1.0, 1.0))
    assert np.array_equal(out["p"]["means"], [[1.0, -1.0], [1.5, -1.5]])


@pytest.mark.parametrize("mode", ["split", "clone"])
def test_refine_surgery_is_the_integration_recipe(mode):
    """pigs_amd.optim.follow_maps (what GaussianAdam.refine applies per group) against INTEGRATION.md's recipe on a
    real torch.optim.Adam state, and for mode "clone" against test_no_mlp.py:222-233 line for line"""
    from pigs_amd.optim import follow_maps
    N, c = 300, 2
    state = make_state(N, c, seed=7, moments=True, steps=4)
    keep, split = random_masks(N, 0.2, 0.2, 7)
    o = refine_oracle(state["p"]["means"], np.exp(state["p"]["scaling"]), state["p"]["transform"], state["p"]["values"],
                      keep, split, mode=mode)
    source, child = torch.as_tensor(o.source), torch.as_tensor(o.child)
    params, optim = torch_state(state)
    with torch.no_grad():                                         # INTEGRATION.md section 4, the second recipe
        fresh = (child >= 0)[:, None]
        for group in optim.param_groups:
            old = group["params"][0]
            st = optim.state.pop(old, None)
            group["params"][0] = torch.nn.Parameter(old.index_select(0, source).requires_grad_(True))
            for key in ("exp_avg", "exp_avg_sq"):
                carried = st[key].index_select(0, source)
                st[key] = torch.where(fresh, torch.zeros_like(carried), carried)
            optim.state[group["params"][0]] = st
    for g, group in zip(GROUPS, optim.param_groups):
        p, m, v = follow_maps(torch.tensor(state["p"][g]), torch.tensor(state["m"][g]), torch.tensor(state["v"][g]),
                              source, child)
        want = group["params"][0]
        assert torch.equal(p, want.detach()) and p.shape[0] == o.n_kept + o.n_split
        assert torch.equal(m, optim.state[want]["exp_avg"]) and torch.equal(v, optim.state[want]["exp_avg_sq"])
        if mode == "clone":
            k, s = torch.as_tensor(keep), torch.as_tensor(split & keep)
            old_m = torch.tensor(state["m"][g])
            assert torch.equal(p, torch.cat((torch.tensor(state["p"][g])[k], torch.tensor(state["p"][g])[s])))
            assert torch.equal(m, torch.cat((old_m[k], torch.zeros_like(old_m[s])), dim=0))
    # a 1-d transform follows too
    p, m, v = follow_maps(torch.tensor(state["p"]["transform"][:, 0]), torch.tensor(state["m"]["transform"][:, 0]),
                          torch.tensor(state["v"]["transform"][:, 0]), source, child)
    assert p.shape == (len(o.source),) and (m[child >= 0] == 0).all() and (v[child >= 0] == 0).all()


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_optim_materialize", "pigs_optim_step")


def test_symbols_declared_exported_and_bound(hip_lib):
    import pigs_amd
    from pigs_amd import _lib, optim
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION
    assert pigs_amd.GaussianAdam is optim.GaussianAdam
    # struct PigsAdamStep: the binding's layout is the header's (18 doubles, 2 ints, 2 pointers)
    assert ctypes.sizeof(_lib.PigsAdamStep) == 18 * 8 + 2 * 4 + 2 * 8
    assert _lib.PigsAdamStep.device_state.offset == 18 * 8 + 8 + 8


def test_refusals_come_before_any_hip_call(hip_lib):
    """pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    from pigs_amd import _lib
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(1 << 12)
    odd = ctypes.c_void_p((1 << 12) + 4)
    mat, step = hip_lib.pigs_optim_materialize, hip_lib.pigs_optim_step
    assert mat(7, 0, 4, 1.0, *([some] * 6), null) == 2                        # dtype
    assert mat(0, 2, 4, 1.0, *([some] * 6), null) == 2                        # map
    assert mat(0, 0, 0, 1.0, *([some] * 6), null) == 1                        # N = 0
    assert mat(1, 1, -3, 1.0, *([some] * 6), null) == 1                       # N < 0
    for k in range(6):
        args = [some] * 6
        args[k] = null
        assert mat(0, 0, 4, 1.0, *args, null) == 1                            # a null array
    assert mat(0, 0, 4, 1.0, odd, *([some] * 5), null) == 1                   # a row array off its alignment
    assert mat(1, 0, 4, 1.0, some, ctypes.c_void_p((1 << 12) + 8), *([some] * 4), null) == 1

    h = _lib.PigsAdamStep()
    h.means_map = 0
    ok = [some] * 19
    assert step(0, 1, 4, None, *ok, null) == 1                                # null hyper
    assert step(7, 1, 4, ctypes.byref(h), *ok, null) == 2                     # dtype
    assert step(0, 0, 4, ctypes.byref(h), *ok, null) == 2                     # c outside 1..4
    assert step(0, 5, 4, ctypes.byref(h), *ok, null) == 2
    assert step(0, 1, 0, ctypes.byref(h), *ok, null) == 1                     # N <= 0
    assert step(1, 4, -1, ctypes.byref(h), *ok, null) == 1
    h.means_map = 3
    assert step(0, 1, 4, ctypes.byref(h), *ok, null) == 2                     # map
    h.means_map = 1
    for k in list(range(12)) + [16, 17, 18]:                                  # parameters, moments, outputs
        args = list(ok)
        args[k] = null
        assert step(0, 1, 4, ctypes.byref(h), *args, null) == 1, k
    args = list(ok)
    args[12:16] = [null] * 4
    assert step(0, 1, 4, ctypes.byref(h), *args, null) == 1                   # no gradient at all
    for k in (0, 2, 4, 6, 8, 10, 12, 16):                                     # the rows of two: off their alignment
        args = list(ok)
        args[k] = odd
        assert step(0, 1, 4, ctypes.byref(h), *args, null) == 1, k


# ---- the Python surface -------------------------------------------------------------------------------------
def test_gaussian_adam_refuses_cpu_tensors_and_bad_arguments(hip_lib):
    from pigs_amd.optim import GaussianAdam
    rm, u, rs, t = torch.zeros(4, 2), torch.ones(4, 3), torch.zeros(4, 2), torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianAdam(rm, u, rs, t)
    with pytest.raises(NotImplementedError):
        GaussianAdam(torch.zeros(4, 1), u, torch.zeros(4, 1), t)                 # d = 1
    with pytest.raises(NotImplementedError):
        GaussianAdam(rm, torch.ones(4, 5), rs, t)                                # c = 5
    with pytest.raises(ValueError):
        GaussianAdam(rm, torch.ones(5, 3), rs, t)                                # row counts differ
    with pytest.raises(TypeError):
        GaussianAdam(rm, u.double(), rs, t)
    with pytest.raises(ValueError):
        GaussianAdam(rm, u, rs, t, means_map="sigmoid")
    with pytest.raises(ValueError):
        GaussianAdam(rm, u, rs, t, means_map="tanh", wrap=(-1.0, 1.0))           # the wrap goes with the identity map
    with pytest.raises(ValueError):
        GaussianAdam(rm, u, rs, t, means_map="identity", wrap=(1.0, -1.0))
    with pytest.raises(ValueError):
        GaussianAdam(rm, u, rs, t, lr={"means": 1e-3})                           # a dict names all four groups
    for kw in ({"weight_decay": 1e-2}, {"amsgrad": True}, {"maximize": True}):
        with pytest.raises(NotImplementedError):
            GaussianAdam(rm, u, rs, t, **kw)
