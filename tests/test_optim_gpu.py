"""GPU: GaussianAdam (pigs_amd/optim.py, csrc/optim.hip) against the float64 checker of tests/test_optim.py.

Every comparison of parameters and moments is ONE step from a given state.  Bars:
    float64   1e-11 of each tensor's scale (its largest magnitude), on every family including the planted rows.
    float32   on the |t| <= 3 families the checker is applied to the float32 inputs promoted; the kernel's error against
              it (RMS over the tensor) must stay within 4 x the error of torch's own float32 composition on the GPU from
              the same state (tanh / exp / synthetic.covariances_from_raw / Adam(foreach=False)) plus 2 ulp of the tensor
              (2 * 2^-23 * its RMS).  The margin covers different tanh / exp implementations and FMA contraction.
              On the planted |t| = 8 rows torch's float32 1 - h^2 is no reference: there the kernel's worst row-relative
              error (|error| over the largest magnitude of the checker's row) must stay within 4 x the worst such ratio
              of the ordinary rows of the same launch.
Each check prints its figure in units of its bar (DESIGN.md section 18 quotes the worst).
"""
import copy

import numpy as np
import pytest
import torch

from test_optim import (BETAS, EPS, GROUPS, RATES, as_dtype, checker_step, forward, make_grads, make_state, read_torch,
                        scale_of, torch_state, torch_step)
from test_refine import random_masks

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}
MAPS = {"tanh": ("tanh", 2.5, None), "identity": ("identity", 1.0, None), "wrap": ("identity", 1.0, (-1.0, 1.0))}
ULP32 = 2.0 ** -23


@pytest.fixture(scope="module")
def optim(hip_lib):
    assert torch.cuda.is_available()
    from pigs_amd import optim
    return optim


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def products(steps):
    """beta^t as the optimiser forms it: t double multiplications from 1.0"""
    out = {"beta1_pow": {}, "beta2_pow": {}}
    for g in GROUPS:
        p1 = p2 = 1.0
        for _ in range(steps[g]):
            p1 *= BETAS[0]
            p2 *= BETAS[1]
        out["beta1_pow"][g], out["beta2_pow"][g] = p1, p2
    return out


def make_opt(optim, state, dtype, map_name="tanh", lr=RATES, capturable=False, flat_transform=False):
    means_map, scale, wrap = MAPS[map_name]
    params = [dev(state["p"][g], dtype) for g in GROUPS]
    if flat_transform:
        params[3] = params[3][:, 0].contiguous()
    opt = optim.GaussianAdam(*params, lr=lr, betas=BETAS, eps=EPS, means_map=means_map, scale=scale, wrap=wrap,
                             capturable=capturable)
    shape = {g: p.shape for g, p in zip(GROUPS, params)}
    opt.load_state_dict({"step": state["steps"], **products(state["steps"]), "lr": lr, "betas": BETAS, "eps": EPS,
                         "exp_avg": {g: dev(state["m"][g], dtype).reshape(shape[g]) for g in GROUPS},
                         "exp_avg_sq": {g: dev(state["v"][g], dtype).reshape(shape[g]) for g in GROUPS}})
    return opt


def give_grads(opt, grads, dtype):
    for leaf, g in zip(opt.gaussians(), grads):
        if g is not None:
            leaf.grad = dev(g, dtype)


def read_opt(opt, like):
    out = copy.deepcopy(like)
    for g, p in zip(GROUPS, (opt.raw_means, opt.values, opt.raw_scaling, opt.transform)):
        out["p"][g] = p.detach().cpu().double().numpy().reshape(like["p"][g].shape)
        out["m"][g] = opt.exp_avg[g].cpu().double().numpy().reshape(like["p"][g].shape)
        out["v"][g] = opt.exp_avg_sq[g].cpu().double().numpy().reshape(like["p"][g].shape)
    out["steps"] = opt.steps
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0


def tensors_of(state, gaussians):
    out = {f"{k}[{g}]": state[k][g] for k in ("p", "m", "v") for g in GROUPS}
    out.update(zip(("next means", "next covariances", "next conics"), gaussians))
    return out


def one_step(optim, family, state, grads, dtype, map_name="tanh", lr=RATES, flat_transform=False):
    """run ONE step on the GPU from ``state`` and hold everything it wrote to its bar; returns (opt, got, want)"""
    means_map, scale, wrap = MAPS[map_name]
    state = as_dtype(state, NP[dtype])
    grads = tuple(None if g is None else g.astype(NP[dtype]).astype(np.float64) for g in grads)
    want, want_g = checker_step(state, grads, lr=lr, means_map=means_map, scale=scale, wrap=wrap)
    opt = make_opt(optim, state, dtype, map_name, lr, flat_transform=flat_transform)
    give_grads(opt, grads, dtype)
    opt.step()
    got = read_opt(opt, state)
    got_g = [t.detach().cpu().double().numpy() for t in (opt.gaussians().means, opt.gaussians().covariances,
                                                         opt.gaussians().conics)]
    assert got["steps"] == want["steps"], (family, got["steps"], want["steps"])
    worst = 0.0
    if dtype == torch.float64:
        for name, w in tensors_of(want, want_g).items():
            g = tensors_of(got, got_g)[name]
            fig = float(np.abs(g - w).max()) / (1e-11 * scale_of(w))
            worst = max(worst, fig)
            assert fig <= 1.0, f"{family} {name}: {fig:.3g} x the float64 bar"
    else:
        params, adam = torch_state(state, torch.float32, "cuda")
        for group, g in zip(adam.param_groups, GROUPS):
            group["lr"] = lr[g]
        torch_step(params, adam, grads, means_map, scale, wrap)
        ref = read_torch(params, adam, state)
        for k in ("p", "m", "v"):
            for g in GROUPS:
                bar = 4.0 * rms(ref[k][g] - want[k][g]) + 2.0 * ULP32 * rms(want[k][g])
                fig = rms(got[k][g] - want[k][g]) / max(bar, 1e-300)
                worst = max(worst, fig)
                assert fig <= 1.0, f"{family} {k}[{g}]: {fig:.3g} x the float32 bar"
        # the next Gaussians: the kernel's against the float64 forward of the kernel's OWN updated parameters, torch's
        # float32 forward of those same parameters as the yardstick
        own = forward(got["p"], means_map, scale)
        from pigs_amd import synthetic
        tp = {g: dev(got["p"][g], torch.float32) for g in GROUPS}
        tcov, tcon = synthetic.covariances_from_raw(torch.exp(tp["scaling"]), tp["transform"])
        tmeans = torch.tanh(tp["means"]) * scale if means_map == "tanh" else tp["means"]
        for name, g, w, t in zip(("next means", "next covariances", "next conics"), got_g, own, (tmeans, tcov, tcon)):
            bar = 4.0 * rms(t.cpu().double().numpy() - w) + 2.0 * ULP32 * rms(w)
            fig = rms(g - w) / bar
            worst = max(worst, fig)
            assert fig <= 1.0, f"{family} {name}: {fig:.3g} x the float32 bar"
    print(f"[figure] {family} {str(dtype)[6:]} {map_name}: worst {worst:.3g} x its bar")
    return opt, got, want


# ---- one step against the checker ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_one_step_sizes(optim, N):
    state = make_state(N, 2, seed=N, moments=True, steps=3)
    one_step(optim, "sizes", state, make_grads(N, 2, seed=N), torch.float32)


@pytest.mark.parametrize("map_name", ["tanh", "identity", "wrap"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_one_step_channels_dtypes_maps(optim, c, dtype, map_name):
    N = 1025
    state = make_state(N, c, seed=20 + c, moments=True, steps=3)
    one_step(optim, "channels x dtypes x maps", state, make_grads(N, c, seed=30 + c, present=(True, True, c % 2 == 0, True)),
             dtype, map_name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("start", ["zero", "t3", "t1000"])
def test_one_step_starting_states(optim, start, dtype):
    """from zero state (the step is t = 1), from a random state (t = 3), from t = 1 000 (bias corrections near 1)"""
    N, c = 1025, 2
    state = make_state(N, c, seed=41, moments=start != "zero", steps={"zero": 0, "t3": 2, "t1000": 999}[start])
    _, got, _ = one_step(optim, "starting states", state, make_grads(N, c, seed=42), dtype)
    assert got["steps"] == {g: {"zero": 1, "t3": 3, "t1000": 1000}[start] for g in GROUPS}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_transform_as_column_and_as_vector(optim, dtype):
    N, c = 257, 1
    state, grads = make_state(N, c, seed=43, moments=True, steps=1), make_grads(N, c, seed=44)
    a, _, _ = one_step(optim, "transform shapes", state, grads, dtype)
    b, _, _ = one_step(optim, "transform shapes", state, grads, dtype, flat_transform=True)
    assert a.transform.shape == (N, 1) and b.transform.shape == (N,) and b.exp_avg["transform"].shape == (N,)
    assert torch.equal(a.transform[:, 0], b.transform) and torch.equal(a.exp_avg_sq["transform"][:, 0], b.exp_avg_sq["transform"])
    assert torch.equal(a.gaussians().conics, b.gaussians().conics)


PATTERNS = [(m, v, k, q) for k in (False, True) for m in (False, True) for v in (False, True) for q in (False, True)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("present", PATTERNS, ids=["".join("mvcq"[i] if on else "-" for i, on in enumerate(p)) for p in PATTERNS])
def test_presence_patterns(optim, hip_lib, monkeypatch, present, dtype):
    """all eight patterns of (d means, d values, d conics), with and without d covariances: an absent group keeps its
    parameters, its moments and its own step count bit for bit"""
    N, c = 257, 2
    steps = {"means": 3, "values": 5, "scaling": 2, "transform": 2}
    state = make_state(N, c, seed=45, moments=True, steps=steps)
    grads = make_grads(N, c, seed=46, present=present)
    if not any(present):                                          # as torch: nothing moves, nothing is launched
        opt = make_opt(optim, state, dtype)
        leaves = opt.gaussians()
        monkeypatch.setattr(hip_lib, "pigs_optim_step", None)     # a call would raise
        opt.step()
        got, start = read_opt(opt, state), as_dtype(state, NP[dtype])
        assert got["steps"] == steps and opt.gaussians() is leaves
        assert all(np.array_equal(got[k][g], start[k][g]) for k in ("p", "m", "v") for g in GROUPS)
        return
    opt, got, _ = one_step(optim, "presence patterns", state, grads, dtype)
    start = as_dtype(state, NP[dtype])
    on = {"means": present[0], "values": present[1], "scaling": present[2] or present[3],
          "transform": present[2] or present[3]}
    for g in GROUPS:
        assert got["steps"][g] == steps[g] + int(on[g])
        if not on[g]:
            assert all(np.array_equal(got[k][g], start[k][g]) for k in ("p", "m", "v")), g


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("group", GROUPS)
def test_zero_rate_leaves_the_parameter_bitwise_and_moves_its_moments(optim, group, dtype):
    N, c = 257, 2
    state = make_state(N, c, seed=47, moments=True, steps=4)
    grads = make_grads(N, c, seed=48, present=(True, True, True, True))
    _, got, _ = one_step(optim, "zero rate", state, grads, dtype, lr=dict(RATES, **{group: 0.0}))
    start = as_dtype(state, NP[dtype])
    assert np.array_equal(got["p"][group], start["p"][group])
    assert not np.array_equal(got["m"][group], start["m"][group]) and not np.array_equal(got["v"][group], start["v"][group])
    assert got["steps"][group] == 5


def planted(N, c, seed, zero_state):
    """rows 0..15 planted in a family of ordinary rows: |t| = 8 (both signs), s0 / s1 = 1e4 (both ways), every gradient
    of a row exactly 0, every gradient of a row 1e-30"""
    state = make_state(N, c, seed=seed, moments=not zero_state, steps=0 if zero_state else 6)
    grads = list(make_grads(N, c, seed=seed + 1, present=(True, True, True, True)))
    p = state["p"]
    p["transform"][0:4, 0] = [8.0, -8.0, 8.0, -8.0]
    p["scaling"][2:8] = [[-1.0, -1.0 - np.log(1e4)], [-1.0 - np.log(1e4), -1.0], [-2.0, -2.0 - np.log(1e4)],
                         [-2.0 - np.log(1e4), -2.0], [0.0, -np.log(1e4)], [-np.log(1e4), 0.0]]
    for g in grads:
        g[8:12] = 0.0
        g[12:16] = 1e-30
    return state, tuple(grads)


@pytest.mark.parametrize("zero_state", [True, False], ids=["zero_state", "random_state"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_planted_rows(optim, dtype, zero_state):
    N, c, rows = 257, 2, 16
    state, grads = planted(N, c, 49, zero_state)
    state = as_dtype(state, NP[dtype])
    grads = tuple(g.astype(NP[dtype]).astype(np.float64) for g in grads)
    want, want_g = checker_step(state, grads, means_map="tanh", scale=2.5)
    opt = make_opt(optim, state, dtype)
    give_grads(opt, grads, dtype)
    opt.step()
    got = read_opt(opt, state)
    g = opt.gaussians()
    got_t = tensors_of(got, [t.detach().cpu().double().numpy() for t in (g.means, g.covariances, g.conics)])
    assert all(np.isfinite(a).all() for a in got_t.values())
    worst = 0.0
    for name, w in tensors_of(want, want_g).items():
        err = np.abs(got_t[name] - w)
        if dtype == torch.float64:
            fig = float(err.max()) / (1e-11 * scale_of(w))
        else:
            ratio = err.max(-1) / np.maximum(np.abs(w).max(-1), 1e-30)          # per row, relative to the row
            fig = float(ratio[:rows].max()) / max(4.0 * float(ratio[rows:].max()), 1e-300)
        worst = max(worst, fig)
        assert fig <= 1.0, f"planted rows, {name}: {fig:.3g} x the bar"
    # a gradient of exactly 0 from zero state moves nothing
    if zero_state:
        for grp in GROUPS:
            assert np.array_equal(got["p"][grp][8:12], state["p"][grp][8:12]) and not got["m"][grp][8:12].any()
    print(f"[figure] planted rows {str(dtype)[6:]} {'zero' if zero_state else 'random'} state: worst {worst:.3g} x its bar")


# ---- the next step's Gaussians ------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@pytest.mark.parametrize("map_name", ["tanh", "wrap"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_next_gaussians_launch_nothing_and_are_the_materialising_launch(optim, hip_lib, monkeypatch, dtype, map_name, capturable):
    N, c = 1025, 3
    calls = {"pigs_optim_materialize": 0, "pigs_optim_step": 0}

    def counting(name):
        fn = getattr(hip_lib, name)

        def wrapper(*args):
            calls[name] += 1
            return fn(*args)
        return wrapper
    for name in calls:
        monkeypatch.setattr(hip_lib, name, counting(name))
    state = make_state(N, c, seed=50, moments=True, steps=2)
    opt = make_opt(optim, state, dtype, map_name, capturable=capturable)
    first = opt.gaussians()
    assert calls == {"pigs_optim_materialize": 1, "pigs_optim_step": 0}
    assert opt.gaussians() is first and calls["pigs_optim_materialize"] == 1
    assert all(leaf.is_leaf and leaf.requires_grad and leaf.grad is None for leaf in first)
    assert first.values.data_ptr() == opt.values.data_ptr()
    for leaf, g in zip(first, make_grads(N, c, seed=51, present=(True, True, True, True))):
        leaf.grad = dev(g, dtype)
    opt.step()
    assert calls == {"pigs_optim_materialize": 1, "pigs_optim_step": 1}
    assert all(leaf.grad is None for leaf in first)
    after = opt.gaussians()
    assert calls == {"pigs_optim_materialize": 1, "pigs_optim_step": 1} and after is not first
    kept = [t.detach().clone() for t in (after.means, after.covariances, after.conics)]
    opt._next = opt._leaves = None                                # what load_state_dict / refine do: materialise again
    again = opt.gaussians()
    assert calls["pigs_optim_materialize"] == 2
    for a, b in zip(kept, (again.means, again.covariances, again.conics)):
        assert torch.equal(a, b)
    if map_name == "wrap":
        assert float(opt.raw_means.abs().max()) <= 1.0 and torch.equal(again.means, opt.raw_means)


def test_in_place_writes_advance_the_version_counters(optim):
    """a stale autograd node complains as it would after torch.optim"""
    N, c = 65, 1
    state = make_state(N, c, seed=52)
    params = [torch.nn.Parameter(dev(state["p"][g], torch.float32)) for g in GROUPS]
    opt = optim.GaussianAdam(*params, lr=1e-2, means_map="tanh", scale=2.5)
    stale = [(p ** 2).sum() for p in params]                      # each saves its parameter for the backward
    versions = [p._version for p in params]
    give_grads(opt, make_grads(N, c, seed=53, present=(True, True, False, True)), torch.float32)
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions))
    for k in (0, 1, 3):                                           # the groups that had a gradient
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            stale[k].backward()
    assert opt.raw_means is params[0] and isinstance(opt.values, torch.nn.Parameter)


def test_rates_are_mutable_and_state_round_trips(optim):
    N, c = 129, 2
    state = make_state(N, c, seed=54, moments=True, steps=7)
    grads = make_grads(N, c, seed=55)
    a = make_opt(optim, state, torch.float64)
    a.lr = 3e-3                                                   # a float: all four
    assert a.lr == {g: 3e-3 for g in GROUPS}
    a.lr["scaling"] = 7e-2                                        # main_pn.py:217-218: a rate changed between steps
    give_grads(a, grads, torch.float64)
    a.step()
    lr = dict({g: 3e-3 for g in GROUPS}, scaling=7e-2)
    want, _ = checker_step(state, grads, lr=lr, means_map="tanh", scale=2.5)
    got = read_opt(a, state)
    for k in ("p", "m", "v"):
        for g in GROUPS:
            assert np.abs(got[k][g] - want[k][g]).max() <= 1e-11 * scale_of(want[k][g])
    saved = a.state_dict()
    assert saved["step"] == {g: 8 for g in GROUPS} and saved["lr"] == lr
    b = optim.GaussianAdam(*[p.clone() for p in (a.raw_means, a.values, a.raw_scaling, a.transform)], lr=1.0,
                           betas=BETAS, eps=EPS, means_map="tanh", scale=2.5, capturable=True)
    b.load_state_dict(saved)
    for o in (a, b):
        give_grads(o, grads, torch.float64)
        o.step()
    assert b.steps == a.steps == {g: 9 for g in GROUPS}
    for x, y in zip((a.raw_means, a.values, a.raw_scaling, a.transform), (b.raw_means, b.values, b.raw_scaling, b.transform)):
        assert torch.equal(x, y)


# ---- host and device counts; capture ------------------------------------------------------------------------
def assert_bitwise(a, b):
    for x, y in zip((a.raw_means, a.values, a.raw_scaling, a.transform), (b.raw_means, b.values, b.raw_scaling, b.transform)):
        assert torch.equal(x, y)
    for g in GROUPS:
        assert torch.equal(a.exp_avg[g], b.exp_avg[g]) and torch.equal(a.exp_avg_sq[g], b.exp_avg_sq[g]), g
    for x, y in zip(a.gaussians(), b.gaussians()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_host_and_device_counts_give_the_same_bits(optim, dtype):
    """ten steps with capturable=False and capturable=True from one state and fixed gradients; the values group sits
    out every third step, so the per-group counts differ"""
    N, c = 257, 2
    state = make_state(N, c, seed=56, moments=True, steps={"means": 1, "values": 4, "scaling": 0, "transform": 0})
    grads = [make_grads(N, c, seed=57 + k, present=(True, k % 3 != 2, k % 2 == 0, True)) for k in range(10)]
    host, device = make_opt(optim, state, dtype, "wrap"), make_opt(optim, state, dtype, "wrap", capturable=True)
    for k in range(10):
        for opt in (host, device):
            give_grads(opt, grads[k], dtype)
            opt.step()
    assert host.steps == device.steps == {"means": 11, "values": 11, "scaling": 10, "transform": 10}
    assert_bitwise(host, device)
    assert device.state_dict()["beta2_pow"] == host.state_dict()["beta2_pow"]


def test_capture_of_the_optimiser_alone(optim):
    """torch.cuda.graph around step() with static gradient tensors, five replays with the gradients rewritten in place,
    against five eager steps: bitwise; the device counts read 5"""
    N, c, dtype = 257, 2, torch.float32
    state = make_state(N, c, seed=70, moments=True, steps=0)
    grads = [make_grads(N, c, seed=71 + k, present=(True, True, False, True)) for k in range(5)]
    eager = make_opt(optim, state, dtype)
    for k in range(5):
        give_grads(eager, grads[k], dtype)
        eager.step()
    opt = make_opt(optim, state, dtype, capturable=True)
    static = [dev(np.zeros_like(g), dtype) if g is not None else None for g in grads[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaves = opt.gaussians()                                  # materialises: the static buffers exist before the capture
        for leaf, g in zip(leaves, static):
            leaf.grad = g
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    assert opt.steps == {g: 0 for g in GROUPS}                    # a capture runs nothing
    for k in range(5):
        for s, g in zip(static, grads[k]):
            if s is not None:
                s.copy_(dev(g, dtype))
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps == {"means": 5, "values": 5, "scaling": 5, "transform": 5}
    assert_bitwise(eager, opt)


def fit_problem(seed=80, N=256, M=1024):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = int(round(N ** 0.5))
    tx = torch.linspace(-1, 1, n) * 0.6
    gx, gy = torch.meshgrid((tx, tx), indexing="ij")
    raw_means = torch.atanh(torch.stack((gx, gy), dim=-1).reshape(N, 2))
    values = 0.1 * torch.rand((N, 1), generator=g)
    samples = (torch.rand((M, 2), generator=g) * 2 - 1) * 2.5
    target = torch.exp(-0.5 * (samples ** 2).sum(-1) / 0.25)
    return raw_means, values, torch.full((N, 2), -3.0), torch.zeros((N, 1)), samples, target


def test_capture_of_the_whole_step(optim):
    """GraphedStep over preprocess -> sample_gaussians -> mean-square loss -> backward -> opt.step(): dense backend,
    N = 256, 1 024 points, ten replays; the loss of every replay against the eager loop within the project's trajectory
    bar 2e-3 (tests/test_training_gpu.py)"""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    warmup, replays = 3, 10
    problem = fit_problem()

    def build(capturable):
        rm, u, rs, t, samples, target = (x.cuda() for x in problem)
        opt = optim.GaussianAdam(rm, u, rs, t, lr=1e-2, means_map="tanh", scale=2.5, capturable=capturable)
        return opt, GaussianSampler(False), samples, target

    def step_of(opt, sampler):
        def fn(samples, target):
            g = opt.gaussians()
            sampler.preprocess(g.means, g.values, g.covariances, g.conics, samples)
            loss = torch.mean((sampler.sample_gaussians()[:, 0] - target) ** 2)
            loss.backward()
            opt.step()
            return loss.detach()
        return fn

    opt_e, sampler_e, samples, target = build(False)
    fn = step_of(opt_e, sampler_e)
    eager = np.array([float(fn(samples, target)) for _ in range(warmup + replays)])
    holder = {}

    def make_inputs():
        holder["opt"], holder["sampler"], s, t = build(True)
        holder["fn"] = step_of(holder["opt"], holder["sampler"])
        return s, t
    step = GraphedStep(lambda s, t: holder["fn"](s, t), make_inputs, warmup=warmup)
    graphed = np.array([float(step()) for _ in range(replays)])
    assert holder["opt"].steps == {g: warmup + replays for g in GROUPS}
    rel = np.abs(graphed - eager[warmup:]) / np.abs(eager[warmup:])
    print(f"[figure] whole-step capture: worst loss difference {rel.max():.3g} ({rel.max() / 2e-3:.3g} x its bar)")
    assert eager[-1] < eager[0] and np.isfinite(graphed).all()
    assert rel.max() < 2e-3, (rel.max(), graphed, eager)


# ---- the training loop --------------------------------------------------------------------------------------
def run_loop_with_gaussian_adam(optim, sampler, steps, n=16, scale=2.5, dt=0.1):
    """tests/test_training_gpu.py::run_loop with GaussianAdam in place of tanh / exp / covariances_from_raw / Adam"""
    device = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(7)
    tx = torch.linspace(-1, 1, n) * 0.6
    gx, gy = torch.meshgrid((tx, tx), indexing="ij")
    raw_means = torch.atanh(torch.stack((gx, gy), dim=-1).reshape(n * n, 2)).to(device)
    raw_scaling = torch.full((n * n, 2), -3.0, device=device)
    transform = torch.zeros((n * n, 1), device=device)
    values = (0.1 * torch.rand((n * n, 1), generator=g)).to(device)
    opt = optim.GaussianAdam(raw_means, values, raw_scaling, transform, lr=1e-2, means_map="tanh", scale=scale)
    losses, prev = [], None
    for it in range(steps):
        samples = ((torch.rand((1024, 2), generator=g) * 2 - 1) * scale).to(device)
        gs = opt.gaussians()
        if it == 10:
            prev = (gs.means.detach().clone(), gs.values.detach().clone(), gs.covariances.detach().clone(),
                    gs.conics.detach().clone())
        sampler.preprocess(gs.means, gs.values, gs.covariances, gs.conics, samples)
        u = sampler.sample_gaussians()
        if it < 10:
            desired = torch.exp(-0.5 * (samples ** 2).sum(-1) / (0.1 * scale))
            loss = torch.mean((u[:, 0] - desired) ** 2)
        else:
            uxx = sampler.sample_gaussians_laplacian()
            ux = sampler.sample_gaussians_derivative()
            with torch.no_grad():
                sampler2 = sampler.__class__(False, backend=sampler.backend)
                sampler2.preprocess(*prev, samples)
                u_prev = sampler2.sample_gaussians()
            ut = (u - u_prev) / dt
            loss = torch.mean((ut[:, 0] - (uxx[:, 0, 0, 0] + uxx[:, 1, 1, 0])) ** 2) + 1e-3 * torch.mean(ux ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_loss_curve_matches_the_reference_functions(optim, backend):
    """against tests/golden/ref_loss_curve_no_mlp.npz at that file's bar, 2e-3"""
    import os
    from conftest import GOLDEN
    from diff_gaussian_sampling import GaussianSampler
    ref = np.load(os.path.join(GOLDEN, "ref_loss_curve_no_mlp.npz"))["losses"]
    sampler = GaussianSampler(False) if backend == "dense" else GaussianSampler(False, backend="binned")
    gpu = run_loop_with_gaussian_adam(optim, sampler, len(ref))
    rel = np.abs(gpu - ref) / np.maximum(np.abs(ref), 1e-12)
    print(f"[figure] loss curve, {backend}: worst {rel.max():.3g} ({rel.max() / 2e-3:.3g} x its bar)")
    assert rel.max() < 2e-3, (rel.max(), gpu, ref)


# ---- densification ------------------------------------------------------------------------------------------
def test_densification_with_refine_index_and_opt_refine(optim):
    """test_no_mlp.py:198-240: refine_index(mode="clone") + opt.refine, one step before and one after, against the same
    with torch.optim.Adam and INTEGRATION.md's recipe; float64, 1e-11 of each tensor's scale"""
    from pigs_amd import refine_index
    N, c, dtype = 300, 2, torch.float64
    state = make_state(N, c, seed=90)
    keep, split = (dev(m, torch.bool) for m in random_masks(N, 0.15, 0.2, 90))
    split = split & keep
    g1 = make_grads(N, c, seed=91)
    opt = make_opt(optim, state, dtype)
    params, adam = torch_state(state, dtype, "cuda")
    give_grads(opt, g1, dtype)
    opt.step()
    torch_step(params, adam, g1, "tanh", 2.5)

    def agree(what):
        want = read_torch(params, adam, state)
        for g, p in zip(GROUPS, (opt.raw_means, opt.values, opt.raw_scaling, opt.transform)):
            for name, a, w in (("p", p, want["p"][g]), ("m", opt.exp_avg[g], want["m"][g]), ("v", opt.exp_avg_sq[g], want["v"][g])):
                a = a.detach().cpu().numpy()
                assert a.shape == w.shape and np.abs(a - w).max() <= 1e-11 * scale_of(w), (what, name, g)
        assert opt.steps == want["steps"]
    agree("before")
    source, child = refine_index(keep, split, mode="clone")
    rows = int(keep.sum()) + int(split.sum())
    with torch.no_grad():                                         # INTEGRATION.md section 4, the recipe on optim.state
        fresh = (child >= 0)[:, None]
        for g, group in zip(GROUPS, adam.param_groups):
            old = group["params"][0]
            st = adam.state.pop(old, None)
            group["params"][0] = params[g] = torch.nn.Parameter(old.index_select(0, source).requires_grad_(True))
            for key in ("exp_avg", "exp_avg_sq"):
                carried = st[key].index_select(0, source)
                st[key] = torch.where(fresh, torch.zeros_like(carried), carried)
            adam.state[params[g]] = st
    old_values = opt.values.detach().clone()
    new = opt.refine(source, child)
    assert all(p.shape[0] == rows for p in new) and new[0] is opt.raw_means and opt.exp_avg["values"].shape == (rows, c)
    assert (opt.exp_avg["means"][child >= 0] == 0).all() and torch.equal(new[1], old_values.index_select(0, source))
    state = make_state(rows, c, seed=92)                          # shapes for the readers below
    agree("after the surgery")
    g2 = make_grads(rows, c, seed=93)
    gs = opt.gaussians()                                          # materialised again, N' rows
    assert gs.means.shape == (rows, 2) and gs.conics.shape == (rows, 3)
    give_grads(opt, g2, dtype)
    opt.step()
    torch_step(params, adam, g2, "tanh", 2.5)
    agree("after")
    assert opt.steps == {g: 2 for g in GROUPS}
