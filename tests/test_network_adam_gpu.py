"""GPU: NetworkAdam (pigs_amd/network_adam.py, csrc/network_adam.hip) against the float64 checker of
tests/test_network_adam.py.

Every comparison of parameters and moments is ONE step from a given state.  Bars, those of tests/test_optim_gpu.py:
    float64   1e-11 of each tensor's scale (its largest magnitude).
    float32   the checker is applied to the float32 inputs promoted; the kernel's error against it (RMS over the tensor)
              must stay within 4 x the error of torch's own float32 Adam(foreach=False) on the GPU from the same state plus
              2 ulp of the tensor (2 * 2^-23 * its RMS).
    rate      rate_scale within 1e-12 relative of the products of math.exp in Python: derived, not measured -- both sides
              are a double exp (1 ulp, 2e-16) and at most three double products; a single-precision exp would miss the
              bar by four orders, a double one meets it by three.
Each check prints its figure in units of its bar.
"""
import copy
import math

import numpy as np
import pytest
import torch

import test_step as ts
from test_network_adam import (BETAS, EPS, LR, as_dtype, checker_step, make_grads, make_state, read_torch, scale_of,
                               torch_adam, torch_step)

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}
ULP32 = 2.0 ** -23
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def NetworkAdam(hip_lib):
    assert torch.cuda.is_available()
    import pigs_amd
    return pigs_amd.NetworkAdam


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0


def torch_dict(opt, state, dtype):
    """``state`` as a torch.optim.Adam state dict over ``opt``'s group (every position takes a slot here)"""
    entries = {s: {"step": torch.tensor(float(t)), "exp_avg": dev(state["m"][s], dtype), "exp_avg_sq": dev(state["v"][s], dtype)}
               for s, t in enumerate(state["steps"])}
    return {"state": entries, "param_groups": opt.state_dict()["param_groups"]}


def make_opt(NetworkAdam, state, dtype, lr=LR, capturable=False, params=None):
    params = [dev(a, dtype).requires_grad_(True) for a in state["p"]] if params is None else params
    opt = NetworkAdam(params, lr=lr, betas=BETAS, eps=EPS, capturable=capturable)
    opt.load_state_dict(torch_dict(opt, state, dtype))
    return opt, params


def give_grads(params, grads, dtype):
    for p, g in zip(params, grads):
        p.grad = None if g is None else dev(g, dtype)


def read_opt(opt, params, like):
    """parameters, moments (from the flat arrays, stepped or not) and step counts as float64 numpy"""
    from pigs_amd.network_adam import segment_offsets
    out = copy.deepcopy(like)
    offsets, _ = segment_offsets([p.numel() for p in params])
    m, v = opt.exp_avg_flat.cpu().double().numpy(), opt.exp_avg_sq_flat.cpu().double().numpy()
    for s, (p, at) in enumerate(zip(params, offsets)):
        out["p"][s] = p.detach().cpu().double().numpy().reshape(like["p"][s].shape)
        out["m"][s] = m[at:at + p.numel()].reshape(like["p"][s].shape).copy()
        out["v"][s] = v[at:at + p.numel()].reshape(like["p"][s].shape).copy()
    out["steps"] = opt.steps
    return out


def hold(family, got, want, state, grads, dtype, lr=LR, only=None):
    """what one step wrote against the checker's ``want``, at the bars of the module text; returns the worst figure"""
    assert got["steps"] == want["steps"], (family, got["steps"], want["steps"])
    tensors = range(len(want["p"])) if only is None else only
    worst = 0.0
    if dtype == torch.float64:
        for k in ("p", "m", "v"):
            for s in tensors:
                fig = float(np.abs(got[k][s] - want[k][s]).max()) / (1e-11 * scale_of(want[k][s]))
                worst = max(worst, fig)
                assert fig <= 1.0, f"{family} {k}[{s}]: {fig:.3g} x the float64 bar"
    else:
        params, adam = torch_adam(state, torch.float32, "cuda", lr=lr)
        torch_step(params, adam, grads)
        ref = read_torch(params, adam, state)
        for k in ("p", "m", "v"):
            for s in tensors:
                bar = 4.0 * rms(ref[k][s] - want[k][s]) + 2.0 * ULP32 * rms(want[k][s])
                fig = rms(got[k][s] - want[k][s]) / max(bar, 1e-300)
                worst = max(worst, fig)
                assert fig <= 1.0, f"{family} {k}[{s}]: {fig:.3g} x the float32 bar"
    print(f"[figure] {family} {str(dtype)[6:]}: worst {worst:.3g} x its bar")
    return worst


def rounded(state, grads, dtype):
    return as_dtype(state, NP[dtype]), [None if g is None else g.astype(NP[dtype]).astype(np.float64) for g in grads]


def one_step(NetworkAdam, family, state, grads, dtype, lr=LR, capturable=False, **step_args):
    """ONE step on the GPU from ``state``, held to its bar; returns (opt, params, got, want)"""
    state, grads = rounded(state, grads, dtype)
    want = checker_step(state, grads, lr=lr)
    opt, params = make_opt(NetworkAdam, state, dtype, lr, capturable)
    give_grads(params, grads, dtype)
    opt.step(**step_args)
    assert all(p.grad is None for p in params)
    got = read_opt(opt, params, state)
    hold(family, got, want, state, grads, dtype, lr)
    return opt, params, got, want


def shapes_of(counts):
    return [(n,) for n in counts]


# ---- one step against the checker ---------------------------------------------------------------------------
@DTYPES
def test_sizes_where_the_kernel_can_go_wrong(NetworkAdam, dtype):
    """a single element, the vector tail (3, 5), a whole vector (4), the chunk's edge (1 023, 1 024, 1 025) and three
    chunks (2 049), in one optimiser"""
    shapes = shapes_of([1, 3, 4, 5, 1023, 1024, 1025, 2049])
    state = make_state(shapes, seed=1, moments=True, steps=3)
    one_step(NetworkAdam, "sizes", state, make_grads(shapes, seed=2), dtype)


@DTYPES
@pytest.mark.parametrize("tensors", [1, 128])
def test_smallest_and_largest_tables(NetworkAdam, dtype, tensors):
    shapes = shapes_of([7] * tensors)
    state = make_state(shapes, seed=3, moments=True, steps=list(range(1, tensors + 1)))
    one_step(NetworkAdam, f"{tensors} tensors", state, make_grads(shapes, seed=4), dtype)


@DTYPES
def test_unaligned_view_takes_the_scalar_path_with_the_same_bits(NetworkAdam, dtype):
    """a parameter that is a contiguous view one element (float32: 4 bytes) into a buffer, its gradient likewise, beside
    an aligned copy with the same values, gradient and state: the 16-byte and the scalar path give the same bits"""
    n = 2051
    shapes = [(n,), (n,)]
    state = make_state([(n,)], seed=5, moments=True, steps=4)
    state = {k: v * 2 for k, v in state.items()}                       # the same tensor twice
    (g,) = make_grads([(n,)], seed=6)
    state, grads = rounded(state, [g, g], dtype)

    def view(a):
        buf = torch.zeros(n + 1, dtype=dtype, device="cuda")
        buf[1:].copy_(dev(a, dtype))
        return buf[1:]
    params = [view(state["p"][0]).requires_grad_(True), dev(state["p"][1], dtype).requires_grad_(True)]
    assert params[0].data_ptr() % 16 != 0 and params[1].data_ptr() % 16 == 0 and params[0].is_contiguous()
    opt, _ = make_opt(NetworkAdam, state, dtype, params=params)
    params[0].grad, params[1].grad = view(grads[0]), dev(grads[1], dtype)
    assert params[0].grad.data_ptr() % 16 != 0 and params[1].grad.data_ptr() % 16 == 0
    opt.step()
    got = read_opt(opt, params, state)
    hold("unaligned view", got, checker_step(state, grads), state, grads, dtype)
    for k in ("p", "m", "v"):
        assert np.array_equal(got[k][0], got[k][1]), k
    assert shapes == [tuple(p.shape) for p in params]


@DTYPES
def test_presence(NetworkAdam, dtype):
    """grad is None for tensors in the middle of the table: their parameters and moments are bitwise unchanged and their
    step is not advanced; the next step, all present, runs with differing step counts"""
    shapes = [(5,), (1025,), (33, 3), (1024,), (7,), (2049,)]
    state = make_state(shapes, seed=7, moments=True, steps=[3, 5, 2, 2, 9, 1])
    grads = make_grads(shapes, seed=8, absent=(2, 3))
    opt, params, got, want = one_step(NetworkAdam, "presence, two absent", state, grads, dtype)
    start = as_dtype(state, NP[dtype])
    for s in (2, 3):
        assert all(np.array_equal(got[k][s], start[k][s]) for k in ("p", "m", "v")), s
    assert got["steps"] == [4, 6, 2, 2, 10, 2]
    assert [int(opt.state[p]["step"]) for p in params] == got["steps"]
    grads2 = rounded(state, make_grads(shapes, seed=9), dtype)[1]
    give_grads(params, grads2, dtype)
    opt.step()
    after = read_opt(opt, params, state)
    assert after["steps"] == [5, 7, 3, 3, 11, 3]
    hold("presence, the next step", after, checker_step(got, grads2), got, grads2, dtype)


@DTYPES
def test_frozen_parameter(NetworkAdam, dtype):
    """a requires_grad=False tensor in the list (the model's ``frequencies``): bitwise unchanged, absent from the state"""
    shapes = [(17,), (6,), (1030,)]
    state, grads = rounded(make_state(shapes, seed=10), make_grads(shapes, seed=11), dtype)
    params = [dev(a, dtype).requires_grad_(k != 1) for k, a in enumerate(state["p"])]
    opt = NetworkAdam(params, lr=LR, betas=BETAS, eps=EPS)
    frozen = params[1].clone()
    give_grads([params[0], params[2]], [grads[0], grads[2]], dtype)
    opt.step()
    assert torch.equal(params[1], frozen) and params[1] not in opt.state and opt.steps == [1, 1]
    assert sorted(opt.state_dict()["state"]) == [0, 2] and opt.state_dict()["param_groups"][0]["params"] == [0, 1, 2]
    want = checker_step(state, [grads[0], None, grads[2]])
    for s in (0, 2):
        bar = 1e-11 if dtype == torch.float64 else 4 * ULP32             # a first step is lr * sign(g) off the parameter
        assert np.abs(params[s].detach().cpu().double().numpy() - want["p"][s]).max() <= bar * scale_of(want["p"][s])


def network_shapes():
    """the reference DynamicsNetwork's 90 trainable shapes at c = 2: the 36 of the input transform, then the 54 of
    tests/test_step.py's Network"""
    from pigs_amd.input_transform import param_shapes
    net = ts.Network(ts.fixture_scene("navier_stokes").sd)
    shapes = [tuple(s) for s in param_shapes(2, 1)] + [tuple(p.shape) for _, p in net.named_parameters()]
    assert len(shapes) == 90
    return shapes


@DTYPES
def test_reference_networks_shapes_five_steps(NetworkAdam, dtype):
    """five steps with fixed random gradients, each held as ONE step from the state the GPU had before it"""
    shapes = network_shapes()
    state = rounded(make_state(shapes, seed=12), [], dtype)[0]
    opt, params = make_opt(NetworkAdam, state, dtype)
    for it in range(5):
        grads = rounded(state, make_grads(shapes, seed=13 + it), dtype)[1]
        give_grads(params, grads, dtype)
        opt.step()
        got = read_opt(opt, params, state)
        hold(f"reference network, step {it + 1}", got, checker_step(state, grads), state, grads, dtype)
        state = got
    assert state["steps"] == [5] * 90


# ---- the rate, the loss statistics, the resets --------------------------------------------------------------
LOSSES = (0.3, 0.0, 2.0)


@DTYPES
def test_rate_scale_loss_statistics_and_resets(NetworkAdam, dtype):
    """three steps with loss = 0.3, 0.0, 2.0 and decay = 1 from rate_scale = 1: each step runs at lr * rate_scale from
    BEFORE its decay; rate_scale follows the products of math.exp; loss_stats() is (2.3, 2.0, 3); the resets restore 1 and
    zeros.  The loss tensors have the parameters' dtype (both loss dtypes of the ABI)"""
    shapes = [(5,), (1030,), (16, 16)]
    state = rounded(make_state(shapes, seed=20, moments=True, steps=2), [], dtype)[0]
    opt, params = make_opt(NetworkAdam, state, dtype)
    assert float(opt.rate_scale) == 1.0 and opt.rate_scale.dim() == 0 and opt.loss_stats() == (0.0, 0.0, 0)
    scale, total = 1.0, 0.0
    for it, value in enumerate(LOSSES):
        loss = dev(value, dtype)
        stored = float(loss)                                             # 0.3 as the loss's dtype holds it
        grads = rounded(state, make_grads(shapes, seed=21 + it), dtype)[1]
        give_grads(params, grads, dtype)
        opt.step(loss=loss, decay=1.0)
        got = read_opt(opt, params, state)
        hold(f"rate, step {it + 1} at {scale:.3g} x lr", got, checker_step(state, grads, lr=LR * scale), state, grads,
             dtype, lr=LR * scale)
        scale *= math.exp(-1.0 * stored)
        total += stored
        fig = abs(float(opt.rate_scale) - scale) / scale / 1e-12
        print(f"[figure] rate_scale after step {it + 1}: {fig:.3g} x its bar")
        assert fig <= 1.0
        state = got
    stats = opt.loss_stats()
    assert stats == (total, 2.0, 3) and abs(stats[0] - 2.3) <= 2.3e-7, stats
    opt.reset_rate_scale()
    assert float(opt.rate_scale) == 1.0 and opt.loss_stats() == stats
    opt.reset_loss_stats()
    assert opt.loss_stats() == (0.0, 0.0, 0) and float(opt.rate_scale) == 1.0
    # a step without a loss leaves the rate and the sums alone
    give_grads(params, make_grads(shapes, seed=25), dtype)
    opt.step()
    assert opt.loss_stats() == (0.0, 0.0, 0) and float(opt.rate_scale) == 1.0


@DTYPES
@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_mutable_lr(NetworkAdam, dtype, capturable):
    """eager: param_groups[0]["lr"] *= 0.5 between steps (main_pn.py:217-218); capturable: lr_tensor written in place"""
    shapes = [(9,), (1025,)]
    state = rounded(make_state(shapes, seed=30, moments=True, steps=1), [], dtype)[0]
    opt, params = make_opt(NetworkAdam, state, dtype, capturable=capturable)
    assert (opt.lr_tensor is not None) == capturable
    for it, lr in enumerate((LR, 0.5 * LR)):
        if it == 1:
            if capturable:
                opt.lr_tensor.mul_(0.5)
                opt.param_groups[0]["lr"] = 123.0                        # not what this mode reads
            else:
                opt.param_groups[0]["lr"] *= 0.5
        grads = rounded(state, make_grads(shapes, seed=31 + it), dtype)[1]
        give_grads(params, grads, dtype)
        opt.step()
        got = read_opt(opt, params, state)
        hold(f"mutable lr, step {it + 1}", got, checker_step(state, grads, lr=lr), state, grads, dtype, lr=lr)
        state = got


def assert_bitwise(a, pa, b, pb):
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert torch.equal(a.exp_avg_flat, b.exp_avg_flat) and torch.equal(a.exp_avg_sq_flat, b.exp_avg_sq_flat)
    assert torch.equal(a._state_tensor, b._state_tensor)


@DTYPES
def test_zero_rate_and_eager_capturable_agreement(NetworkAdam, dtype):
    """a zero rate leaves the parameters bitwise and moves the moments; eager and capturable=True give the same bits, at
    the zero rate and at an ordinary one"""
    shapes = [(5,), (1030,), (16, 16)]
    state = rounded(make_state(shapes, seed=40, moments=True, steps=4), [], dtype)[0]
    for lr in (0.0, LR):
        grads = rounded(state, make_grads(shapes, seed=41), dtype)[1]
        eager, pe = make_opt(NetworkAdam, state, dtype, lr=lr)
        device, pd = make_opt(NetworkAdam, state, dtype, lr=lr, capturable=True)
        for opt, params in ((eager, pe), (device, pd)):
            give_grads(params, grads, dtype)
            opt.step(loss=dev(0.5, torch.float64), decay=2.0)
        assert_bitwise(eager, pe, device, pd)
        got = read_opt(eager, pe, state)
        assert got["steps"] == [5, 5, 5]
        for s in range(3):
            assert np.array_equal(got["p"][s], state["p"][s]) == (lr == 0.0)
            assert not np.array_equal(got["m"][s], state["m"][s]) and not np.array_equal(got["v"][s], state["v"][s])


def test_graph_replay_of_the_step_alone(NetworkAdam):
    """torch.cuda.graph around step(loss=, decay=) with the gradients and the loss in static tensors: three replays are
    bit-equal to three eager steps from the same state, rate_scale and the loss sums included"""
    dtype = torch.float32
    shapes = [(5,), (1030,), (16, 16), (2049,)]
    state = rounded(make_state(shapes, seed=50, moments=True, steps=[0, 2, 2, 7]), [], dtype)[0]
    grads = [make_grads(shapes, seed=51 + k, absent=(2,)) for k in range(3)]
    losses = (0.7, 0.1, 1.3)
    eager, pe = make_opt(NetworkAdam, state, dtype)
    for k in range(3):
        give_grads(pe, grads[k], dtype)
        eager.step(loss=dev(losses[k], dtype), decay=0.5)
    opt, params = make_opt(NetworkAdam, state, dtype, capturable=True)
    static = [None if g is None else torch.zeros(g.shape, dtype=dtype, device="cuda") for g in grads[0]]
    static_loss = torch.zeros((), dtype=dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for p, g in zip(params, static):
        p.grad = g
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        opt.step(loss=static_loss, decay=0.5)
    torch.cuda.current_stream().wait_stream(side)
    assert opt.steps == [0, 2, 2, 7] and float(opt.rate_scale) == 1.0      # a capture runs nothing
    assert all(p.grad is None for p in params)
    for k in range(3):
        for s, g in zip(static, grads[k]):
            if s is not None:
                s.copy_(dev(g, dtype))
        static_loss.copy_(dev(losses[k], dtype))
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps == [3, 5, 2, 10]
    assert_bitwise(eager, pe, opt, params)
    assert opt.loss_stats() == eager.loss_stats() and opt.loss_stats()[2] == 3


def test_checkpoints(NetworkAdam):
    """two steps, state_dict(); a fresh NetworkAdam and a torch.optim.Adam each load it: the fresh NetworkAdam's third step
    is bit-equal to the uninterrupted third step, torch's is within the float32 bar.  Tensor 1 never has a gradient
    (no entry in the state dict), tensor 2 misses the first step"""
    dtype = torch.float32
    shapes = [(5,), (12,), (1030,), (16, 16)]
    state = rounded(make_state(shapes, seed=60), [], dtype)[0]
    params = [dev(a, dtype).requires_grad_(True) for a in state["p"]]
    opt = NetworkAdam(params, lr=LR, betas=BETAS, eps=EPS)
    for it in range(2):
        give_grads(params, make_grads(shapes, seed=61 + it, absent=(1, 2) if it == 0 else (1,)), dtype)
        opt.step()
    saved = copy.deepcopy(opt.state_dict())
    assert sorted(saved["state"]) == [0, 2, 3] and [float(saved["state"][k]["step"]) for k in (0, 2, 3)] == [2.0, 1.0, 2.0]
    assert all(saved["state"][k]["step"].dtype == torch.float32 and saved["state"][k]["exp_avg"].shape == shapes[k]
               for k in (0, 2, 3))
    before = read_opt(opt, params, state)
    fresh_params = [p.detach().clone().requires_grad_(True) for p in params]
    fresh = NetworkAdam(fresh_params, lr=5.0, betas=BETAS, eps=EPS, capturable=True)
    fresh.load_state_dict(saved)
    torch_params = [p.detach().clone().requires_grad_(True) for p in params]
    adam = torch.optim.Adam(torch_params, lr=5.0, betas=BETAS, eps=EPS, foreach=False)
    adam.load_state_dict(copy.deepcopy(saved))
    assert fresh.steps == opt.steps == [2, 0, 1, 2] and fresh.param_groups[0]["lr"] == LR == adam.param_groups[0]["lr"]
    grads = rounded(state, make_grads(shapes, seed=63), dtype)[1]
    for o, ps in ((opt, params), (fresh, fresh_params)):
        give_grads(ps, grads, dtype)
        o.step()
    for a, b in zip(params, fresh_params):
        assert torch.equal(a, b)
    assert torch.equal(opt.exp_avg_flat, fresh.exp_avg_flat) and torch.equal(opt.exp_avg_sq_flat, fresh.exp_avg_sq_flat)
    assert torch.equal(opt._state_tensor, fresh._state_tensor)
    torch_step(torch_params, adam, grads)
    want = checker_step(before, grads)
    ref = read_torch(torch_params, adam, before)
    assert ref["steps"] == want["steps"] == [3, 1, 2, 3]
    ours = read_opt(opt, params, state)
    for k in ("p", "m", "v"):
        for s in range(len(shapes)):
            # torch's step from our state dict against the checker: within the float32 bar taken with OUR error
            bar = 4.0 * rms(ours[k][s] - want[k][s]) + 2.0 * ULP32 * rms(want[k][s])
            assert rms(ref[k][s] - want[k][s]) <= bar, (k, s)


def test_version_counters_and_gradients(NetworkAdam):
    """a stale autograd node complains as it would after torch.optim; a gradient of the wrong dtype or layout is refused
    with the tensor's position"""
    params = [torch.nn.Parameter(dev(np.ones(n), torch.float32)) for n in (5, 9)]
    opt = NetworkAdam(params, lr=1e-2)
    stale = [(p ** 2).sum() for p in params]
    versions = [p._version for p in params]
    params[1].grad = torch.ones(9, device="cuda")
    opt.step()
    assert params[1]._version > versions[1] and params[0]._version == versions[0]
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        stale[1].backward()
    stale[0].backward()
    params[0].grad = None
    params[1].grad = torch.ones(18, device="cuda")[::2]
    with pytest.raises(TypeError, match="parameter 1"):
        opt.step()
    with pytest.raises(TypeError):
        opt.step(loss=torch.zeros(2, device="cuda"))
    opt.zero_grad()
    assert all(p.grad is None for p in params)
    with pytest.raises(ValueError, match="ONE parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(3, device="cuda"))]})


# ---- launches -----------------------------------------------------------------------------------------------
def test_launch_count(NetworkAdam, hip_lib, monkeypatch):
    """one call of pigs_network_adam_step per step -- the entry launches its two kernels and nothing else -- and none with
    no gradient anywhere; pigs_network_adam_state_doubles is called at construction only"""
    calls = {"pigs_network_adam_step": 0, "pigs_network_adam_state_doubles": 0}

    def counting(name):
        fn = getattr(hip_lib, name)

        def wrapper(*args):
            calls[name] += 1
            return fn(*args)
        return wrapper
    for name in calls:
        monkeypatch.setattr(hip_lib, name, counting(name))
    shapes = network_shapes()
    state = make_state(shapes, seed=70)
    opt, params = make_opt(NetworkAdam, state, torch.float32)
    assert calls == {"pigs_network_adam_step": 0, "pigs_network_adam_state_doubles": 1}
    opt.step()                                                          # no gradient anywhere
    assert calls["pigs_network_adam_step"] == 0 and opt.steps == [0] * 90
    for it in range(3):
        give_grads(params, make_grads(shapes, seed=71 + it), torch.float32)
        opt.step(loss=dev(0.1, torch.float32), decay=1.0)
    assert calls == {"pigs_network_adam_step": 3, "pigs_network_adam_state_doubles": 1}
    assert opt.steps == [3] * 90 and opt.loss_stats()[2] == 3
