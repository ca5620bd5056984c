"""GPU: GaussianAdam(grad_stats=True) (pigs_amd/optim.py, csrc/optim.hip: optim_step_stats_kernel) against the float64
checkers of tests/test_optim.py and tests/test_optim_stats.py.  The harness is written over a ``kind`` (the class, its
groups, its checker and torch's composition) so that tests/test_optim_1d_gpu.py drives GaussianAdam1D through it too.

Every comparison of parameters, moments and statistics is ONE step from a given state, the statistics from random
NON-zero sums with counts 3.  Bars, as tests/test_optim_gpu.py has them:
    float64   1e-11 of each tensor's scale.
    float32   the kernel's RMS error against the checker (on the float32 inputs promoted) within 4 x the RMS error of
              torch's own float32 composition on the GPU from the same state plus 2 ulp of the tensor; torch's
              composition includes its ``+=`` and ``torch.norm`` for the statistics (test_no_mlp.py:149-155).
    planted   float32: the worst row-relative error of the planted rows within 4 x the worst of the ordinary rows.
    loops     2e-3: relative for the losses, of each array's scale for the six statistic arrays.
Each check prints its figure in units of its bar (DESIGN.md section 18 quotes the worst).
"""
import copy
import os
import types

import numpy as np
import pytest
import torch

import test_optim as t2
from conftest import GOLDEN
from test_optim import BETAS, EPS, scale_of
from test_optim_gpu import MAPS, NP, ULP32, dev, planted, rms
from test_optim_stats import (STAT_GROUPS, STATS, init_2d, loop_2d, make_stats, read_grad_stats, reference_lines,
                              stats_as_dtype, stats_step, torch_stats)
from test_refine import random_masks

pytestmark = pytest.mark.gpu


def _torch_forward_2d(tp, means_map, scale):
    from pigs_amd import synthetic
    cov, con = synthetic.covariances_from_raw(torch.exp(tp["scaling"]), tp["transform"])
    return (torch.tanh(tp["means"]) * scale if means_map == "tanh" else tp["means"]), cov, con


KIND_2D = types.SimpleNamespace(
    name="d=2", cls="GaussianAdam", d=2, GROUPS=t2.GROUPS, RATES=t2.RATES, make_state=t2.make_state, make_grads=t2.make_grads,
    as_dtype=t2.as_dtype, checker_step=t2.checker_step, forward=t2.forward, chain=t2.chain_rule,
    torch_state=t2.torch_state, torch_step=t2.torch_step, read_torch=t2.read_torch, torch_forward=_torch_forward_2d,
    step_entry="pigs_optim_step_stats", plain_entry="pigs_optim_step", materialize_entry="pigs_optim_materialize",
    steps={"means": 3, "values": 5, "scaling": 2, "transform": 2})


@pytest.fixture(scope="module")
def optim(hip_lib):
    assert torch.cuda.is_available()
    from pigs_amd import optim
    return optim


# ---- the harness --------------------------------------------------------------------------------------------
def products(kind, steps):
    out = {"beta1_pow": {}, "beta2_pow": {}}
    for g in kind.GROUPS:
        p1 = p2 = 1.0
        for _ in range(steps[g]):
            p1 *= BETAS[0]
            p2 *= BETAS[1]
        out["beta1_pow"][g], out["beta2_pow"][g] = p1, p2
    return out


def make_opt(kind, optim, state, stats, dtype, map_name="tanh", capturable=False, grad_stats=True):
    means_map, scale, wrap = MAPS[map_name]
    params = [dev(state["p"][g], dtype) for g in kind.GROUPS]
    opt = getattr(optim, kind.cls)(*params, lr=kind.RATES, betas=BETAS, eps=EPS, means_map=means_map, scale=scale, wrap=wrap,
                                   capturable=capturable, grad_stats=grad_stats)
    saved = {"step": state["steps"], **products(kind, state["steps"]), "lr": kind.RATES, "betas": BETAS, "eps": EPS,
             "exp_avg": {g: dev(state["m"][g], dtype) for g in kind.GROUPS},
             "exp_avg_sq": {g: dev(state["v"][g], dtype) for g in kind.GROUPS}}
    if grad_stats and stats is not None:
        saved["grad_stats"] = dict({k: dev(stats[k], dtype) for k in STATS}, counts=stats["counts"])
    opt.load_state_dict(saved)
    return opt


def give_grads(opt, grads, dtype):
    for leaf, g in zip(opt.gaussians(), grads):
        if g is not None:
            leaf.grad = dev(g, dtype)


def read_opt(kind, opt, like):
    out = copy.deepcopy(like)
    for g, p in zip(kind.GROUPS, opt._params()):
        out["p"][g] = p.detach().cpu().double().numpy().reshape(like["p"][g].shape)
        out["m"][g] = opt.exp_avg[g].cpu().double().numpy().reshape(like["p"][g].shape)
        out["v"][g] = opt.exp_avg_sq[g].cpu().double().numpy().reshape(like["p"][g].shape)
    out["steps"] = opt.steps
    return out


def tensors_of(kind, state, gaussians, stats):
    out = {f"{k}[{g}]": state[k][g] for k in ("p", "m", "v") for g in kind.GROUPS}
    out.update(zip(("next means", "next covariances", "next conics"), gaussians))
    out.update({k: stats[k] for k in STATS})
    return out


def next_gaussians(opt):
    g = opt.gaussians()
    return [t.detach().cpu().double().numpy() for t in (g.means, g.covariances, g.conics)]


def one_step(kind, optim, family, state, stats, grads, dtype, map_name="tanh"):
    """ONE step on the GPU from (state, stats); everything it wrote held to its bar; returns (opt, got, got_stats)"""
    means_map, scale, wrap = MAPS[map_name]
    state, stats = kind.as_dtype(state, NP[dtype]), stats_as_dtype(stats, NP[dtype])
    grads = tuple(None if g is None else g.astype(NP[dtype]).astype(np.float64) for g in grads)
    want, want_g = kind.checker_step(state, grads, lr=kind.RATES, means_map=means_map, scale=scale, wrap=wrap)
    want_s = stats_step(state["p"], stats, grads, means_map, scale, chain=kind.chain)
    opt = make_opt(kind, optim, state, stats, dtype, map_name)
    give_grads(opt, grads, dtype)
    opt.step()
    got, got_s, got_g = read_opt(kind, opt, state), read_grad_stats(opt), next_gaussians(opt)
    assert got["steps"] == want["steps"], (family, got["steps"], want["steps"])
    assert opt.grad_counts == want_s["counts"], (family, opt.grad_counts, want_s["counts"])
    worst = 0.0
    if dtype == torch.float64:
        have = tensors_of(kind, got, got_g, got_s)
        for name, w in tensors_of(kind, want, want_g, want_s).items():
            fig = float(np.abs(have[name] - w).max()) / (1e-11 * scale_of(w))
            worst = max(worst, fig)
            assert fig <= 1.0, f"{family} {name}: {fig:.3g} x the float64 bar"
    else:
        params, adam = kind.torch_state(state, torch.float32, "cuda")
        ts = torch_stats(stats, torch.float32, "cuda")
        kind.torch_step(params, adam, grads, means_map, scale, wrap)
        reference_lines(ts, params["means"], params["scaling"])
        ref = kind.read_torch(params, adam, state)
        pairs = [(f"{k}[{g}]", got[k][g], want[k][g], ref[k][g]) for k in ("p", "m", "v") for g in kind.GROUPS]
        pairs += [(k, got_s[k], want_s[k], ts[k].cpu().double().numpy()) for k in STATS]
        # the next Gaussians: against the float64 forward of the kernel's OWN updated parameters, torch's float32
        # forward of those same parameters as the yardstick
        own = kind.forward(got["p"], means_map, scale)
        tp = {g: dev(got["p"][g], torch.float32) for g in kind.GROUPS}
        for name, g, w, t in zip(("next means", "next covariances", "next conics"), got_g, own,
                                 kind.torch_forward(tp, means_map, scale)):
            pairs.append((name, g, w, t.cpu().double().numpy()))
        for name, g, w, r in pairs:
            bar = 4.0 * rms(r - w) + 2.0 * ULP32 * rms(w)
            fig = rms(g - w) / max(bar, 1e-300)
            worst = max(worst, fig)
            assert fig <= 1.0, f"{family} {name}: {fig:.3g} x the float32 bar"
    print(f"[figure] {kind.name} {family} {str(dtype)[6:]} {map_name}: worst {worst:.3g} x its bar")
    return opt, got, got_s


def check_sizes(kind, optim, N):
    state, stats = kind.make_state(N, 2, seed=N, moments=True, steps=3), make_stats(N, seed=N, d=kind.d)
    one_step(kind, optim, "sizes", state, stats, kind.make_grads(N, 2, seed=N), torch.float32)


def check_channels_dtypes_maps(kind, optim, c, dtype, map_name):
    N = 1025
    state, stats = kind.make_state(N, c, seed=20 + c, moments=True, steps=3), make_stats(N, seed=20 + c, d=kind.d)
    grads = kind.make_grads(N, c, seed=30 + c, present=(True, True, c % 2 == 0, True))
    one_step(kind, optim, "channels x dtypes x maps", state, stats, grads, dtype, map_name)


def group_presence(kind, present):
    on = {"means": present[0], "values": present[1], "scaling": present[2] or present[3]}
    on["transform"] = on["scaling"]
    return {g: on[g] for g in kind.GROUPS}


def check_presence(kind, optim, present, dtype):
    """an absent group keeps parameters, moments, count and its three statistic arrays bit for bit"""
    N, c = 257, 2
    state, stats = kind.make_state(N, c, seed=45, moments=True, steps=kind.steps), make_stats(N, seed=45, d=kind.d)
    grads = kind.make_grads(N, c, seed=46, present=present)
    _, got, got_s = one_step(kind, optim, "presence patterns", state, stats, grads, dtype)
    start, start_s = kind.as_dtype(state, NP[dtype]), stats_as_dtype(stats, NP[dtype])
    on = group_presence(kind, present)
    for g in kind.GROUPS:
        assert got["steps"][g] == kind.steps[g] + int(on[g])
        if not on[g]:
            assert all(np.array_equal(got[k][g], start[k][g]) for k in ("p", "m", "v")), g
    for g, names in STAT_GROUPS.items():
        if not on[g]:
            assert all(np.array_equal(got_s[k], start_s[k]) for k in names), g


def check_planted(kind, optim, state, stats, grads, dtype, rows=16):
    state, stats = kind.as_dtype(state, NP[dtype]), stats_as_dtype(stats, NP[dtype])
    grads = tuple(g.astype(NP[dtype]).astype(np.float64) for g in grads)
    want, want_g = kind.checker_step(state, grads, lr=kind.RATES, means_map="tanh", scale=2.5)
    want_s = stats_step(state["p"], stats, grads, "tanh", 2.5, chain=kind.chain)
    opt = make_opt(kind, optim, state, stats, dtype)
    give_grads(opt, grads, dtype)
    opt.step()
    have = tensors_of(kind, read_opt(kind, opt, state), next_gaussians(opt), read_grad_stats(opt))
    assert all(np.isfinite(a).all() for a in have.values())
    worst = 0.0
    for name, w in tensors_of(kind, want, want_g, want_s).items():
        w2 = w.reshape(len(w), -1)
        err = np.abs(have[name].reshape(w2.shape) - w2)
        if dtype == torch.float64:
            fig = float(err.max()) / (1e-11 * scale_of(w))
        else:
            ratio = err.max(-1) / np.maximum(np.abs(w2).max(-1), 1e-30)           # per row, relative to the row
            fig = float(ratio[:rows].max()) / max(4.0 * float(ratio[rows:].max()), 1e-300)
        worst = max(worst, fig)
        assert fig <= 1.0, f"planted rows, {name}: {fig:.3g} x the bar"
    print(f"[figure] {kind.name} planted rows {str(dtype)[6:]}: worst {worst:.3g} x its bar")


def assert_bitwise(a, b, stats=True):
    for x, y in zip(a._params(), b._params()):
        assert torch.equal(x, y)
    for g in a.GROUPS:
        assert torch.equal(a.exp_avg[g], b.exp_avg[g]) and torch.equal(a.exp_avg_sq[g], b.exp_avg_sq[g]), g
    for x, y in zip(a.gaussians(), b.gaussians()):
        assert torch.equal(x, y)
    if stats:
        for k, x, y in zip(STATS, a.grad_stats, b.grad_stats):
            assert torch.equal(x, y), k
        assert a.grad_counts == b.grad_counts


def check_on_off(kind, optim, dtype, map_name, present):
    """parameters, moments and the next Gaussians bit for bit with statistics on and off"""
    N, c = 1025, 3
    state, stats = kind.make_state(N, c, seed=60, moments=True, steps=2), make_stats(N, seed=60, d=kind.d)
    on = make_opt(kind, optim, state, stats, dtype, map_name)
    off = make_opt(kind, optim, state, None, dtype, map_name, grad_stats=False)
    for k in range(2):
        grads = kind.make_grads(N, c, seed=61 + k, present=present)
        for opt in (on, off):
            give_grads(opt, grads, dtype)
            opt.step()
    assert_bitwise(on, off, stats=False)
    for read in (lambda: off.grad_stats, lambda: off.grad_counts, off.reset_grad_stats):
        with pytest.raises(RuntimeError, match="grad_stats=True"):
            read()


def check_calls(kind, optim, hip_lib, monkeypatch, dtype, capturable):
    """a statistics step is exactly one call of the new entry and none of pigs_optim_step; the next gaussians() launches
    nothing and is a second materialisation bit for bit"""
    N, c = 1025, 3
    names = sorted({kind.step_entry, "pigs_optim_step", kind.materialize_entry})
    calls = {name: 0 for name in names}

    def counting(name):
        fn = getattr(hip_lib, name)

        def wrapper(*args):
            calls[name] += 1
            return fn(*args)
        return wrapper
    for name in names:
        monkeypatch.setattr(hip_lib, name, counting(name))
    state, stats = kind.make_state(N, c, seed=50, moments=True, steps=2), make_stats(N, seed=50, d=kind.d)
    opt = make_opt(kind, optim, state, stats, dtype, "tanh", capturable=capturable)
    first = opt.gaussians()
    assert calls[kind.materialize_entry] == 1 and calls[kind.step_entry] == 0
    give_grads(opt, kind.make_grads(N, c, seed=51, present=(True, True, True, True)), dtype)
    versions = [t._version for t in opt.grad_stats]
    opt.step()
    assert calls[kind.step_entry] == 1 and calls["pigs_optim_step"] == 0 and calls[kind.materialize_entry] == 1
    assert all(t._version > v for t, v in zip(opt.grad_stats, versions))
    after = opt.gaussians()
    assert calls[kind.step_entry] == 1 and calls[kind.materialize_entry] == 1 and after is not first
    kept = [t.detach().clone() for t in (after.means, after.covariances, after.conics)]
    opt._next = opt._leaves = None
    again = opt.gaussians()
    assert calls[kind.materialize_entry] == 2
    for a, b in zip(kept, (again.means, again.covariances, again.conics)):
        assert torch.equal(a, b)


def check_host_and_device_counts(kind, optim, dtype):
    """ten steps in both modes from one state; the values sit out every third step, the means every fourth, the scaling
    every fifth: per-group counts differ, and every bit agrees, statistics included"""
    N, c = 257, 2
    state = kind.make_state(N, c, seed=56, moments=True, steps={g: k for k, g in enumerate(kind.GROUPS)})
    stats = make_stats(N, seed=56, d=kind.d)
    grads = [kind.make_grads(N, c, seed=57 + k, present=(k % 4 != 3, k % 3 != 2, k % 2 == 0 and k % 5 != 4, k % 5 != 4))
             for k in range(10)]
    host, device = make_opt(kind, optim, state, stats, dtype, "wrap"), make_opt(kind, optim, state, stats, dtype, "wrap", capturable=True)
    for k in range(10):
        for opt in (host, device):
            give_grads(opt, grads[k], dtype)
            opt.step()
    assert host.steps == device.steps and host.steps["means"] == 8 and host.steps["values"] == 1 + 7
    assert host.grad_counts == device.grad_counts == {"means": 3 + 8, "scaling": 3 + 8}
    assert_bitwise(host, device)


def check_capture_alone(kind, optim):
    """torch.cuda.graph around step() with static gradients, five replays against five eager steps: bitwise, counts 5"""
    N, c, dtype = 257, 2, torch.float32
    state, stats = kind.make_state(N, c, seed=70, moments=True, steps=0), make_stats(N, seed=70, d=kind.d, counts=0)
    grads = [kind.make_grads(N, c, seed=71 + k, present=(True, True, False, True)) for k in range(5)]
    eager = make_opt(kind, optim, state, stats, dtype)
    for k in range(5):
        give_grads(eager, grads[k], dtype)
        eager.step()
    opt = make_opt(kind, optim, state, stats, dtype, capturable=True)
    static = [dev(np.zeros_like(g), dtype) if g is not None else None for g in grads[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaves = opt.gaussians()
        for leaf, g in zip(leaves, static):
            leaf.grad = g
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    assert opt.grad_counts == {"means": 0, "scaling": 0}            # a capture runs nothing
    for k in range(5):
        for s, g in zip(static, grads[k]):
            if s is not None:
                s.copy_(dev(g, dtype))
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps == {g: 5 for g in kind.GROUPS} and opt.grad_counts == {"means": 5, "scaling": 5}
    assert_bitwise(eager, opt)


def check_reset_and_round_trip(kind, optim):
    """reset_grad_stats zeroes in place; state_dict carries the statistics across modes; a dict without them zeroes"""
    N, c, dtype = 129, 2, torch.float64
    state, stats = kind.make_state(N, c, seed=54, moments=True, steps=7), make_stats(N, seed=54, d=kind.d)
    grads = kind.make_grads(N, c, seed=55)
    a = make_opt(kind, optim, state, stats, dtype)
    give_grads(a, grads, dtype)
    a.step()
    saved = a.state_dict()
    assert saved["grad_stats"]["counts"] == {"means": 4, "scaling": 4} and set(saved["grad_stats"]) == set(STATS) | {"counts"}
    b = getattr(optim, kind.cls)(*[p.clone() for p in a._params()], lr=1.0, betas=BETAS, eps=EPS, means_map="tanh", scale=2.5,
                                 capturable=True, grad_stats=True)
    b.load_state_dict(saved)
    for o in (a, b):
        give_grads(o, grads, dtype)
        o.step()
    assert b.grad_counts == a.grad_counts == {"means": 5, "scaling": 5}
    assert_bitwise(a, b)
    for o in (a, b):
        buffers = o.grad_stats
        o.reset_grad_stats()
        assert all(t is u for t, u in zip(buffers, o.grad_stats)) and not any(bool(t.any()) for t in o.grad_stats)
        assert o.grad_counts == {"means": 0, "scaling": 0}
        give_grads(o, grads, dtype)
        o.step()                                                   # from zero sums: sum = last, norm = |last|
        s = o.grad_stats
        assert torch.equal(s.mean_grad, s.last_mean_grad) and torch.equal(s.scale_grad, s.last_scale_grad)
        assert torch.allclose(s.mean_grad_norm, torch.linalg.norm(s.last_mean_grad, dim=-1), rtol=1e-12, atol=0)
        assert o.grad_counts == {"means": 1, "scaling": 1}
    del saved["grad_stats"]
    b.load_state_dict(saved)
    assert not any(bool(t.any()) for t in b.grad_stats) and b.grad_counts == {"means": 0, "scaling": 0}


# ---- d = 2 --------------------------------------------------------------------------------------------------
PATTERNS = [(m, v, k, q) for k in (False, True) for m in (False, True) for v in (False, True) for q in (False, True)
            if m or v or k or q]
PATTERN_IDS = ["".join("mvcq"[i] if on else "-" for i, on in enumerate(p)) for p in PATTERNS]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_one_step_sizes(optim, N):
    check_sizes(KIND_2D, optim, N)


@pytest.mark.parametrize("map_name", ["tanh", "identity", "wrap"])
@DTYPES
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_one_step_channels_dtypes_maps(optim, c, dtype, map_name):
    check_channels_dtypes_maps(KIND_2D, optim, c, dtype, map_name)


@DTYPES
@pytest.mark.parametrize("present", PATTERNS, ids=PATTERN_IDS)
def test_presence_patterns(optim, present, dtype):
    check_presence(KIND_2D, optim, present, dtype)


@DTYPES
def test_planted_rows(optim, dtype):
    """|t| = 8, s0 / s1 = 1e4 both ways, every gradient of a row exactly 0, every gradient of a row 1e-30"""
    N, c = 257, 2
    state, grads = planted(N, c, 49, zero_state=False)
    check_planted(KIND_2D, optim, state, make_stats(N, seed=49), grads, dtype)


@pytest.mark.parametrize("present", [(True, True, True, True), (True, False, False, True), (False, True, True, False)],
                         ids=["mvcq", "m--q", "-vc-"])
@pytest.mark.parametrize("map_name", ["tanh", "wrap"])
@DTYPES
def test_statistics_change_no_bit_of_the_update(optim, dtype, map_name, present):
    check_on_off(KIND_2D, optim, dtype, map_name, present)


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@DTYPES
def test_abi_calls_and_the_next_gaussians(optim, hip_lib, monkeypatch, dtype, capturable):
    check_calls(KIND_2D, optim, hip_lib, monkeypatch, dtype, capturable)


@DTYPES
def test_host_and_device_counts_give_the_same_bits(optim, dtype):
    check_host_and_device_counts(KIND_2D, optim, dtype)


def test_capture_of_the_optimiser_alone(optim):
    check_capture_alone(KIND_2D, optim)


def test_reset_and_state_round_trip(optim):
    check_reset_and_round_trip(KIND_2D, optim)


def test_densification_recipe_of_integration_md(optim):
    """INTEGRATION.md section 4 as written: mean_grad_norm from opt.grad_stats over the count (test_no_mlp.py:190-205),
    threshold_mask, refine_index(mode="clone"), opt.refine; against the reference's lines in torch; afterwards the
    statistics are zeros of the new row count with counts 0 (:249-252)"""
    from pigs_amd import refine_index, threshold_mask
    N, c, dtype = 300, 2, torch.float64
    state = t2.make_state(N, c, seed=90)
    opt = make_opt(KIND_2D, optim, state, None, dtype)
    for k in range(3):
        give_grads(opt, t2.make_grads(N, c, seed=91 + k), dtype)
        opt.step()
    stats, counter = opt.grad_stats, opt.grad_counts["means"]
    assert counter == 3
    mean_grad_norm = stats.mean_grad_norm / counter
    keep_mask = (torch.norm(opt.values, dim=-1) > 0.01) & (torch.sum(torch.exp(opt.raw_scaling), dim=-1) < 0.5)   # :198-201
    assert 0 < int((~keep_mask).sum()) < N // 2
    split_indices = threshold_mask(mean_grad_norm, keep_mask, k=1.6)
    quantile = torch.mean(mean_grad_norm) + 1.6 * torch.std(mean_grad_norm)              # test_no_mlp.py:203-205
    assert torch.equal(split_indices, torch.logical_and(mean_grad_norm > quantile, keep_mask)) and int(split_indices.sum()) > 0
    old_means, old_m = opt.raw_means.detach().clone(), opt.exp_avg["means"].clone()
    source, child = refine_index(keep_mask, split_indices, mode="clone")
    opt.refine(source, child)
    rows = int(keep_mask.sum()) + int(split_indices.sum())
    assert torch.equal(opt.raw_means, torch.cat((old_means[keep_mask], old_means[split_indices])))
    assert torch.equal(opt.exp_avg["means"], torch.cat((old_m[keep_mask], torch.zeros_like(old_m[split_indices]))))
    new = opt.grad_stats
    assert new.mean_grad.shape == (rows, 2) and new.scale_grad_norm.shape == (rows,) and new.mean_grad.dtype == dtype
    assert not any(bool(t.any()) for t in new) and opt.grad_counts == {"means": 0, "scaling": 0}
    give_grads(opt, t2.make_grads(rows, c, seed=95), dtype)
    opt.step()
    assert opt.grad_counts == {"means": 1, "scaling": 1} and opt.gaussians().means.shape == (rows, 2)
    assert torch.equal(opt.grad_stats.mean_grad, opt.grad_stats.last_mean_grad)


def test_refine_with_shift_means(optim):
    """a row with child >= 0 gets raw_means[source] + shift_means[source]; the others and the default are untouched"""
    from pigs_amd import refine_index
    N, c, dtype = 200, 1, torch.float32
    state = t2.make_state(N, c, seed=96, moments=True, steps=2)
    keep, split = (dev(m, torch.bool) for m in random_masks(N, 0.15, 0.2, 96))
    split = split & keep
    source, child = refine_index(keep, split, mode="clone")
    shift = dev(np.random.default_rng(97).standard_normal((N, 2)), dtype)
    a, b = make_opt(KIND_2D, optim, state, None, dtype), make_opt(KIND_2D, optim, state, None, dtype)
    old = a.raw_means.detach().clone()
    a.refine(source, child, shift_means=shift)
    b.refine(source, child)
    assert torch.equal(a.raw_means, torch.cat((old[keep], old[split] + shift[split])))
    assert torch.equal(b.raw_means, torch.cat((old[keep], old[split])))
    assert torch.equal(a.values, b.values) and torch.equal(a.exp_avg_sq["means"], b.exp_avg_sq["means"])
    with pytest.raises(ValueError):
        a.refine(source, child, shift_means=shift)                # the old shape no longer fits


# ---- the recorded loop --------------------------------------------------------------------------------------
def hold_to_fixture(name, losses, got, what):
    f = np.load(os.path.join(GOLDEN, "grad_stats", name))
    rel = float((np.abs(losses - f["losses"]) / np.maximum(np.abs(f["losses"]), 1e-12)).max())
    worst = {k: float(np.abs(got[k] - f[k]).max()) / scale_of(f[k]) for k in STATS}
    k_worst = max(worst, key=worst.get)
    print(f"[figure] {what}: losses {rel:.3g} ({rel / 2e-3:.3g} x its bar), statistics worst {worst[k_worst]:.3g} of "
          f"{k_worst}'s scale ({worst[k_worst] / 2e-3:.3g} x its bar)")
    assert rel < 2e-3, (what, rel)
    for k in STATS:
        assert worst[k] < 2e-3, (what, k, worst[k])


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_recorded_loop_losses_and_statistics(optim, backend):
    """loop_2d through the HIP sampler with GaussianAdam(grad_stats=True) against tests/golden/grad_stats/no_mlp_2d.npz"""
    from diff_gaussian_sampling import GaussianSampler
    device, dtype = torch.device("cuda"), torch.float32
    params, g = init_2d(device, dtype)
    opt = optim.GaussianAdam(*params, lr=1e-2, means_map="tanh", scale=2.5, grad_stats=True)
    new_sampler = (lambda: GaussianSampler(False)) if backend == "dense" else (lambda: GaussianSampler(False, backend="binned"))
    losses = loop_2d(opt, g, new_sampler, device, dtype)
    assert opt.grad_counts == {"means": 30, "scaling": 30}
    hold_to_fixture("no_mlp_2d.npz", losses, read_grad_stats(opt), f"2-D loop, {backend}")
