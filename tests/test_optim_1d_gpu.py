"""GPU: GaussianAdam1D (pigs_amd/optim.py, csrc/optim.hip: optim1d_*) against the float64 checker of
tests/test_optim_1d.py, through the harness and at the bars of tests/test_optim_stats_gpu.py; statistics on throughout
(random NON-zero sums, counts 3), and bit for bit against statistics off.  Then the 1-D densification of
test_no_mlp_1d.py:192-262 as INTEGRATION.md section 4 writes it, the whole 1-D step in a GraphedStep, and the recorded
Burgers loop of tests/golden/grad_stats/no_mlp_1d.npz.
"""
import types

import numpy as np
import pytest
import torch

import test_optim_1d as t1
from test_optim_gpu import dev
from test_optim_stats import make_stats, read_grad_stats
from test_optim_stats_gpu import (DTYPES, PATTERN_IDS, PATTERNS, check_calls, check_capture_alone, check_channels_dtypes_maps,
                                  check_host_and_device_counts, check_on_off, check_planted, check_presence,
                                  check_reset_and_round_trip, check_sizes, give_grads, hold_to_fixture, make_opt)
from test_optim_stats_gpu import optim  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu


def _torch_forward_1d(tp, means_map, scale):
    covariances = torch.exp(tp["scaling"]).reshape(-1, 1)         # test_no_mlp_1d.py:109-111
    return (torch.tanh(tp["means"]) * scale if means_map == "tanh" else tp["means"]), covariances, 1.0 / covariances


KIND_1D = types.SimpleNamespace(
    name="d=1", cls="GaussianAdam1D", d=1, GROUPS=t1.GROUPS, RATES=t1.RATES, make_state=t1.make_state_1d,
    make_grads=t1.make_grads_1d, as_dtype=t1.as_dtype_1d, checker_step=t1.checker_step_1d, forward=t1.forward_1d,
    chain=t1.chain_rule_1d, torch_state=t1.torch_state_1d, torch_step=t1.torch_step_1d, read_torch=t1.read_torch_1d,
    torch_forward=_torch_forward_1d, step_entry="pigs_optim1d_step", plain_entry="pigs_optim1d_step",
    materialize_entry="pigs_optim1d_materialize", steps={"means": 3, "values": 5, "scaling": 2})


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_one_step_sizes(optim, N):
    check_sizes(KIND_1D, optim, N)


@pytest.mark.parametrize("map_name", ["tanh", "identity", "wrap"])
@DTYPES
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_one_step_channels_dtypes_maps(optim, c, dtype, map_name):
    check_channels_dtypes_maps(KIND_1D, optim, c, dtype, map_name)


@DTYPES
@pytest.mark.parametrize("present", PATTERNS, ids=PATTERN_IDS)
def test_presence_patterns(optim, present, dtype):
    check_presence(KIND_1D, optim, present, dtype)


def test_no_gradient_moves_nothing_and_launches_nothing(optim, hip_lib, monkeypatch):
    state, stats = t1.make_state_1d(65, 2, seed=5, moments=True, steps=2), make_stats(65, seed=5, d=1)
    opt = make_opt(KIND_1D, optim, state, stats, torch.float32)
    leaves, before = opt.gaussians(), [t.clone() for t in opt.grad_stats]
    monkeypatch.setattr(hip_lib, "pigs_optim1d_step", None)       # a call would raise
    opt.step()
    assert opt.gaussians() is leaves and opt.steps == {g: 2 for g in t1.GROUPS} and opt.grad_counts == {"means": 3, "scaling": 3}
    assert all(torch.equal(a, b) for a, b in zip(before, opt.grad_stats))


@DTYPES
def test_planted_rows(optim, dtype):
    """rows 0..15 planted among ordinary ones: s 1e4 times smaller / larger than its neighbours', raw_means at |x| = 8
    (sech^2 = 4.5e-7), every gradient of a row exactly 0, every gradient of a row 1e-30"""
    N, c = 257, 2
    state = t1.make_state_1d(N, c, seed=49, moments=True, steps=6)
    grads = list(t1.make_grads_1d(N, c, seed=50, present=(True, True, True, True)))
    state["p"]["means"][0:4, 0] = [8.0, -8.0, 8.0, -8.0]
    state["p"]["scaling"][2:8, 0] = [-1.0 - np.log(1e4), -1.0 + np.log(1e4), -2.0 - np.log(1e4), -2.0 + np.log(1e4),
                                     -np.log(1e4), np.log(1e4)]
    for g in grads:
        g[8:12] = 0.0
        g[12:16] = 1e-30
    check_planted(KIND_1D, optim, state, make_stats(N, seed=49, d=1), tuple(grads), dtype)


@pytest.mark.parametrize("present", [(True, True, True, True), (True, False, False, True), (False, True, True, False)],
                         ids=["mvcq", "m--q", "-vc-"])
@pytest.mark.parametrize("map_name", ["tanh", "wrap"])
@DTYPES
def test_statistics_change_no_bit_of_the_update(optim, dtype, map_name, present):
    check_on_off(KIND_1D, optim, dtype, map_name, present)


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@DTYPES
def test_abi_calls_and_the_next_gaussians(optim, hip_lib, monkeypatch, dtype, capturable):
    check_calls(KIND_1D, optim, hip_lib, monkeypatch, dtype, capturable)


@DTYPES
def test_host_and_device_counts_give_the_same_bits(optim, dtype):
    check_host_and_device_counts(KIND_1D, optim, dtype)


def test_capture_of_the_optimiser_alone(optim):
    check_capture_alone(KIND_1D, optim)


def test_reset_and_state_round_trip(optim):
    check_reset_and_round_trip(KIND_1D, optim)


def test_leaves_and_parameters(optim):
    """[N,1] leaves that require grad, values on the parameter's storage, nn.Parameters updated in place"""
    N = 25
    params = [torch.nn.Parameter(t) for t in t1.init_1d(torch.device("cuda"), torch.float32)[0]]
    opt = optim.GaussianAdam1D(*params, lr=1e-2, means_map="tanh", scale=2.5)
    g = opt.gaussians()
    assert [tuple(t.shape) for t in g] == [(N, 1)] * 4 and all(t.is_leaf and t.requires_grad for t in g)
    assert g.values.data_ptr() == params[1].data_ptr()
    assert torch.allclose(g.conics * g.covariances, torch.ones_like(g.conics)) and torch.allclose(g.covariances, torch.exp(params[2]))
    versions = [p._version for p in params]
    give_grads(opt, t1.make_grads_1d(N, 1, seed=1, present=(True, True, False, True)), torch.float32)
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions)) and opt.raw_means is params[0]
    assert opt.steps == {"means": 1, "values": 1, "scaling": 1}


# ---- the 1-D densification ----------------------------------------------------------------------------------
def test_densification_recipe_of_integration_md(optim):
    """INTEGRATION.md section 4's 1-D recipe as written against test_no_mlp_1d.py:194-262 in torch: mean_grad and
    mean_grad_norm over the count, the keep mask, threshold_mask, refine_index(mode="clone"),
    opt.refine(source, child, shift_means=mean_grad); the statistics restart as zeros"""
    from pigs_amd import refine_index, threshold_mask
    N, c, dtype = 120, 1, torch.float64
    state = t1.make_state_1d(N, c, seed=90)
    state["p"]["values"][::7] = 1e-3                              # some rows the keep mask drops (:205)
    opt = make_opt(KIND_1D, optim, state, None, dtype)
    for k in range(3):
        give_grads(opt, t1.make_grads_1d(N, c, seed=91 + k), dtype)
        opt.step()
    raw_means, values, scaling = opt.raw_means, opt.values, opt.raw_scaling
    counter = opt.grad_counts["means"]
    mean_grad = opt.grad_stats.mean_grad / counter                # :194-195
    mean_grad_norm = opt.grad_stats.mean_grad_norm / counter
    keep_mask = torch.logical_and(                                # :204-213
        torch.norm(values, dim=-1) > 0.01,
        torch.logical_and(torch.sum(torch.abs(raw_means), dim=-1) < 10.0,
                          torch.logical_and(torch.sum(scaling, dim=-1) < 0.0, torch.sum(scaling, dim=-1) > -5.0)))
    split_indices = threshold_mask(mean_grad_norm, keep_mask, k=1.6)
    quantile = torch.mean(mean_grad_norm) + 1.6 * torch.std(mean_grad_norm)                # :216-217
    assert torch.equal(split_indices, torch.logical_and(mean_grad_norm > quantile, keep_mask))
    assert int(split_indices.sum()) > 0 and int((~keep_mask).sum()) > 0
    old = [t.detach().clone() for t in (raw_means, values, scaling)]
    old_m = [opt.exp_avg[g].clone() for g in t1.GROUPS]
    source, child = refine_index(keep_mask, split_indices, mode="clone")
    new = opt.refine(source, child, shift_means=mean_grad)
    split_dir = mean_grad[split_indices]                          # :219-225
    extensions = (old[0][split_indices] + split_dir, old[1][split_indices], old[2][split_indices])
    for p, o, e, m, g in zip(new, old, extensions, old_m, t1.GROUPS):
        assert torch.equal(p, torch.cat((o[keep_mask], e), dim=0)), g
        assert torch.equal(opt.exp_avg[g], torch.cat((m[keep_mask], torch.zeros_like(e)), dim=0)), g
    rows = int(keep_mask.sum()) + int(split_indices.sum())
    s = opt.grad_stats                                            # :259-262
    assert s.mean_grad.shape == (rows, 1) and s.mean_grad_norm.shape == (rows,) and not any(bool(t.any()) for t in s)
    assert opt.grad_counts == {"means": 0, "scaling": 0}
    give_grads(opt, t1.make_grads_1d(rows, c, seed=95), dtype)
    opt.step()
    assert opt.gaussians().means.shape == (rows, 1) and opt.grad_counts == {"means": 1, "scaling": 1}


# ---- the whole step in a graph; the recorded loop -----------------------------------------------------------
def test_capture_of_the_whole_1d_step(optim):
    """GraphedStep over preprocess -> the three plain sample_* calls -> the Burgers residual against a fixed previous
    level -> backward -> opt.step(): dense sampler, d = 1, N = 25, 128 points; ten replays against ten eager steps at the
    bar of tests/test_optim_gpu.py::test_capture_of_the_whole_step, 2e-3; the statistics counted on the device"""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    warmup, replays = 3, 10
    nu, dt = 1.0 / (100.0 * np.pi), 0.05
    g = torch.Generator(device="cpu").manual_seed(3)
    samples = ((torch.rand((128, 1), generator=g) * 2 - 1) * 2.5)
    prev_img = torch.exp(-2.0 * samples ** 2)

    def build(capturable):
        params, _ = t1.init_1d(torch.device("cuda"), torch.float32)
        opt = optim.GaussianAdam1D(*params, lr=1e-2, means_map="tanh", scale=2.5, capturable=capturable, grad_stats=True)
        return opt, GaussianSampler(False), samples.cuda(), prev_img.cuda()

    def step_of(opt, sampler):
        def fn(samples, prev_img):
            gs = opt.gaussians()
            sampler.preprocess(gs.means, gs.values, gs.covariances, gs.conics, samples)
            img = sampler.sample_gaussians()
            ux = sampler.sample_gaussians_derivative()
            uxx = sampler.sample_gaussians_laplacian()
            ut = (img - prev_img) / dt
            loss = torch.mean((ut[:, 0] - (nu * uxx[:, 0, 0, 0] - img[:, 0] * ux[:, 0, 0])) ** 2)
            loss.backward()
            opt.step()
            return loss.detach()
        return fn

    opt_e, sampler_e, s, p = build(False)
    fn = step_of(opt_e, sampler_e)
    eager = np.array([float(fn(s, p)) for _ in range(warmup + replays)])
    holder = {}

    def make_inputs():
        holder["opt"], holder["sampler"], s, p = build(True)
        holder["fn"] = step_of(holder["opt"], holder["sampler"])
        return s, p
    step = GraphedStep(lambda s, p: holder["fn"](s, p), make_inputs, warmup=warmup)
    graphed = np.array([float(step()) for _ in range(replays)])
    assert holder["opt"].steps == {grp: warmup + replays for grp in t1.GROUPS}
    assert holder["opt"].grad_counts == {"means": warmup + replays, "scaling": warmup + replays}
    rel = np.abs(graphed - eager[warmup:]) / np.abs(eager[warmup:])
    got, want = read_grad_stats(holder["opt"]), read_grad_stats(opt_e)
    worst = max(float(np.abs(got[k] - want[k]).max()) / max(float(np.abs(want[k]).max()), 1e-300) for k in got)
    print(f"[figure] whole 1-D step capture: worst loss difference {rel.max():.3g} ({rel.max() / 2e-3:.3g} x its bar), "
          f"statistics {worst:.3g} ({worst / 2e-3:.3g} x its bar)")
    assert eager[-1] < eager[0] and np.isfinite(graphed).all()
    assert rel.max() < 2e-3 and worst < 2e-3, (rel.max(), worst, graphed, eager)


def test_recorded_loop_losses_and_statistics(optim):
    """loop_1d through the HIP sampler (dense, d = 1) with GaussianAdam1D(grad_stats=True) against
    tests/golden/grad_stats/no_mlp_1d.npz"""
    from diff_gaussian_sampling import GaussianSampler
    device, dtype = torch.device("cuda"), torch.float32
    params, g = t1.init_1d(device, dtype)
    opt = optim.GaussianAdam1D(*params, lr=1e-2, means_map="tanh", scale=2.5, grad_stats=True)
    losses = t1.loop_1d(opt, g, lambda: GaussianSampler(False), device, dtype)
    assert opt.grad_counts == {"means": 30, "scaling": 30}
    hold_to_fixture("no_mlp_1d.npz", losses, read_grad_stats(opt), "1-D loop, dense")
