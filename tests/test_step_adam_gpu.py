"""GPU: the model's time step WITH its update -- NetworkAdam on the network's parameters behind the HIP step of
tests/test_step_gpu.py, eager and with the whole of it (forward, loss, backward, update, loss-weighted rate) in ONE
GraphedStep.

The bar is test_step_gpu.py::test_five_adam_steps's: both loss curves against the float64 curve (tests/test_step.py's
oracle under torch.optim.Adam on the CPU),  err_hip <= 4 err_torch32 + 1e-6 x the curve's scale,  err_torch32 that of the
float32 torch step under torch.optim.Adam on the GPU.  With ``decay`` the oracle loops carry the recurrence of
main_pn.py:217-225 on the host: the step's rate is lr x rate_scale, then rate_scale *= exp(-decay x loss).
The sampler's backward uses float atomics, so nothing is claimed bitwise here.
"""
import math

import numpy as np
import pytest
import torch

import test_step as ts
from test_step import Network, OracleOps, run_scene, scene_tensors
from test_step_gpu import HipOps, fused_network, reference

pytestmark = pytest.mark.gpu

LR = 1e-3


def torch_curve(scene, ops, net, dtype, device, steps, decay=None):
    """ts.adam_curve, with the loss-weighted rate of main_pn.py:217-225 kept on the host when ``decay`` is given"""
    opt = torch.optim.Adam([p for _, p in net.named_parameters()], lr=LR)
    losses, rate_scale = [], 1.0
    for _ in range(steps):
        rec = run_scene(scene, ops, net, dtype, device, state_grad=False)
        for name, p in net.named_parameters():
            p.grad = rec["grad/" + name].clone()
        opt.param_groups[0]["lr"] = LR * rate_scale
        opt.step()
        losses.append(float(rec["loss"]))
        if decay is not None:
            rate_scale *= math.exp(-decay * losses[-1])
    return np.array(losses)


def held(what, got, single, want):
    err_h, err_t, scale = np.abs(got - want).max(), np.abs(single - want).max(), ts.scale_of(want)
    ratio = err_h / (4.0 * err_t + 1e-6 * scale)
    print(f"[figure] {what}: hip {err_h:.3g}, torch32 {err_t:.3g} off the float64 curve of scale {scale:.3g}: ratio {ratio:.3f}")
    assert err_h <= 4.0 * err_t + 1e-6 * scale
    return ratio


def test_five_network_adam_steps(hip_lib):
    """ts.adam_curve with NetworkAdam in place of torch.optim.Adam, on the HIP step of the navier_stokes scene"""
    import pigs_amd
    scene = reference("navier_stokes")[0]
    want = ts.adam_curve(scene, OracleOps(), Network(scene.sd), torch.float64, "cpu")
    single = ts.adam_curve(scene, OracleOps(), Network(scene.sd, torch.float32, "cuda"), torch.float32, "cuda")
    net, ops = fused_network(scene.sd), HipOps(hip_lib)
    opt = pigs_amd.NetworkAdam([p for _, p in net.named_parameters()], lr=LR)
    got = []
    for _ in range(5):
        rec = run_scene(scene, ops, net, torch.float32, "cuda", state_grad=False)
        for name, p in net.named_parameters():
            p.grad = rec["grad/" + name].clone()
        opt.step()
        got.append(float(rec["loss"]))
    assert opt.steps == [5] * len(opt.steps) and all(p.grad is None for _, p in net.named_parameters())
    assert want[-1] < want[0] and got[-1] < got[0]
    held("five NetworkAdam steps", np.array(got), single, want)


def test_the_whole_step_and_its_update_in_one_graphed_step(hip_lib):
    """forward, loss, backward and opt.step(loss=loss, decay=1.0) with capturable=True in ONE GraphedStep (scene capture0:
    N = 257, the lists are built without a read-back).  The warm-up runs are steps of the same recurrence; the five
    replays that follow are held against steps 3..7 of the float64 curve, and loss_stats() holds their sum, maximum and
    count"""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    warmup, replays, decay = 2, 5, 1.0
    scene = reference("capture0")[0]
    want = torch_curve(scene, OracleOps(), Network(scene.sd), torch.float64, "cpu", warmup + replays, decay)
    single = torch_curve(scene, OracleOps(), Network(scene.sd, torch.float32, "cuda"), torch.float32, "cuda",
                         warmup + replays, decay)
    net = fused_network(scene.sd)
    named = net.named_parameters()
    holder = {}

    def make_inputs():
        holder["ops"] = HipOps(hip_lib)
        holder["opt"] = pigs_amd.NetworkAdam([p for _, p in named], lr=LR, capturable=True)
        x = holder["x"] = scene_tensors(scene, torch.float32, "cuda", state_grad=False)
        return x.t_params + x.state

    def fn(*leaves):
        rec = run_scene(scene, holder["ops"], net, tensors=holder["x"])
        for name, p in named:
            p.grad = rec["grad/" + name]
        holder["opt"].step(loss=rec["loss"], decay=decay)
        return rec["loss"]
    step = GraphedStep(fn, make_inputs, warmup=warmup)
    opt = holder["opt"]
    assert opt.steps == [warmup] * len(named) and opt.loss_stats()[2] == warmup
    opt.reset_loss_stats()
    got = []
    for _ in range(replays):
        got.append(float(step()))
    got = np.array(got)
    torch.cuda.synchronize()
    assert opt.steps == [warmup + replays] * len(named) and np.isfinite(got).all()
    held("graphed step with its update", got, single[warmup:], want[warmup:])
    total, worst, count = opt.loss_stats()
    assert count == replays
    assert abs(total - got.sum()) <= 1e-6 * got.sum() and abs(worst - got.max()) <= 1e-6 * got.max(), (total, worst, got)
    # the rate the next step would run at: the recurrence over all seven losses, the warm-up's included
    print(f"[figure] rate_scale after {warmup + replays} steps: {float(opt.rate_scale):.6g}")
    assert 0.0 < float(opt.rate_scale) < 1.0
