"""GPU: the model's whole time step with delta_net reading (features, heads) through FusedMLP.joined -- no cat -- and the
head magnitudes of magnitude_loss (model_pn.py:892-901) from the same launch, held to the
float64 step oracle of tests/test_step.py with the bar and the allowance of tests/test_step_gpu.py:

    err_hip <= 4 err_torch32 + floor x scale.

``JoinedOps`` is test_step_gpu.HipOps with the query / key nets in one FusedMLPBank (tests/test_step_bank_gpu.py) and

    deltas, mags = delta_net.joined((features, nf), block_means=(0, H))

in the place of the cat and the net's call.  ``magnitudes`` [H] and ``magnitude_loss = mean((magnitudes - 1)^2)`` are held
to a float64 statement on the oracle's ``local_global_features`` (the mean square of each head's 16 columns), with the
upstream floor 1e-6; err_torch32 is that of the same statement in float32 torch ops on the float32 composition's tensor.
Every case prints its worst ratio.
"""
import numpy as np
import pytest
import torch

import test_step as ts
from test_step import Network, OracleOps, allowance, errors, run_scene, scene_tensors
from test_step_gpu import BITWISE, HipOps, fused_network, hold, reference

pytestmark = pytest.mark.gpu


def magnitudes_of(joined, exchanged=False):
    """the statement: the mean square of each head's LATENT columns of local_global_features [N, (1 + H) LATENT], in the
    tensor's own dtype.  ``exchanged``: the planted mistake, the head blocks taken in the wrong order."""
    L = ts.LATENT
    heads = range(ts.HEADS)[::-1] if exchanged else range(ts.HEADS)
    return torch.stack([joined[:, L * (1 + h):L * (2 + h)].pow(2).mean() for h in heads])


def magnitude_loss_of(magnitudes):
    return ((magnitudes - 1.0) ** 2).mean()


class JoinedOps(HipOps):
    def step(self, net, t_params, means, u, scaling, transforms, mask, wrap, k, covs=None):
        from pigs_amd import FusedMLPBank, advance_gaussians
        from pigs_amd.covariances import build_covariances
        smp = self.sampler
        with torch.no_grad():
            if covs is None:
                covs = build_covariances(scaling, transforms)
            smp.preprocess(means, u, covs[0], covs[1], means)
        features = net.seq["input_projection"](t_params[None])                        # [1, N, L]
        smp.preprocess_aggregate()
        rows = features[0]
        qk = FusedMLPBank([net.query(0), net.query(1), net.key(0), net.key(1)], groups=2)(features)      # [2, N, H, K]
        nf = smp.aggregate_neighbors_heads(rows, net.transform, qk[0], qk[1], net.frequencies, net.distance_transform)
        deltas, mags = net.seq["delta_net"].joined((features, nf), block_means=(0, ts.HEADS))      # [1, N, 5 + c], [H]
        new = advance_gaussians(means, u, scaling, transforms, deltas, mask[:, None], wrap=wrap)
        with torch.no_grad():                     # for the record alone: the step itself forms no cat
            joined = torch.cat((rows, nf.reshape(nf.shape[0], -1)), dim=-1)
        rec = {"global_features": rows, "neighbor_features": nf.permute(1, 0, 2), "local_global_features": joined,
               "deltas": deltas[0], "magnitudes": mags, "magnitude_loss": magnitude_loss_of(mags)}
        rec.update(new._asdict())
        return rec


def with_magnitudes(rec):
    """a float64 or float32 torch run's results, with the statement's magnitudes of its own local_global_features"""
    mags = magnitudes_of(rec["s0/local_global_features"])
    return {**rec, "s0/magnitudes": mags, "s0/magnitude_loss": magnitude_loss_of(mags)}


MAGNITUDES = ("s0/magnitudes", "s0/magnitude_loss")
_joined = {}


def joined_run(hip_lib, name):
    if name not in _joined:
        scene = reference(name)[0]
        _joined[name] = run_scene(scene, JoinedOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    return _joined[name]


@pytest.mark.parametrize("name", ts.FIXTURES)
def test_one_recorded_step_through_the_joined_net(hip_lib, name):
    """the recorded state, t_params and weights of the reference's own step: every intermediate and every gradient, and
    the magnitudes against the float64 statement"""
    scene, want, single = reference(name)
    got = joined_run(hip_lib, name)
    hold(f"{name}, delta_net on (features, heads) without the cat", got, single, want)
    hold(f"{name}, magnitudes and magnitude_loss", got, with_magnitudes(single), with_magnitudes(want), keys=MAGNITUDES)
    assert got["s0/magnitudes"].shape == (ts.HEADS,) and float(got["s0/magnitude_loss"]) > 0


@pytest.mark.parametrize("name", ts.FIXTURES)
def test_exchanged_head_blocks_move_the_magnitudes_past_the_allowance(name):
    """the bar discriminates: the statement with the two head blocks exchanged is off the statement by many allowances"""
    scene, want, single = reference(name)
    right, wrong = magnitudes_of(want["s0/local_global_features"]), magnitudes_of(want["s0/local_global_features"], True)
    e_t = errors(with_magnitudes(single), with_magnitudes(want))["s0/magnitudes"]
    factor = float((wrong - right).abs().max()) / allowance("s0/magnitudes", *e_t)
    print(f"[figure] {name}: exchanged head blocks move the magnitudes by {factor:.3g} x the allowance")
    assert factor > 100.0


def magnitude_step(scene, ops, net, dtype, device):
    """one step, and ONE backward of the step's weighted penalties + magnitude_loss to every parameter, t_params and the
    state.  ``ops`` gives the magnitudes (JoinedOps) or the statement is applied to its local_global_features."""
    x = scene_tensors(scene, dtype, device)
    s = ops.step(net, x.t_params[0], *x.state, x.mask, scene.wrap, 0)
    mags = s["magnitudes"] if "magnitudes" in s else magnitudes_of(s["local_global_features"])
    magnitude_loss = magnitude_loss_of(mags)
    loss = (s["penalty"] * x.weights).sum() + magnitude_loss
    leaves = list(net.named_parameters()) + [("t_params0", x.t_params[0])] + list(zip(ts.STATE, x.state))
    grads = torch.autograd.grad(loss, [t for _, t in leaves], allow_unused=True)
    rec = {"s0/magnitudes": mags, "s0/magnitude_loss": magnitude_loss, "loss": loss}
    rec.update({"grad/" + n: torch.zeros_like(t) if g is None else g for (n, t), g in zip(leaves, grads)})
    return {k: v.detach() for k, v in rec.items()}


@pytest.mark.parametrize("name", ts.FIXTURES)
def test_one_backward_of_the_step_loss_and_magnitude_loss(hip_lib, name):
    """magnitude_loss's gradient enters the heads through the joined backward's own store and meets the penalties' there:
    every parameter's gradient (the query / key nets' and the aggregation's come through the heads alone) under the bar"""
    scene = reference(name)[0]
    want = magnitude_step(scene, OracleOps(), Network(scene.sd), torch.float64, "cpu")
    single = magnitude_step(scene, OracleOps(), Network(scene.sd, torch.float32, "cuda"), torch.float32, "cuda")
    got = magnitude_step(scene, JoinedOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    assert float(want["grad/query_transform.0.0.weight"].abs().max()) > 0
    hold(f"{name}, one backward of penalties + magnitude_loss", got, single, want)
    again = magnitude_step(scene, JoinedOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    for k in ("s0/magnitudes", "s0/magnitude_loss", "grad/delta_net.0.weight", "grad/delta_net.10.bias"):
        assert torch.equal(got[k], again[k]), f"{name} {k} differs between two runs on the same inputs"


def test_the_whole_step_through_the_joined_net_in_one_graphed_step(hip_lib):
    """as test_step_gpu.test_the_whole_step_in_one_graphed_step: three replays rewrite t_params, the state, the sample
    points and two weight tensors in place; each is held to the oracle under the bar, the magnitudes included"""
    from pigs_amd.graphs import GraphedStep
    scenes = [reference(f"capture{k}")[0] for k in range(4)]
    net = fused_network(scenes[0].sd)
    params = dict(net.named_parameters())
    holder = {}

    def make_inputs():
        holder["ops"] = JoinedOps(hip_lib)
        x = holder["x"] = scene_tensors(scenes[0], torch.float32, "cuda")
        return x.t_params + x.state

    def fn(*leaves):
        rec = run_scene(scenes[0], holder["ops"], net, tensors=holder["x"])
        holder["names"] = list(rec)
        return tuple(rec.values())
    step = GraphedStep(fn, make_inputs, warmup=2)
    for k in (1, 2, 3):
        scene, want, single = reference(f"capture{k}")
        with torch.no_grad():
            for leaf, a in zip(step.inputs, scene.t_params + [scene.state[n] for n in ts.STATE]):
                leaf.copy_(torch.as_tensor(a, dtype=torch.float32))
            holder["x"].samples.copy_(torch.as_tensor(scene.samples, dtype=torch.float32))
            for name in ("delta_net.10.weight", "transform"):
                params[name].copy_(torch.as_tensor(scene.sd[name], dtype=torch.float32))
        got = dict(zip(holder["names"], [t.clone() for t in step()]))
        torch.cuda.synchronize()
        hold(f"graphed step through the joined net, replay {k}", got, single, want)
        hold(f"graphed step through the joined net, replay {k}, magnitudes", got, with_magnitudes(single),
             with_magnitudes(want), keys=MAGNITUDES)


@pytest.mark.parametrize("name", ["navier_stokes", "chain"])
def test_two_runs_give_the_same_bits(hip_lib, name):
    """the joined net promises the same bits on every call, as fused_mlp does: features, deltas, magnitudes, new state and
    penalties of two runs are bit-equal"""
    scene = reference(name)[0]
    first = joined_run(hip_lib, name)
    again = run_scene(scene, JoinedOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    for k in first:
        if k.split("/")[-1] in BITWISE + ("magnitudes", "magnitude_loss") and k.startswith("s"):
            assert torch.equal(first[k], again[k]), f"{name} {k} differs between two runs on the same inputs"
