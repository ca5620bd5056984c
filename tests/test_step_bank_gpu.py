"""GPU: the model's whole time step with the four query / key nets as ONE FusedMLPBank, held to
the float64 step oracle of tests/test_step.py with the bar and the allowance of tests/test_step_gpu.py:

    err_hip <= 4 err_torch32 + floor x scale.

``BankOps`` is test_step_gpu.HipOps with one difference: ``queries`` and ``keys`` are the two groups of
``FusedMLPBank([query(0), query(1), key(0), key(1)], groups=2)`` instead of four net calls and two torch.stacks.  Every
case prints its worst ratio (DESIGN.md section 22's table).
"""
import pytest
import torch

import test_step as ts
from test_step import run_scene, scene_tensors
from test_step_gpu import HipOps, fused_network, hold, reference

pytestmark = pytest.mark.gpu


class BankOps(HipOps):
    def step(self, net, t_params, means, u, scaling, transforms, mask, wrap, k, covs=None):
        from pigs_amd import FusedMLPBank, advance_gaussians
        from pigs_amd.covariances import build_covariances
        smp, N = self.sampler, means.shape[0]
        with torch.no_grad():
            if covs is None:
                covs = build_covariances(scaling, transforms)
            smp.preprocess(means, u, covs[0], covs[1], means)
        features = net.seq["input_projection"](t_params[None])                        # [1, N, L]
        smp.preprocess_aggregate()
        rows = features[0]
        qk = FusedMLPBank([net.query(0), net.query(1), net.key(0), net.key(1)], groups=2)(features)      # [2, N, H, K]
        out = smp.aggregate_neighbors_heads(rows, net.transform, qk[0], qk[1], net.frequencies, net.distance_transform)
        joined = torch.cat((features, out.reshape(1, N, -1)), dim=-1)
        deltas = net.seq["delta_net"](joined)                                         # [1, N, 5 + c]
        new = advance_gaussians(means, u, scaling, transforms, deltas, mask[:, None], wrap=wrap)
        rec = {"global_features": rows, "neighbor_features": out.permute(1, 0, 2), "local_global_features": joined[0],
               "deltas": deltas[0]}
        rec.update(new._asdict())
        return rec


@pytest.mark.parametrize("name", ts.FIXTURES)
def test_one_recorded_step_through_the_bank(hip_lib, name):
    """the recorded state, t_params and weights of the reference's own step: every intermediate and every gradient"""
    scene, want, single = reference(name)
    got = run_scene(scene, BankOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    hold(f"{name}, query / key nets in one bank", got, single, want)


def test_the_whole_step_through_the_bank_in_one_graphed_step(hip_lib):
    """as test_step_gpu.test_the_whole_step_in_one_graphed_step: three replays rewrite t_params, the state, the sample
    points and two weight tensors in place; each is held to the oracle under the bar"""
    from pigs_amd.graphs import GraphedStep
    scenes = [reference(f"capture{k}")[0] for k in range(4)]
    net = fused_network(scenes[0].sd)
    params = dict(net.named_parameters())
    holder = {}

    def make_inputs():
        holder["ops"] = BankOps(hip_lib)
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
        hold(f"graphed step through the bank, replay {k}", got, single, want)
