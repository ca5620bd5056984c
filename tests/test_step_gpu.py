"""GPU: the model's whole time step through the HIP operators, as INTEGRATION.md section 4 composes them, against the
float64 step oracle of tests/test_step.py.

The HIP step (``HipOps``): FusedMLP.from_sequential for all six nets, GaussianSampler.preprocess on the incoming state,
preprocess_aggregate, aggregate_neighbors_heads (or H aggregate_neighbors calls), the cat, delta_net, advance_gaussians,
preprocess of the new state's free rows on M = 128 points, sample((0, 1, 2)), the loss + the weighted penalty, and
torch.autograd.grad to every network parameter, to t_params and to the state.

The bar is measured, not fixed, in the form of tests/test_mlp_gpu.py: for every intermediate and every gradient

    err_hip <= 4 err_torch32 + floor x scale,        both errors against the float64 oracle,

err_torch32 that of the same composition in float32 torch ops on the GPU (test_step.step_oracle on float32 tensors);
floor = 1e-6 upstream of the sampler (the MLP's floor), 1e-5 for the loss, the sampler's outputs and every gradient (the
sampler's own tolerance: its cut-off is not in the dense baseline).  Every case prints its worst ratio.

MEASURED (MI355X), worst ratio per case: one recorded step 0.28 - 0.43 with the heads in one launch, 0.24 - 0.46 with H
calls; the head routes apart by 0.31 - 0.57 of one allowance; two chained steps 0.41 / 0.47 / 0.38 (all gradients / state
without gradient / one net frozen); step, refinement, step 0.36; the graphed step's replays 0.69; five Adam steps 0.12.

WHAT THESE CASES FOUND.  With the aggregation's backward as it was, test_one_recorded_step[diffusion-*-separate],
test_two_chained_steps[*] and test_the_whole_step_in_one_graphed_step stood at 1.02 - 1.72: every quantity above its bar
a weight or bias gradient of a QUERY net (once a key net's last bias, whose true gradient is zero), 1e-5 of the size of
delta_net's gradients.  What reaches those nets is d queries_i = sum_j a_ij (da_ij - D_i) keys_j / sqrt(K), a small
difference of large contributions.  The row kernels took D_i = <dacc_i, acc_i> from the forward's saved means, while the
a_ij of the backward are recomputed: sum_j ds_ij did not vanish, and the rest is an error of the same sign in a whole
row.  They now sum D_i = sum_j a_ij da_ij / sum_j a_ij over the pairs, in double, before they form ds
(csrc/aggregate.hip).  These cases are the regression cases of that change.
"""
import numpy as np
import pytest
import torch

import test_step as ts
from test_step import Network, OracleOps, all_scenes, allowance, errors, oracle_run, run_scene, scene_tensors

pytestmark = pytest.mark.gpu

HOSTS = ("native", "ctypes")
ROUTES = ("one_launch", "separate")
BITWISE = ("global_features", "neighbor_features", "local_global_features", "deltas") + ts.OUTPUTS


class HipOps:
    """The three operations a scene is made of, through the library, written as INTEGRATION.md section 4 says."""

    def __init__(self, hip_lib, host="native", route="one_launch", sampler=None):
        from diff_gaussian_sampling import GaussianSampler
        self.sampler = GaussianSampler(False, unpinned_aggregate=True, host=host) if sampler is None else sampler
        self.route = route

    def step(self, net, t_params, means, u, scaling, transforms, mask, wrap, k, covs=None):
        from pigs_amd import advance_gaussians
        from pigs_amd.covariances import build_covariances
        smp, N = self.sampler, means.shape[0]
        with torch.no_grad():                                    # Model.forward :645-648: the sampler bound at the means
            if covs is None:
                covs = build_covariances(scaling, transforms)
            smp.preprocess(means, u, covs[0], covs[1], means)
        features = net.seq["input_projection"](t_params[None])                        # [1, N, L]
        smp.preprocess_aggregate()
        rows = features[0]
        queries = [net.query(h)(features)[0] for h in range(ts.HEADS)]
        keys = [net.key(h)(features)[0] for h in range(ts.HEADS)]
        if self.route == "one_launch":
            out = smp.aggregate_neighbors_heads(rows, net.transform, torch.stack(queries, dim=1), torch.stack(keys, dim=1),
                                                net.frequencies, net.distance_transform)            # [N, H, L]
            joined = torch.cat((features, out.reshape(1, N, -1)), dim=-1)
            heads = out.permute(1, 0, 2)
        else:
            joined, heads = features, []
            for h in range(ts.HEADS):                                                 # :259-266
                heads.append(smp.aggregate_neighbors(rows, net.transform[h], queries[h], keys[h], net.frequencies,
                                                     net.distance_transform[h]))
                joined = torch.cat((joined, heads[-1][None]), dim=-1)
            heads = torch.stack(heads)
        deltas = net.seq["delta_net"](joined)                                         # [1, N, 5 + c]
        out = advance_gaussians(means, u, scaling, transforms, deltas, mask[:, None], wrap=wrap)
        rec = {"global_features": rows, "neighbor_features": heads, "local_global_features": joined[0], "deltas": deltas[0]}
        rec.update(out._asdict())
        return rec

    def refine(self, state, mask, keep, split):
        from pigs_amd.covariances import build_covariances
        from pigs_amd.refine import split_gaussians
        means, u, scaling, transforms = state
        r = split_gaussians(means, scaling, transforms, u, torch.as_tensor(split).cuda(), torch.as_tensor(keep).cuda())
        new_mask = mask.index_select(0, r.source) | (r.child >= 0)
        return [r.means, r.values, r.scaling, r.transforms], new_mask, build_covariances(r.scaling, r.transforms)

    def sample(self, means, u, covariances, conics, samples):
        self.sampler.preprocess(means, u, covariances, conics, samples)
        return self.sampler.sample((0, 1, 2))


def fused_network(sd):
    import pigs_amd
    return Network(sd, torch.float32, "cuda").fuse(pigs_amd.FusedMLP.from_sequential)


def hold(what, got, ref32, want, keys=None):
    """the bar of the module text over every name of ``want`` (or ``keys``); returns the worst err_hip / allowance"""
    e_hip, e_t = errors(got, want), errors(ref32, want)
    worst, bad = 0.0, []
    for k in (want if keys is None else keys):
        assert tuple(got[k].shape) == tuple(want[k].shape), (what, k, tuple(got[k].shape), tuple(want[k].shape))
        ratio = e_hip[k][0] / allowance(k, *e_t[k])
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad.append(f"{k}: hip {e_hip[k][0]:.3g}, torch32 {e_t[k][0]:.3g}, scale {e_hip[k][1]:.3g}, ratio {ratio:.3g}")
    print(f"[figure] {what}: worst err_hip / (4 err_torch32 + floor x scale) = {worst:.3f}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return worst


_reference, _hip = {}, {}


def reference(name):
    """the scene, the float64 oracle's results (CPU) and the float32 torch composition's (GPU): computed once, shared"""
    if name not in _reference:
        scene, want, _ = oracle_run(name)
        single = run_scene(scene, OracleOps(), Network(scene.sd, torch.float32, "cuda"), torch.float32, "cuda")
        _reference[name] = (scene, want, single)
    return _reference[name]


def hip_run(hip_lib, name, host="native", route="one_launch"):
    key = (name, host, route)
    if key not in _hip:
        scene = reference(name)[0]
        _hip[key] = run_scene(scene, HipOps(hip_lib, host, route), fused_network(scene.sd), torch.float32, "cuda")
    return _hip[key]


# ---- 1. one step from each fixture --------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name", ts.FIXTURES)
def test_one_recorded_step(hip_lib, name, host, route):
    """the recorded state, t_params and weights of the reference's own step (rounded to float32): every intermediate and
    every gradient, on both hosts of the sampler, the heads in one launch and as H calls"""
    scene, want, single = reference(name)
    hold(f"{name}, host {host}, heads {route}", hip_run(hip_lib, name, host, route), single, want)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name", ts.FIXTURES)
def test_the_two_head_routes_agree(hip_lib, name, host):
    """one launch for all heads against H separate calls: both run the same arithmetic per head, so their difference is
    held to ONE allowance of the bar (each meeting the bar alone would grant two)"""
    scene, want, single = reference(name)
    a, b = hip_run(hip_lib, name, host, "one_launch"), hip_run(hip_lib, name, host, "separate")
    e_t, diff = errors(single, want), errors(a, b)
    ratios = {k: diff[k][0] / allowance(k, *e_t[k]) for k in want}
    worst = max(ratios, key=ratios.get)
    print(f"[figure] {name}, host {host}: the head routes differ by at most {ratios[worst]:.3f} x the allowance ({worst})")
    assert ratios[worst] <= 1.0, (worst, ratios[worst])


# ---- 2. two chained steps, one backward ---------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["all_gradients", "state_without_gradient", "one_net_frozen"])
def test_two_chained_steps(hip_lib, variant):
    """N = 257, c = 2, wrap: step 2 rebuilds the sampler's lists, plans and the MLP scratch while step 1's are still owed a
    backward; its t_params carry step 1's covariances and u (a strided slice of a cat arrives at advance's backward).  The
    gradients with respect to step 1's inputs and to the shared weights meet the bar -- also when the state asks for no
    gradient, and with one net frozen."""
    scene, want, single = reference("chain")
    if variant == "all_gradients":
        got = hip_run(hip_lib, "chain")
    else:
        net = fused_network(scene.sd)
        frozen = []
        if variant == "one_net_frozen":
            frozen = ["key_transform.0." + n for n, p in net.key(0).named_parameters()]
            for p in net.key(0).parameters():
                p.requires_grad_(False)
        got = run_scene(scene, HipOps(hip_lib), net, torch.float32, "cuda", state_grad=variant != "state_without_gradient")
        missing = {k for k in want if k not in got}
        expect = {"grad/" + n for n in frozen} if frozen else {"grad/" + n for n in ts.STATE}
        assert missing == expect, (missing, expect)
    assert float(want["s1/means"].sub(want["s0/means"]).abs().max()) > 0
    hold(f"two chained steps, {variant}", got, single, want, keys=[k for k in want if k in got])


# ---- 3. a step, a refinement, a step ------------------------------------------------------------------------
def test_step_refinement_step(hip_lib):
    """split_gaussians with seeded keep / split masks between two steps (no criterion: no decision on a tie): N goes from
    257 to a count that is no multiple of 16, the second step runs at the new N on the same sampler and the same FusedMLP
    objects; results and gradients through both steps and the surgery"""
    scene, want, single = reference("refine")
    got = hip_run(hip_lib, "refine")
    n_new = got["s1/means"].shape[0]
    assert n_new == want["s1/means"].shape[0] and n_new != 257 and n_new % 16
    hold(f"step, refinement 257 -> {n_new}, step", got, single, want)


# ---- 4. capture ---------------------------------------------------------------------------------------------
def test_the_whole_step_in_one_graphed_step(hip_lib):
    """GraphedStep over the whole step, preprocess_aggregate included (N = 257: the lists are built without a read-back).
    Three replays rewrite t_params, the state, the sample points and two weight tensors in place; each is held to the
    oracle under the bar, independent of the eager step, and the largest replay-against-eager difference is printed."""
    from pigs_amd.graphs import GraphedStep
    scenes = [reference(f"capture{k}")[0] for k in range(4)]
    net = fused_network(scenes[0].sd)
    params = dict(net.named_parameters())
    holder = {}

    def make_inputs():
        holder["ops"] = HipOps(hip_lib)
        x = holder["x"] = scene_tensors(scenes[0], torch.float32, "cuda")
        return x.t_params + x.state

    def fn(*leaves):
        rec = run_scene(scenes[0], holder["ops"], net, tensors=holder["x"])
        holder["names"] = list(rec)
        return tuple(rec.values())
    step = GraphedStep(fn, make_inputs, warmup=2)
    apart = 0.0
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
        hold(f"graphed step, replay {k}", got, single, want)
        eager = hip_run(hip_lib, f"capture{k}")
        apart = max([apart] + [e / s for e, s in errors(got, eager).values()])
    print(f"[figure] graphed step: the replays differ from the eager step by at most {apart:.3g} of a tensor's scale")


# ---- 5. five Adam steps -------------------------------------------------------------------------------------
def test_five_adam_steps(hip_lib):
    """torch.optim.Adam on the network's parameters through the HIP step and through the float32 torch step, both loss
    curves against the float64 curve: err_hip <= 4 err_torch32 + 1e-6 of the loss"""
    scene = reference("navier_stokes")[0]
    want = ts.adam_curve(scene, OracleOps(), Network(scene.sd), torch.float64, "cpu")
    single = ts.adam_curve(scene, OracleOps(), Network(scene.sd, torch.float32, "cuda"), torch.float32, "cuda")
    got = ts.adam_curve(scene, HipOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    err_h, err_t, scale = np.abs(got - want).max(), np.abs(single - want).max(), ts.scale_of(want)
    print(f"[figure] five Adam steps: hip {err_h:.3g}, torch32 {err_t:.3g} off the float64 curve of scale {scale:.3g}: "
          f"ratio {err_h / (4.0 * err_t + 1e-6 * scale):.3f}")
    assert want[-1] < want[0]
    assert err_h <= 4.0 * err_t + 1e-6 * scale


# ---- 6. determinism -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["navier_stokes", "chain"])
def test_two_runs_give_the_same_bits_upstream_of_the_samplers_backward(hip_lib, name):
    """fused_mlp and advance_gaussians promise the same bits on every call, the aggregation's forward sums its lists in a
    fixed order: features, deltas, new state and penalties of two runs are bit-equal (the gradients behind the sampler's
    atomics meet only the bar: cases 1 and 2)"""
    scene = reference(name)[0]
    first = hip_run(hip_lib, name)
    again = run_scene(scene, HipOps(hip_lib), fused_network(scene.sd), torch.float32, "cuda")
    for k in first:
        if k.split("/")[-1] in BITWISE and k.startswith("s"):
            assert torch.equal(first[k], again[k]), f"{name} {k} differs between two runs on the same inputs"
