"""CPU: the model's whole time step composed from the checkers the suite already owns, in float64 -- and pinned.

INTEGRATION.md section 4 puts six HIP operators together: input_projection -> query / key nets -> preprocess_aggregate +
aggregate_neighbors_heads -> cat -> delta_net -> advance_gaussians -> preprocess -> sampler outputs -> loss -> one
backward.  ``step_oracle`` is that chain in plain torch (nn.Sequential, oracle/aggregate_torch.py,
test_advance.torch_forward; oracle/dense_torch.forward for the sampler end, test_refine.refine_oracle for the
refinement), autograd supplies every gradient, dtype and device follow the inputs: in float64 on the CPU it is the
reference of tests/test_step_gpu.py, in float32 it is the composition the HIP step's error is measured against.

Here, without a GPU:
  * pinning: the oracle reproduces every recorded tensor and gradient of one ``Model.forward`` of the reference
    (tests/golden/model_pn_step/*.npz, tools/gen_model_step.py) at 1e-10 of each tensor's scale;
  * input conditions, on the fixtures and on every scene of the GPU file, none excepted: no pair of Gaussians has q
    within a relative 1e-4 of q_max (a neighbour that flips between float32 and float64 changes a softmax), no updated
    mean lies within 1e-5 of a wrap edge.  A scene that violated one got another seed (SEEDS);
  * the bar discriminates: six perturbations of the ORACLE each move a checked quantity by at least 100 x what the GPU
    bar allows for it, the allowance taken with the float32 composition's error measured on the CPU.
"""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import aggregate_torch, dense_torch
from test_advance import OUTPUTS, scale_of, torch_forward
from test_refine import refine_oracle

HEADS, LATENT, Q_MAX, M = 2, 16, 36.0, 128
FIXTURES = ("diffusion", "navier_stokes")
STATE = ("means", "u", "scaling", "transforms")
NETS = ("input_projection", "query_transform.0", "query_transform.1", "key_transform.0", "key_transform.1", "delta_net")
PENALTY_WEIGHTS = (2.0, 2.0, 2.0, 1.0)     # dmean, dscale, dtransform, du weights of the model, in the penalty's order
UPSTREAM = ("global_features", "neighbor_features", "local_global_features", "deltas") + OUTPUTS
FLOOR_UPSTREAM, FLOOR_SAMPLER = 1e-6, 1e-5
Q_MARGIN, WRAP_MARGIN = 1e-4, 1e-5
# the seed of every synthetic scene: the first, counted up from the scene's number x 100, that meets the input conditions
# (and, with a refinement, leaves a row count that is no multiple of 16)
SEEDS = {"chain": 100, "refine": 202, "capture0": 300, "capture1": 401, "capture2": 500, "capture3": 608}


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, "model_pn_step", f"{name}.npz")) as f:
        return {k: f[k] for k in f.files}


def as_float32(a):
    """the values a float32 path can hold, in float64: every path of a scene starts from the same numbers"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- the network --------------------------------------------------------------------------------------------
class Network:
    """The six nn.Sequential nets, transform, distance_transform and frequencies of a recorded dynamics_network, under
    the reference's state_dict keys."""

    def __init__(self, sd, dtype=torch.float64, device="cpu"):
        def tensor(a):          # a copy: an optimiser steps these in place, the scene's arrays stay what they are
            return torch.tensor(np.asarray(a), dtype=dtype, device=device)
        self.seq = {}
        for prefix in NETS:
            index = sorted(int(k[len(prefix) + 1:].split(".")[0]) for k in sd
                           if k.startswith(prefix + ".") and k.endswith(".weight"))
            mods = []
            for i in index:
                W = sd[f"{prefix}.{i}.weight"]
                linear = torch.nn.Linear(W.shape[1], W.shape[0]).to(device=device, dtype=dtype)
                with torch.no_grad():
                    linear.weight.copy_(tensor(W))
                    linear.bias.copy_(tensor(sd[f"{prefix}.{i}.bias"]))
                mods += [linear, torch.nn.Tanh()]
            self.seq[prefix] = torch.nn.Sequential(*mods[:-1])
            assert [2 * k for k in range(len(index))] == index
        self.transform = tensor(sd["transform"]).requires_grad_(True)
        self.distance_transform = tensor(sd["distance_transform"]).requires_grad_(True)
        self.frequencies = tensor(sd["frequencies"])

    def query(self, h):
        return self.seq[f"query_transform.{h}"]

    def key(self, h):
        return self.seq[f"key_transform.{h}"]

    def named_parameters(self):
        out = [(f"{prefix}.{n}", p) for prefix in NETS for n, p in self.seq[prefix].named_parameters()]
        return out + [("transform", self.transform), ("distance_transform", self.distance_transform)]

    def fuse(self, wrap):
        """every net through ``wrap`` (FusedMLP.from_sequential on the GPU): the same Parameters under the same names"""
        self.seq = {k: wrap(v) for k, v in self.seq.items()}
        return self


# ---- the oracle ---------------------------------------------------------------------------------------------
def flat_covariances(scaling, transforms):
    tau = torch.tanh(transforms[:, 0]) * torch.sqrt(scaling[:, 0] * scaling[:, 1])
    det = scaling[:, 0] * scaling[:, 1] - tau * tau
    return (torch.stack((scaling[:, 0], tau, scaling[:, 1]), -1),
            torch.stack((scaling[:, 1] / det, -tau / det, scaling[:, 0] / det), -1))


def q_margin(means, conics):
    """the smallest |q_ij / q_max - 1| over all pairs: how far the nearest pair is from changing sides"""
    delta = means[None, :, :] - means[:, None, :]
    a, b, c = conics[:, 0], conics[:, 1], conics[:, 2]
    q = a[None] * delta[..., 0] ** 2 + 2 * b[None] * delta[..., 0] * delta[..., 1] + c[None] * delta[..., 1] ** 2
    return float((q / Q_MAX - 1.0).abs().min())


def step_oracle(net, t_params, means, u, scaling, transforms, mask, wrap=None, *, perturb=None, lists=None):
    """One time step: t_params [N, in] and the state -> the features, the heads' neighbour features, their cat, the deltas
    and the nine outputs of the update (a dict), and the neighbour structure it used.  The neighbour structure is that of
    the INCOMING state (the model binds the sampler at :648, before the network runs) and a constant of autograd.
    ``perturb``: one of the deliberate mistakes of test_the_bar_discriminates; ``lists``: a structure to use instead."""
    if lists is None:
        conics = flat_covariances(scaling.detach(), transforms.detach())[1]
        lists = aggregate_torch.neighbor_structure(means.detach(), conics, Q_MAX)
    features = net.seq["input_projection"](t_params)
    heads = [aggregate_torch.aggregate(*lists, features, net.transform[h], net.query(h)(features), net.key(h)(features),
                                       net.frequencies, net.distance_transform[h]) for h in range(HEADS)]
    joined = torch.cat([features] + (heads[::-1] if perturb == "heads_swapped" else heads), dim=-1)
    deltas = net.seq["delta_net"](joined)
    if perturb == "columns_exchanged":          # dtransforms read where dscaling starts
        deltas = deltas[:, [0, 1, 3, 4, 2] + list(range(5, deltas.shape[1]))]
    outs = torch_forward(means, u, scaling, transforms, deltas, mask, wrap)
    if perturb == "mask_ignored":               # the values of the masked update, the gradients of an unmasked one
        free = torch_forward(means, u, scaling, transforms, deltas, torch.ones_like(mask), wrap)
        outs = [a + (o - a).detach() for o, a in zip(outs, free)]
    rec = {"global_features": features, "neighbor_features": torch.stack(heads), "local_global_features": joined,
           "deltas": deltas}
    rec.update(zip(OUTPUTS, outs))
    return rec, lists


class OracleOps:
    """The three operations a scene is made of, in torch; ``margins`` collects the input conditions of every step."""

    def __init__(self, perturb=None):
        self.perturb, self.first_lists, self.margins = perturb, None, []

    def step(self, net, t_params, means, u, scaling, transforms, mask, wrap, k, covs=None):
        lists = None
        if self.perturb == "lists_post_update":
            with torch.no_grad():
                new = step_oracle(net, t_params, means, u, scaling, transforms, mask, wrap)[0]
            lists = aggregate_torch.neighbor_structure(new["means"], new["conics"], Q_MAX)
        if self.perturb == "stale_lists" and k > 0:
            lists = self.first_lists
        rec, lists = step_oracle(net, t_params, means, u, scaling, transforms, mask, wrap, perturb=self.perturb, lists=lists)
        if k == 0:
            self.first_lists = lists
        if means.dtype == torch.float64 and self.perturb is None:
            with torch.no_grad():
                moved = means + rec["deltas"][:, 0:2] * mask[:, None]
                edge = float("inf") if wrap is None else float(torch.minimum((moved - wrap[0]).abs(), (moved - wrap[1]).abs()).min())
                self.margins.append((q_margin(means, flat_covariances(scaling, transforms)[1]), edge))
        return rec

    def refine(self, state, mask, keep, split):
        means, u, scaling, transforms = state
        host = [t.detach().cpu().double().numpy() for t in (means, scaling, transforms, u)]
        o = refine_oracle(*host, keep, split)

        def const(a, dtype=means.dtype):
            return torch.as_tensor(a, dtype=dtype, device=means.device)
        source, fresh = const(o.source, torch.long), const(o.child >= 0, torch.bool)
        new = [means[source] + const(o.means - host[0][o.source]), u[source] * const(np.where(o.child >= 0, 0.5, 1.0))[:, None],
               scaling[source], transforms[source]]          # e is a constant, as under the reference's no_grad
        return new, mask[source] | fresh, flat_covariances(new[2], new[3])

    def sample(self, means, u, covariances, conics, samples):
        out = dense_torch.forward(means, conics, u, samples, orders=(0, 1, 2))
        return out[0], out[1], out[2]


# ---- scenes -------------------------------------------------------------------------------------------------
def couple(base, covariances, u):
    """the next step's t_params: the model's carry the full covariances and u in their first columns (:248-249)"""
    full = torch.stack((covariances[:, 0], covariances[:, 1], covariances[:, 1], covariances[:, 2]), dim=-1)
    return torch.cat((full, u, base[:, 4 + u.shape[1]:]), dim=-1)


def fixture_scene(name):
    fx = load_fixture(name)
    mask = fx["boundary_mask"]
    rng = np.random.default_rng(len(name))
    return types.SimpleNamespace(
        name=name, sd={k[3:]: as_float32(v) for k, v in fx.items() if k.startswith("sd/")}, mask=mask,
        wrap=tuple(float(x) for x in fx["wrap"]) or None, t_params=[as_float32(fx["t_params"])],
        state={k: as_float32(fx["in/" + k]) for k in STATE}, samples=as_float32(rng.uniform(-1.0, 1.0, (M, 2))),
        keep=None, split=None, n_boundary=int((~mask).sum()))


def synthetic_scene(name, steps=2, refine=False, N=257, seed=None, rewrite=0):
    """N = 257 Gaussians (one past a 256-thread workgroup of advance and one past sixteen 16-row MLP tiles), c = 2, wrap
    (-1, 1), the Navier-Stokes fixture's weights; 50 boundary rows in front.  Narrow Gaussians (variance about e^-6): some
    twenty neighbours each, so that a seed without a pair on the cut-off exists.  ``rewrite`` = k: delta_net's last weight
    and ``transform`` scaled, the two tensors that replay k of the captured step rewrites in place."""
    seed = SEEDS[name] if seed is None else seed
    fx = load_fixture("navier_stokes")
    rng = np.random.default_rng(seed)
    width = fx["t_params"].shape[1]
    mask = np.arange(N) >= 50
    state = {"means": rng.uniform(-1.0, 1.0, (N, 2)), "u": rng.standard_normal((N, 2)) * 0.2,
             "scaling": np.exp(rng.standard_normal((N, 2)) * 0.3 - 6.0), "transforms": np.tanh(rng.standard_normal((N, 1)) * 0.3)}
    keep = split = None
    rows = [N] * steps
    if refine:
        keep = (rng.random(N) >= 0.05) | ~mask
        split = (rng.random(N) < 0.15) & mask
        rows[1] = int(keep.sum() + (keep & split).sum())
    sd = {k[3:]: v for k, v in fx.items() if k.startswith("sd/")}
    sd["delta_net.10.weight"] = sd["delta_net.10.weight"] * (1.0 + 0.1 * rewrite)      # what a replay writes in place
    sd["transform"] = sd["transform"] * (1.0 - 0.05 * rewrite)
    return types.SimpleNamespace(
        name=name, sd={k: as_float32(v) for k, v in sd.items()}, mask=mask, wrap=(-1.0, 1.0),
        t_params=[as_float32(rng.standard_normal((n, width)) * 0.5) for n in rows],
        state={k: as_float32(v) for k, v in state.items()}, samples=as_float32(rng.uniform(-1.0, 1.0, (M, 2))),
        keep=keep, split=split, n_boundary=50)


def all_scenes():
    """every scene of tests/test_step_gpu.py"""
    scenes = {name: fixture_scene(name) for name in FIXTURES}
    scenes["chain"] = synthetic_scene("chain")
    scenes["refine"] = synthetic_scene("refine", refine=True)
    for k in range(4):                                     # the captured step and the three states its replays run on
        scenes[f"capture{k}"] = synthetic_scene(f"capture{k}", steps=1, rewrite=k)
    return scenes


def scene_tensors(scene, dtype=torch.float64, device="cpu", state_grad=True):
    """the scene's arrays as tensors: the t_params of every step and the first state (leaves), the mask, the sample
    points and the penalty's weights"""
    def tensor(a):
        return torch.as_tensor(a, dtype=dtype, device=device)
    return types.SimpleNamespace(
        t_params=[tensor(t).requires_grad_(True) for t in scene.t_params],
        state=[tensor(scene.state[k]).requires_grad_(state_grad) for k in STATE],
        mask=torch.as_tensor(scene.mask, device=device), samples=tensor(scene.samples), weights=tensor(PENALTY_WEIGHTS))


def run_scene(scene, ops, net, dtype=torch.float64, device="cpu", state_grad=True, tensors=None):
    """The scene through ``ops``: every intermediate of every step (``s<k>/<name>``), the sampler's outputs on the last
    state's free rows, the loss (mean squares of u, grad u and the Hessian + the weighted penalties of every step) and its
    gradient with respect to every parameter that requires one, to the t_params of every step and to the first state."""
    x = scene_tensors(scene, dtype, device, state_grad) if tensors is None else tensors
    steps = len(x.t_params)
    t_params, state, mask, samples, weights = x.t_params, list(x.state), x.mask, x.samples, x.weights
    rec, loss, covs = {}, 0.0, None
    for k in range(steps):
        t = t_params[k] if k == 0 else couple(t_params[k], covs[0], state[1])
        s = ops.step(net, t, *state, mask, scene.wrap, k, covs)
        rec.update({f"s{k}/{name}": v for name, v in s.items()})
        loss = loss + (s["penalty"] * weights).sum()
        state, covs = [s[name] for name in STATE], (s["covariances"], s["conics"])
        if scene.split is not None and k == 0:
            state, mask, covs = ops.refine(state, mask, scene.keep, scene.split)
            rec.update({f"refined/{name}": v for name, v in zip(STATE + ("covariances", "conics"), state + list(covs))})
    nb = scene.n_boundary
    f, fx, fxx = ops.sample(state[0][nb:], state[1][nb:], covs[0][nb:], covs[1][nb:], samples)
    loss = loss + torch.mean(f ** 2) + 1e-3 * torch.mean(fx ** 2) + 1e-6 * torch.mean(fxx ** 2)
    rec.update(f=f, fx=fx, fxx=fxx, loss=loss)
    leaves = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    leaves += [(f"t_params{k}", t) for k, t in enumerate(t_params)]
    leaves += [(n, t) for n, t in zip(STATE, x.state) if t.requires_grad]
    grads = torch.autograd.grad(loss, [t for _, t in leaves], allow_unused=True)
    for (name, leaf), g in zip(leaves, grads):
        rec["grad/" + name] = torch.zeros_like(leaf) if g is None else g
    return {k: v.detach() for k, v in rec.items()}


def floor_of(name):
    """1e-6 of scale upstream of the sampler (the MLP's floor), 1e-5 for the loss, the sampler's outputs and every
    gradient: they are downstream of the sampler, whose cut-off is not in the dense baseline"""
    return FLOOR_UPSTREAM if name.split("/")[0].startswith(("s0", "s1", "refined")) else FLOOR_SAMPLER


def host(t):
    return t.detach().cpu().double().numpy()


def scale_from(name):
    """The tensor whose largest magnitude is the scale of ``name``: its own, except for the gradient of a key net's last
    bias.  That bias adds the same <query_i, b> to every score of row i, the softmax does not see it, and its gradient is
    zero but for rounding: it is held to the scale of the same layer's weight gradient."""
    if "key_transform" in name and name.endswith(".6.bias"):
        return name[:-len("bias")] + "weight"
    return name


def errors(got, want):
    """{name: (largest absolute error, scale of the reference)} over the names both hold"""
    return {k: (float(np.abs(host(got[k]) - host(want[k])).max()), scale_of(host(want[scale_from(k)]))) for k in want if k in got}


def allowance(name, err_torch32, scale):
    return 4.0 * err_torch32 + floor_of(name) * scale


_runs = {}


def oracle_run(name, dtype=torch.float64):
    """the unperturbed oracle on a scene: computed once, shared, never changed.  Returns (scene, results, margins)"""
    if (name, dtype) not in _runs:
        scene = all_scenes()[name]
        ops = OracleOps()
        _runs[(name, dtype)] = (scene, run_scene(scene, ops, Network(scene.sd, dtype), dtype), ops.margins)
    return _runs[(name, dtype)]


def adam_curve(scene, ops, net, dtype, device, steps=5, lr=1e-3):
    """the losses of five torch.optim.Adam steps on the network's parameters, the scene's inputs fixed"""
    params = [p for _, p in net.named_parameters()]
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for _ in range(steps):
        rec = run_scene(scene, ops, net, dtype, device, state_grad=False)
        for (name, p) in net.named_parameters():
            p.grad = rec["grad/" + name].clone()
        opt.step()
        losses.append(float(rec["loss"]))
    return np.array(losses)


# ---- pinning ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_recorded_step(name):
    """float64 against float64: every recorded tensor and every gradient of the recorded functional, 1e-10 of scale"""
    fx = load_fixture(name)
    net = Network({k[3:]: v for k, v in fx.items() if k.startswith("sd/")})
    assert sorted(n for n, _ in net.named_parameters()) == sorted(k[3:] for k in fx if k.startswith("sd/") and k != "sd/frequencies")
    t_params = torch.tensor(fx["t_params"], requires_grad=True)
    state = [torch.tensor(fx["in/" + k], requires_grad=True) for k in STATE]
    mask = torch.tensor(fx["boundary_mask"])
    wrap = tuple(float(x) for x in fx["wrap"]) or None
    rec, _ = step_oracle(net, t_params, *state, mask, wrap)
    c = state[1].shape[1]
    rec.update(dmeans=rec["deltas"][:, 0:2], dscaling=rec["deltas"][:, 2:4], dtransforms=rec["deltas"][:, 4:5],
               du=rec["deltas"][:, 5:5 + c])
    worst = 0.0

    def hold(what, got, want):
        nonlocal worst
        assert got.shape == want.shape, what
        err = np.abs(host(got) - want).max() / scale_of(fx.get(scale_from(what), want))
        worst = max(worst, err)
        assert err <= 1e-10, f"{name} {what}: {err:.3g} of its scale"
    for key in ("global_features", "neighbor_features", "local_global_features", "deltas", "dmeans", "dscaling",
                "dtransforms", "du", "penalty"):
        hold(key, rec[key], fx[key])
    for key in OUTPUTS[:-1]:
        hold("out/" + key, rec[key], fx["out/" + key])
    loss = sum((torch.tensor(fx["w/" + k]) * rec[k]).sum() for k in STATE + ("conics", "penalty"))
    leaves = net.named_parameters() + [("t_params", t_params)] + list(zip(STATE, state))
    for (key, _), g in zip(leaves, torch.autograd.grad(loss, [t for _, t in leaves])):
        hold("grad/" + key, g, fx["grad/" + key])
    assert len([k for k in fx if k.startswith("grad/")]) == len(leaves)
    if wrap is not None:
        assert (np.abs(fx["in/means"] + fx["dmeans"]) > 1.0).any()          # some recorded rows crossed an edge
    print(f"[figure] {name}: oracle against the recorded step, worst {worst:.3g} of a tensor's scale")


def test_fixtures_hold_float64_data_within_the_size_of_the_largest_fixture():
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    for name in FIXTURES:
        fx = load_fixture(name)
        N = fx["in/means"].shape[0]
        assert N % 16 and N % 64 and N <= 300
        assert all(v.dtype == np.float64 for k, v in fx.items() if k != "boundary_mask")
        assert os.path.getsize(os.path.join(GOLDEN, "model_pn_step", f"{name}.npz")) <= largest


# ---- input conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(all_scenes()))
def test_input_conditions(name):
    """no pair on the cut-off, no updated mean on a wrap edge: in every step of every scene, float64, none excepted"""
    scene, rec, margins = oracle_run(name)
    assert len(margins) == len(scene.t_params)
    for k, (q, edge) in enumerate(margins):
        assert q >= Q_MARGIN, f"{name} step {k}: a pair has q within {q:.3g} of q_max (relative)"
        assert edge >= WRAP_MARGIN, f"{name} step {k}: an updated mean lies {edge:.3g} from a wrap edge"
    if scene.split is not None:
        n_new = rec["s1/means"].shape[0]
        assert n_new != scene.mask.size and n_new % 16, n_new
        assert not (scene.split & ~scene.mask).any() and (scene.keep | scene.mask).all()      # the boundary rows stay a prefix
    print(f"[figure] {name}: q margins {[f'{q:.2g}' for q, _ in margins]}, edge margins {[f'{e:.2g}' for _, e in margins]}")


def test_input_conditions_of_the_adam_steps():
    """the weights move in the five Adam steps, so the deltas do: the same two conditions in each of them"""
    scene = all_scenes()["navier_stokes"]
    ops = OracleOps()
    losses = adam_curve(scene, ops, Network(scene.sd), torch.float64, "cpu")
    assert len(ops.margins) == 5 and losses[-1] < losses[0]
    for q, edge in ops.margins:
        assert q >= Q_MARGIN and edge >= WRAP_MARGIN, (q, edge)


# ---- the bar discriminates ----------------------------------------------------------------------------------
PERTURBATIONS = [("heads_swapped", "diffusion"), ("heads_swapped", "navier_stokes"), ("columns_exchanged", "diffusion"),
                 ("columns_exchanged", "navier_stokes"), ("mask_ignored", "diffusion"), ("mask_ignored", "chain"),
                 ("lists_post_update", "navier_stokes"), ("lists_post_update", "chain"), ("stale_lists", "chain"),
                 ("bias_dropped", "diffusion"), ("bias_dropped", "navier_stokes")]


@pytest.mark.parametrize("perturb,name", PERTURBATIONS)
def test_the_bar_discriminates(perturb, name):
    """A mistake made in the ORACLE -- heads swapped in the cat, the dscaling / dtransforms columns exchanged, the mask
    ignored in the deltas' gradient, neighbour lists of the post-update state, step 1's lists reused in step 2, delta_net's
    last bias dropped from the gradient set -- moves at least one checked quantity by 100 x what the GPU bar allows for it,
    4 err_torch32 + floor x scale with the float32 composition's error measured here on the CPU."""
    scene, want, _ = oracle_run(name)
    _, single, _ = oracle_run(name, torch.float32)
    if perturb == "bias_dropped":
        wrong = dict(want)
        wrong["grad/delta_net.10.bias"] = torch.zeros_like(want["grad/delta_net.10.bias"])
    else:
        wrong = run_scene(scene, OracleOps(perturb), Network(scene.sd))
    err32, moved = errors(single, want), errors(wrong, want)
    margins = {k: moved[k][0] / allowance(k, *err32[k]) for k in want}
    best = max(margins, key=margins.get)
    print(f"[figure] {perturb} on {name}: {best} moves by {margins[best]:.3g} x its allowance")
    assert margins[best] >= 100.0, f"{perturb} on {name}: nothing moves by more than {margins[best]:.3g} x its allowance"
