#!/usr/bin/env python3
"""One recorded time step of the reference's PINN model, in float64, for tests/test_step.py.

TEST INFRASTRUCTURE, build container only: like tools/gen_model_trace.py (whose device rewriting mode, dense oracle
and boundary points it reuses) it imports the reference's model_pn.py read-only and never copies from it.  Under
``torch.set_default_dtype(torch.float64)`` it constructs ``model_pn.Model`` for

    DIFFUSION       c = 1, no wrap, 100 boundary Gaussians in front of a 7 x 7 lattice made random by ``randomize``
    NAVIER_STOKES   c = 2, wrap (-1, 1), a seeded cloud of 117 Gaussians through ``set_initial_params``

(N = 149 and 117: multiples of neither 16 nor 64, and as many rows as the size of the largest fixture allows), drives ``sample`` -> ``forward(t, dt, False)`` once with a stand-in
sampler -- ``sample_*`` from the dense float64 oracle, the aggregation from oracle/aggregate_torch.py (parity unpinned:
the reference's own arithmetic is absent) -- and records

  * ``sd/<key>``: the state_dict of dynamics_network without input_transform (the six nets, transform,
    distance_transform, frequencies),
  * ``t_params`` (the input of input_projection; InputTransform stays out of scope), the state that went in
    (``in/means`` ...), ``boundary_mask``,
  * ``global_features``, ``neighbor_features`` [H, N, L], ``local_global_features``, ``deltas`` and its four slices, the
    new state (``out/means`` ... ``out/full_conics``) and ``penalty``, the four mean(x[mask] ** 2) of compute_loss,
  * ``w/<name>``: seeded weights of a linear functional of the new means, u, scaling, transforms, conics and the penalty,
    and ``grad/<name>``: its gradient with respect to every recorded parameter, to t_params and to the incoming state.
    The state's gradient is the one through the update alone (t_params is an input of its own here: a hook stops the
    gradient at it for that pass).

    python tools/gen_model_step.py            # writes tests/golden/model_pn_step/{diffusion,navier_stokes}.npz

(a directory of their own: tests/conftest.py hands every other *.npz directly under tests/golden/ to the sampler's parity
tests as a sampler fixture.)
"""
import os
import sys
import types

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_model_trace as trace       # noqa: E402

KEPT = ("input_projection.", "query_transform.", "key_transform.", "delta_net.", "transform", "distance_transform",
        "frequencies")
STATE = ("means", "u", "scaling", "transforms")


class StepSampler:
    """diff_gaussian_sampling.GaussianSampler for the reference's eyes: dense float64 oracle, no recording"""

    def __init__(self, flag=False):
        self.args = None

    def preprocess(self, means, values, covariances, conics, samples):
        self.args = (means, values.reshape(means.shape[0], -1), conics.reshape(means.shape[0], -1), samples)

    def _order(self, o):
        return trace.dense_orders(*self.args, (o,))[o]

    def sample_gaussians(self):
        return self._order(0)

    def sample_gaussians_derivative(self):
        return self._order(1)

    def sample_gaussians_laplacian(self):
        return self._order(2)

    def sample_gaussians_third_derivative(self):
        return self._order(3)

    def preprocess_aggregate(self):
        from oracle import aggregate_torch
        self.lists = aggregate_torch.neighbor_structure(self.args[0].detach(), self.args[2].detach(), 36.0)

    def aggregate_neighbors(self, features, transform, queries, keys, frequencies, distance_transform):
        from oracle import aggregate_torch
        return aggregate_torch.aggregate(*self.lists, features, transform, queries, keys, frequencies, distance_transform)


def install():
    mod = types.ModuleType("diff_gaussian_sampling")
    mod.GaussianSampler = StepSampler
    sys.modules["diff_gaussian_sampling"] = mod
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, trace.REF)


def record(problem_name, n_lattice, n_cloud, seed):
    import model_pn
    torch.manual_seed(seed)
    np.random.seed(seed)
    problem = getattr(model_pn.Problem, problem_name)
    scale, d = 1.0, 2
    model = model_pn.Model(problem, model_pn.IntegrationRule.TRAPEZOID, n_lattice, n_lattice, d, scale)
    model.train()
    if problem == model_pn.Problem.NAVIER_STOKES:
        n = n_cloud
        model.set_initial_params((torch.rand((n, d)) * 2.0 - 1.0) * scale, torch.randn((n, 2)) * 0.2,
                                 torch.exp(torch.randn((n, d)) * 0.3 - 4.0) * scale, torch.tanh(torch.randn((n, 1)) * 0.3))
    else:
        model.randomize(n_lattice)
    model.sample((torch.rand((64, d)) * 2.0 - 1.0) * scale, trace.boundary_points(64, scale))
    for name in STATE:
        setattr(model, name, getattr(model, name).detach().clone().requires_grad_(True))
    state_in = {name: getattr(model, name) for name in STATE}
    mask = model.boundary_mask.squeeze(-1).clone()
    model.forward(0.0, 1.0, False)

    net = model.dynamics_network
    assert net.t_params.dtype == torch.float64 and model.conics.dtype == torch.float64
    L = model_pn.LATENT_SIZE
    lgf = net.local_global_features
    slices = {"dmeans": model.dmeans, "dscaling": model.dscaling, "dtransforms": model.dtransforms, "du": model.du}
    penalty = torch.stack([torch.mean(x[mask] ** 2) for x in slices.values()])
    out = {"means": model.means, "u": model.u, "scaling": model.scaling, "transforms": model.transforms,
           "covariances": model.covariances, "conics": model.conics, "full_covariances": model.full_covariances,
           "full_conics": model.full_conics}
    gen = torch.Generator().manual_seed(seed + 100)
    w = {k: torch.randn(out[k].shape, generator=gen) for k in STATE + ("conics",)}
    w["penalty"] = torch.randn(4, generator=gen)
    loss = sum((w[k] * out[k]).sum() for k in STATE + ("conics",)) + (w["penalty"] * penalty).sum()

    sd = {k: v for k, v in net.state_dict().items() if k.startswith(KEPT) and not k.startswith("input_transform")}
    params = {k: p for k, p in net.named_parameters() if k in sd and p.requires_grad}
    grads = torch.autograd.grad(loss, list(params.values()) + [net.t_params], retain_graph=True)
    named = dict(zip(list(params) + ["t_params"], grads[:-1] + (grads[-1][0],)))
    hook = net.t_params.register_hook(torch.zeros_like)          # the state's gradient through the update alone
    named.update(zip(STATE, torch.autograd.grad(loss, [state_in[k] for k in STATE])))
    hook.remove()

    arrays = {"t_params": net.t_params[0], "boundary_mask": mask, "global_features": net.global_features[0],
              "neighbor_features": torch.stack([lgf[0, :, (h + 1) * L:(h + 2) * L] for h in range(model_pn.ATTENTION_HEADS)]),
              "local_global_features": lgf[0], "deltas": torch.cat(list(slices.values()), dim=-1), "penalty": penalty,
              "wrap": torch.tensor([-1.0, 1.0] if problem == model_pn.Problem.NAVIER_STOKES else [])}
    arrays.update(slices)
    arrays.update({"sd/" + k: v for k, v in sd.items()})
    arrays.update({"in/" + k: v for k, v in state_in.items()})
    arrays.update({"out/" + k: v for k, v in out.items()})
    arrays.update({"w/" + k: v for k, v in w.items()})
    arrays.update({"grad/" + k: v for k, v in named.items()})
    arrays = {k: v.detach().numpy() for k, v in arrays.items()}
    assert all(a.dtype == np.float64 for k, a in arrays.items() if k != "boundary_mask"), "not float64 throughout"
    return arrays


def main():
    install()
    torch.set_default_dtype(torch.float64)
    out = os.path.join(ROOT, "tests", "golden", "model_pn_step")
    os.makedirs(out, exist_ok=True)
    with trace.CudaToCpu():
        for name, n_lattice, n_cloud, seed in (("DIFFUSION", 7, None, 11), ("NAVIER_STOKES", 12, 117, 14)):
            arrays = record(name, n_lattice, n_cloud, seed)
            path = os.path.join(out, f"{name.lower()}.npz")
            np.savez_compressed(path, **arrays)
            N = arrays["in/means"].shape[0]
            print(f"{path}: N = {N}, {len(arrays)} arrays, {os.path.getsize(path) / 1e3:.0f} kB, "
                  f"deltas up to {np.abs(arrays['deltas']).max():.3g}, {int((~arrays['boundary_mask']).sum())} boundary rows")


if __name__ == "__main__":
    main()
