#!/usr/bin/env python3
"""The reference's InputTransform on one recorded time step, in float64, for tests/test_input_transform*.py.

TEST INFRASTRUCTURE, build container only: like tools/gen_model_step.py (whose stand-in sampler, construction and seeds
it reuses, so that the step is the SAME step) it imports the reference's model_pn.py read-only and never copies from it.
It drives ``sample`` -> ``forward(t, dt, False)`` once for

    DIFFUSION       c = 1, pde_size = 1, N = 149
    NAVIER_STOKES   c = 2, pde_size = 1, N = 117

and records what ``dynamics_network.input_transform`` (model_pn.py:51-152, called at :237-249) saw and made:

  * ``sd/<key>``: the ``input_transform.*`` entries of dynamics_network's state_dict, under the keys of the module itself
    (``latent_net.layers.0.weight`` ...),
  * ``in/<name>``: its eight inputs (means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde),
  * ``latent`` [16], ``T/<name>``: the five matrices (transform, transform_u, transform_ux, transform_uxx, transform_pde),
  * ``t_params`` [N, in_dims] (asserted equal to the one in tests/golden/model_pn_step/ to 1e-12),
  * ``w``: seeded weights of a linear functional of t_params, and ``grad/<name>``: its gradient with respect to every
    parameter (``grad/sd/<key>``) and to means, full_covariances and u.

    python tools/gen_input_transform.py       # writes tests/golden/input_transform/{diffusion,navier_stokes}.npz
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_model_step as step         # noqa: E402
import gen_model_trace as trace       # noqa: E402

INPUTS = ("means", "full_covariances", "u", "boundaries", "sample_u", "sample_ux", "sample_uxx", "sample_pde")
MATRICES = ("transform", "transform_u", "transform_ux", "transform_uxx", "transform_pde")


def record(problem_name, n_lattice, n_cloud, seed):
    import model_pn
    # the construction of gen_model_step.record, draw for draw
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
    for name in step.STATE:
        setattr(model, name, getattr(model, name).detach().clone().requires_grad_(True))

    module = model.dynamics_network.input_transform
    seen = {}

    def leaves(_, args):       # the three differentiable inputs as leaves of their own: the values do not change
        args = list(args)
        for k in range(3):
            args[k] = args[k].detach().clone().requires_grad_(True)
        seen.update(zip(INPUTS, args))
        return tuple(args)

    def latent(_, __, out):
        seen["latent"] = out.mean(-1)[0]
    hooks = [module.register_forward_pre_hook(leaves), module.latent_net.register_forward_hook(latent)]
    model.forward(0.0, 1.0, False)
    for h in hooks:
        h.remove()

    net = model.dynamics_network
    t_params = net.t_params[0]
    assert t_params.dtype == torch.float64
    gen = torch.Generator().manual_seed(seed + 200)
    w = torch.randn(t_params.shape, generator=gen)
    params = dict(module.named_parameters())
    wrt = list(params.values()) + [seen[k] for k in INPUTS[:3]]
    grads = torch.autograd.grad((w * t_params).sum(), wrt)

    arrays = {"t_params": t_params, "latent": seen["latent"], "w": w}
    arrays.update({"sd/" + k: v for k, v in module.state_dict().items()})
    arrays.update({"in/" + k: (v.reshape(-1, 1) if k == "boundaries" else v) for k, v in seen.items() if k in INPUTS})
    arrays.update({"T/" + k: getattr(module, k)[0] for k in MATRICES})
    arrays.update({"grad/sd/" + k: g for k, g in zip(params, grads)})
    arrays.update({"grad/" + k: g for k, g in zip(INPUTS[:3], grads[len(params):])})
    arrays = {k: v.detach().to(torch.float64).numpy() for k, v in arrays.items()}
    return arrays


def main():
    step.install()
    torch.set_default_dtype(torch.float64)
    out = os.path.join(ROOT, "tests", "golden", "input_transform")
    os.makedirs(out, exist_ok=True)
    with trace.CudaToCpu():
        for name, n_lattice, n_cloud, seed in (("DIFFUSION", 7, None, 11), ("NAVIER_STOKES", 12, 117, 14)):
            arrays = record(name, n_lattice, n_cloud, seed)
            recorded = np.load(os.path.join(ROOT, "tests", "golden", "model_pn_step", f"{name.lower()}.npz"))["t_params"]
            worst = np.abs(arrays["t_params"] - recorded).max()
            assert worst <= 1e-12, f"{name}: t_params differs from the recorded step by {worst:.3g}"
            path = os.path.join(out, f"{name.lower()}.npz")
            np.savez_compressed(path, **arrays)
            N, c = arrays["in/u"].shape
            print(f"{path}: N = {N}, c = {c}, pde_size = {arrays['in/sample_pde'].shape[1]}, {len(arrays)} arrays, "
                  f"{os.path.getsize(path) / 1e3:.0f} kB, t_params within {worst:.3g} of the recorded step")


if __name__ == "__main__":
    main()
