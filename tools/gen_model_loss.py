#!/usr/bin/env python3
"""One recorded ``Model.compute_loss`` of the reference's PINN model per problem and integration rule, in float64, for
tests/test_model_loss.py.

TEST INFRASTRUCTURE, build container only: like tools/gen_model_trace.py (whose ``install()``, device rewriting mode,
recording sampler over the dense float64 oracle and boundary points it reuses) it imports the reference's model_pn.py
read-only and never copies from it.  Under ``torch.set_default_dtype(torch.float64)`` it constructs ``model_pn.Model``
for DIFFUSION, BURGERS (c = 1, an 11 x 11 lattice made random by ``randomize`` behind 100 boundary Gaussians), WAVE
(c = 2, the same 100 boundary Gaussians) and NAVIER_STOKES (c = 2, no boundary Gaussians), the last two on a seeded
cloud of 121 Gaussians through ``set_initial_params`` as ``gen_model_trace.run`` does, once per ``IntegrationRule`` from
the SAME seed: 121 free Gaussians (a multiple of neither 16 nor 64), M = 100 collocation points, 60 boundary points,
dt = 0.25.  Per scene it drives, as the training loop does (main_pn.py:99-232),

    sample -> forward / compute_loss / backward (warm) -> clear / sample / detach
           -> forward(t, dt, False) -> compute_loss -> (pde_loss + bc_loss).backward()        the recorded iteration

with t > 0 (no initial loss) and no optimiser step; the previous level is then a constant, and the tool asserts that no
gradient arrived at its ``preprocess`` calls.  Recorded, in float64:

  * ``prev/*`` and ``cur/*``: means, values, conics handed to ``preprocess`` for the two levels (after the boundary mask),
  * ``samples``, ``bc_samples``, ``time_samples``, ``dt``, ``nu`` (NaN where the model has none), ``pde_weight``,
    ``bc_weight``, ``rules``, and ``u_now`` / ``u_prev`` (``w_now`` / ``w_prev`` for NAVIER_STOKES): the model's own
    ``u_samples[-1]`` / ``[-2]`` (``w_samples``), the two terms of its ``ut`` (``wt``),
  * per rule ``<RULE>/rhs`` (the return value of ``model.pde_rhs`` inside compute_loss, captured by a wrapper at run
    time), ``<RULE>/pde_loss`` and ``<RULE>/bc_loss`` as compute_loss returns them (weights included), and
    ``<RULE>/grad_pde/*`` / ``<RULE>/grad_bc/*``: the gradients that left the current level's two ``preprocess`` calls
    (collocation points / boundary points) towards means, values and conics (absent where none arrived: NAVIER_STOKES
    has no boundary loss).

NAVIER_STOKES under FORWARD and BACKWARD: the reference defines wx / wxx under TRAPEZOID only (model_pn.py:801-805),
so its compute_loss raises under the other two rules.  Those two scenes are recorded under TRAPEZOID with
``time_samples`` all 0.0 (FORWARD) and all 1.0 (BACKWARD), what the two rules select for u, ux and uxx (:806-813);
``time_samples`` in the file is the random draw of the TRAPEZOID scene.

    python tools/gen_model_loss.py            # writes tests/golden/model_pn_loss/{diffusion,burgers,wave,navier_stokes}.npz

(a directory of their own: tests/conftest.py hands every *.npz directly under tests/golden/ to the sampler's parity
tests.)  np.savez_compressed writes no time stamps: a second run gives the same bytes.
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

import gen_model_trace as trace       # noqa: E402

PROBLEMS = (("DIFFUSION", 21), ("BURGERS", 22), ("WAVE", 23), ("NAVIER_STOKES", 24))
RULES = ("TRAPEZOID", "FORWARD", "BACKWARD")
N_LATTICE, M, M_BC, DT = 11, 100, 60, 0.25
INPUTS = ("means", "values", "conics")


def record(problem_name, rule_name, seed):
    import model_pn
    trace.TRACE.clear()
    torch.manual_seed(seed)
    np.random.seed(seed)
    problem = getattr(model_pn.Problem, problem_name)
    scale, d = 1.0, 2
    ns = problem == model_pn.Problem.NAVIER_STOKES
    rule = model_pn.IntegrationRule.TRAPEZOID if ns else getattr(model_pn.IntegrationRule, rule_name)
    model = model_pn.Model(problem, rule, N_LATTICE, N_LATTICE, d, scale)
    model.train()
    time_samples = torch.rand(M)
    samples = (torch.rand((M, d)) * 2.0 - 1.0) * scale
    bc_samples = trace.boundary_points(M_BC, scale)
    if problem in (model_pn.Problem.NAVIER_STOKES, model_pn.Problem.WAVE):      # gen_model_trace.run has the reasons
        n = N_LATTICE * N_LATTICE
        model.set_initial_params((torch.rand((n, d)) * 2.0 - 1.0) * scale, torch.randn((n, 2)) * 0.2,
                                 torch.exp(torch.randn((n, d)) * 0.3 - 4.0) * scale, torch.tanh(torch.randn((n, 1)) * 0.3))
    else:
        model.randomize(N_LATTICE)
    used = time_samples
    if ns and rule_name != "TRAPEZOID":
        used = torch.full_like(time_samples, 0.0 if rule_name == "FORWARD" else 1.0)

    returned = []
    inner = model.pde_rhs
    model.pde_rhs = lambda *a, **k: (returned.append(inner(*a, **k)), returned[-1])[1]

    def total(parts):
        return parts[0] + parts[1]
    model.sample(samples, bc_samples)
    model.forward(DT, DT, False)
    total(model.compute_loss(DT, DT, samples, used, bc_samples)).backward()
    model.clear()
    model.sample(samples, bc_samples)
    model.detach()
    prev = trace.TRACE[-2:]
    model.forward(2 * DT, DT, False)
    parts = model.compute_loss(2 * DT, DT, samples, used, bc_samples)
    cur = trace.TRACE[-2:]
    total(parts).backward()

    for level in (prev, cur):
        assert torch.equal(level[0]["samples"], samples) and torch.equal(level[1]["samples"], bc_samples)
        assert all(torch.equal(level[0][k], level[1][k]) for k in INPUTS)
    assert not any(k in r for r in prev for k in ("gmeans", "gvalues", "gconics")), "a gradient reached the previous level"
    assert "gmeans" in cur[0] and ("gmeans" in cur[1]) == (not ns)
    N = cur[0]["means"].shape[0]
    assert N == N_LATTICE * N_LATTICE and N % 16 and N % 64 and 100 <= N <= 150

    shared = {"samples": samples, "bc_samples": bc_samples, "time_samples": time_samples, "dt": torch.tensor(DT),
              "nu": torch.tensor(float(getattr(model, "nu", float("nan")))), "pde_weight": torch.tensor(float(model.pde_weight)),
              "bc_weight": torch.tensor(float(model.bc_weight))}
    for name, level in (("prev", prev), ("cur", cur)):
        shared.update({f"{name}/{k}": level[0][k] for k in INPUTS})
    if ns:
        shared.update(w_now=model.w_samples[-1], w_prev=model.w_samples[-2])
    else:
        shared.update(u_now=model.u_samples[-1], u_prev=model.u_samples[-2])
    own = {"rhs": returned[-1], "pde_loss": parts[0].reshape(()), "bc_loss": parts[1].reshape(())}
    for name, r in (("grad_pde", cur[0]), ("grad_bc", cur[1])):
        own.update({f"{name}/{k}": r["g" + k] for k in INPUTS if "g" + k in r})

    def arrays(t):
        out = {k: v.detach().numpy().copy() for k, v in t.items()}
        assert all(a.dtype == np.float64 for a in out.values()), "not float64 throughout"
        return out
    return arrays(shared), arrays(own)


def main():
    trace.install()
    torch.set_default_dtype(torch.float64)
    out = os.path.join(ROOT, "tests", "golden", "model_pn_loss")
    os.makedirs(out, exist_ok=True)
    with trace.CudaToCpu():
        for name, seed in PROBLEMS:
            arrays = {"rules": np.array(RULES)}
            for rule in RULES:
                shared, own = record(name, rule, seed)
                for k, v in shared.items():      # the same seeded state under the three rules of one problem
                    assert np.array_equal(arrays.setdefault(k, v), v, equal_nan=True), (name, rule, k)
                arrays.update({f"{rule}/{k}": v for k, v in own.items()})
            path = os.path.join(out, f"{name.lower()}.npz")
            np.savez_compressed(path, **arrays)
            moved = np.abs(arrays["cur/means"] - arrays["prev/means"]).max()
            print(f"{path}: N = {arrays['cur/means'].shape[0]}, {len(arrays)} arrays, {os.path.getsize(path) / 1e3:.0f} kB, "
                  f"means moved by up to {moved:.3g}, pde_loss "
                  + ", ".join(f"{r} {float(arrays[r + '/pde_loss']):.4g}" for r in RULES))


if __name__ == "__main__":
    main()
