#!/usr/bin/env python3
"""Recorded ``Model.compute_loss`` of the reference's TEST problem, in float64, for tests/test_state_loss.py and
tests/test_state_loss_gpu.py.

TEST INFRASTRUCTURE, build container only: like tools/gen_model_loss.py it reuses ``install()`` and ``CudaToCpu`` of
tools/gen_model_trace.py, imports the reference's model_pn.py read-only and copies nothing from it.  Under
``torch.set_default_dtype(torch.float64)`` it constructs ``model_pn.Model(Problem.TEST, IntegrationRule.TRAPEZOID, 9, 9,
2, 1.0)``: 56 Gaussians, 50 boundary rows in front and 6 free ones, c = 1.  ``randomize`` gives the free rows one common
height and the network's deltas then spread them, so which of the three sets of model_pn.py:855-876 (y < -0.8, y > 0.8,
|y| < 0.8) a scene fills depends on the seed.  The tool walks seeds from FIRST_SEED upwards and keeps the first scene of
each kind, until it holds an all-MID, an all-LOW, an all-HIGH and MIXED_SCENES mixed scenes, and ASSERTS that it does.

Per scene it drives ``randomize -> sample -> forward(t, dt, False) -> compute_loss`` with t = dt = 0.25 and records

  * ``prev_means``, ``prev_u``: the state before the step; ``means``, ``u``: the new state; ``boundary_mask`` [N] bool;
  * ``deltas`` [N, 6]: the network's packed output assembled from the model's four slices (dmeans, dscaling,
    dtransforms, du);
  * ``pde_loss``, ``bc_loss``, ``conservation_loss`` as compute_loss returns them, the model's weights included;
  * ``grad_dmeans``, ``grad_dscaling``, ``grad_dtransforms``, ``grad_du``: the gradients of the sum of the three with
    respect to the model's four delta tensors (``retain_grad``), and ``grad_means``, ``grad_u``: the gradients that arrive
    at the new state, which are the gradients towards the previous ``means`` and ``u`` along ``prev + delta * mask``
    (the path through the network's inputs is not part of them);
  * ``counts``: |LOW|, |HIGH|, |MID| of the free rows, and ``seed``.

and once the model's weights (``weights``, in the order of WEIGHTS).

    python tools/gen_state_loss.py            # writes tests/golden/model_pn_state_loss/test.npz

(a directory of its own: tests/conftest.py hands every *.npz directly under tests/golden/ to the sampler's parity
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

N_LATTICE, M, M_BC, DT = 9, 64, 32, 0.25
FIRST_SEED, LAST_SEED, MIXED_SCENES = 40, 400, 2
WEIGHTS = ("pde_weight", "bc_weight", "conservation_weight", "dmean_weight", "du_weight", "dscale_weight",
           "dtransform_weight")
WALL = 0.8


def record(seed):
    import model_pn
    trace.TRACE.clear()
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = model_pn.Model(model_pn.Problem.TEST, model_pn.IntegrationRule.TRAPEZOID, N_LATTICE, N_LATTICE, 2, 1.0)
    model.train()
    time_samples = torch.rand(M)
    samples = torch.rand((M, 2)) * 2.0 - 1.0
    bc_samples = trace.boundary_points(M_BC, 1.0)
    model.randomize(N_LATTICE)
    model.sample(samples, bc_samples)
    prev_means, prev_u = model.means.detach().clone(), model.u.detach().clone()
    model.forward(DT, DT, False)
    blocks = (model.dmeans, model.dscaling, model.dtransforms, model.du)
    state = (model.means, model.u)
    for t in blocks + state:
        t.retain_grad()
    parts = model.compute_loss(DT, DT, samples, time_samples, bc_samples)
    (parts[0] + parts[1] + parts[2]).backward()

    mask = model.boundary_mask.reshape(-1)
    N = mask.shape[0]
    assert all(b.shape[0] == N and b.dim() == 2 for b in blocks) and model.u.shape == (N, 1)
    assert torch.equal(model.prev_means, prev_means) and torch.equal(model.prev_u, prev_u)
    y = model.means.detach()[mask, 1]
    counts = np.array([int((y < -WALL).sum()), int((y > WALL).sum()), int((y.abs() < WALL).sum())])
    assert counts.sum() == int(mask.sum()), "a free row sits exactly on a wall"
    out = {"prev_means": prev_means, "prev_u": prev_u, "means": model.means, "u": model.u,
           "deltas": torch.cat(blocks, dim=-1), "pde_loss": parts[0].reshape(()), "bc_loss": parts[1].reshape(()),
           "conservation_loss": parts[2].reshape(()), "grad_means": model.means.grad, "grad_u": model.u.grad}
    out.update({"grad_" + k: b.grad for k, b in zip(("dmeans", "dscaling", "dtransforms", "du"), blocks)})
    out = {k: v.detach().numpy().copy() for k, v in out.items()}
    assert all(a.dtype == np.float64 for a in out.values()), "not float64 throughout"
    assert out["deltas"].shape == (N, 6)
    out.update(boundary_mask=mask.numpy().copy(), counts=counts, seed=np.array(seed))
    weights = np.array([float(getattr(model, k)) for k in WEIGHTS])
    return out, weights


def kind_of(counts):
    low, high, mid = (int(v) for v in counts)
    if low + high + mid in (low, high, mid):
        return "low" if low else ("high" if high else "mid")
    return "mixed"


def main():
    trace.install()
    torch.set_default_dtype(torch.float64)
    out = os.path.join(ROOT, "tests", "golden", "model_pn_state_loss")
    os.makedirs(out, exist_ok=True)
    wanted = {"mid": 1, "low": 1, "high": 1, "mixed": MIXED_SCENES}
    scenes, weights = [], None
    with trace.CudaToCpu():
        for seed in range(FIRST_SEED, LAST_SEED):
            if not any(wanted.values()):
                break
            scene, w = record(seed)
            assert weights is None or np.array_equal(weights, w)
            weights = w
            kind = kind_of(scene["counts"])
            if wanted[kind]:
                wanted[kind] -= 1
                scenes.append((kind, scene))
    kinds = [k for k, _ in scenes]
    assert not any(wanted.values()), f"seeds {FIRST_SEED}..{LAST_SEED - 1} do not cover {wanted}"
    assert {"mid", "low", "high", "mixed"} <= set(kinds)
    arrays = {"weights": weights, "weight_names": np.array(WEIGHTS), "kinds": np.array(kinds)}
    for k, (_, scene) in enumerate(scenes):
        arrays.update({f"s{k}/{name}": v for name, v in scene.items()})
    path = os.path.join(out, "test.npz")
    np.savez_compressed(path, **arrays)
    for k, (kind, scene) in enumerate(scenes):
        print(f"scene {k}: seed {int(scene['seed'])}, {kind}, LOW / HIGH / MID = {scene['counts'].tolist()}, "
              f"N = {scene['means'].shape[0]}, free {int(scene['boundary_mask'].sum())}, pde {float(scene['pde_loss']):.4g}, "
              f"bc {float(scene['bc_loss']):.4g}, conservation {float(scene['conservation_loss']):.4g}")
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
