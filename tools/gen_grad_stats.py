#!/usr/bin/env python3
"""Gradient-statistics fixtures for the MLP-free loops from the REFERENCE's own sampling functions.

TEST INFRASTRUCTURE, build container only (imports the reference's gaussians.py read-only through tools/gen_loss_curve.py; nothing is copied).
The two loops live in the test modules -- tests/test_optim_stats.py::loop_2d (tests/test_training_gpu.py::run_loop
restated) and tests/test_optim_1d.py::loop_1d (the Burgers loop of the reference's test_no_mlp_1d.py:97-153) -- and are
driven here through the reference's ``gaussians.sample_gaussians`` / ``gaussian_derivative`` / ``gaussian_derivative2``
with the reference's parameterisation, torch.optim.Adam (lr 1e-2) and the four statistic lines of
test_no_mlp.py:149-155 / test_no_mlp_1d.py:156-162 after every backward, from step 0, 30 steps, on the CPU.  Recorded
per loop, in float32 and (suffix ``_f64``, for information) float64: the losses, mean_grad, mean_grad_norm, scale_grad,
scale_grad_norm and the last step's two gradients, to tests/golden/grad_stats/no_mlp_2d.npz and no_mlp_1d.npz.
The 2-D float32 losses must be those of ref_loss_curve_no_mlp.npz (asserted here within 1e-6 relative).

    MPLBACKEND=Agg python tools/gen_grad_stats.py
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from gen_loss_curve import ReferenceSampler          # the sampler's surface over the reference's functions, d = 2


class ReferenceSampler1D(ReferenceSampler):
    def preprocess(self, means, values, covariances, conics, samples):
        self.args = (means, conics.reshape(-1, 1, 1), values, samples)


def record(chain, losses, out, tag):
    out["losses" + tag] = losses
    for k, a in chain.read_stats().items():
        out[k + tag] = a if tag else a.astype(np.float32)


def spread(out, names):
    worst = max(float(np.abs(out[k] - out[k + "_f64"]).max()) / float(np.abs(out[k + "_f64"]).max()) for k in names)
    loss = float((np.abs(out["losses"] - out["losses_f64"]) / np.abs(out["losses_f64"])).max())
    return loss, worst


def main():
    from test_optim_1d import TorchChain1D, init_1d, loop_1d
    from test_optim_stats import STATS, TorchChain, init_2d, loop_2d
    torch.set_num_threads(8)
    device, steps = torch.device("cpu"), 30
    golden = os.path.join(ROOT, "tests", "golden")

    out = {"steps": np.array(steps)}
    for dtype, tag in ((torch.float32, ""), (torch.float64, "_f64")):
        params, g = init_2d(device, dtype)
        chain = TorchChain(*params, lr=1e-2, scale=2.5)
        record(chain, loop_2d(chain, g, ReferenceSampler, device, dtype, steps), out, tag)
    ref = np.load(os.path.join(golden, "ref_loss_curve_no_mlp.npz"))["losses"]
    rel = float((np.abs(out["losses"] - ref) / np.abs(ref)).max())
    print("2-D float32 losses vs ref_loss_curve_no_mlp.npz:", rel)
    assert rel <= 1e-6
    print("2-D float32 vs float64 (losses, statistics):", spread(out, STATS))
    np.savez_compressed(os.path.join(golden, "grad_stats", "no_mlp_2d.npz"), **out)

    out = {"steps": np.array(steps)}
    for dtype, tag in ((torch.float32, ""), (torch.float64, "_f64")):
        params, g = init_1d(device, dtype)
        chain = TorchChain1D(*params, lr=1e-2, scale=2.5)
        record(chain, loop_1d(chain, g, ReferenceSampler1D, device, dtype, steps), out, tag)
    print("1-D float32 vs float64 (losses, statistics):", spread(out, STATS))
    print("1-D losses:", out["losses"][:3], "...", out["losses"][-3:])
    np.savez_compressed(os.path.join(golden, "grad_stats", "no_mlp_1d.npz"), **out)


if __name__ == "__main__":
    main()
