#!/usr/bin/env python3
"""The split criterion of Model.forward(split=True), two ways in one process:

  (a) the reference's lines model_pn.py:716-754 restated in stock torch over this sampler: three preprocess /
      sample_gaussians passes, min, max, the element-wise chain, torch.quantile, compare, any, multiply;
  (b) pigs_amd.refine.split_criterion: two passes (the density rides as one more channel where it can) and split_mask.

And the quantile rule alone, from the three sampled fields: the torch lines :733-754 against split_mask.

Sizes n = 1 600 with c = 2 (the model's) and n = 65 536 with c = 1, jittered lattices with widths of about 1.3
spacings.  The legs alternate after a warm-up.  Timed with the HOST clock around work that ends in a synchronise.
Prints medians and p10-p90 and one JSON line.

    python tools/bench_criterion.py [--reps 50] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_criterion.py --reps 5 --warmup 2     # kernel times
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pigs_amd.build import ensure_built  # noqa: E402

ensure_built()      # before anything touches the GPU

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pigs_amd import GaussianSampler, refine  # noqa: E402
from pigs_amd.covariances import build_covariances  # noqa: E402


def inputs(n, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    grid = int(round(n ** 0.5))
    assert grid * grid == n, "n must be a square: the scene is a lattice"
    h = 2.0 / grid
    centre = -1.0 + h * (torch.arange(grid) + 0.5)
    means = torch.stack(torch.meshgrid(centre, centre, indexing="ij"), -1).reshape(n, 2)
    means = means + (torch.rand((n, 2), generator=g) - 0.5) * 0.5 * h
    scaling = (1.3 * h * torch.exp(0.3 * torch.randn((n, 2), generator=g))) ** 2
    transforms = 0.5 * torch.randn((n, 1), generator=g)
    values = torch.randn((n, c), generator=g)
    prev_means = means + 0.1 * h * torch.randn((n, 2), generator=g)
    prev_values = values + 0.05 * torch.randn((n, c), generator=g)
    boundary_mask = torch.rand((n, 1), generator=g) < 0.9
    means, scaling, transforms, values, prev_means, prev_values, boundary_mask = (
        t.cuda() for t in (means, scaling, transforms, values, prev_means, prev_values, boundary_mask))
    cov, con = build_covariances(scaling, transforms)
    return means, values, cov, con, prev_means, prev_values, cov, con, boundary_mask


def torch_rule(sample_u, prev_sample_u, density, boundary_mask):
    # :733, :745, :750-754
    density = 1.0 - (density - density.min()) / density.max()
    ut = (sample_u - prev_sample_u) ** 2
    metric = ut * density
    quantile = torch.quantile(metric, 0.98)
    return ((metric > quantile).any(-1, keepdim=True) * boundary_mask).squeeze(-1)


def leg_torch(sampler, means, u, cov, con, prev_means, prev_u, prev_cov, prev_con, boundary_mask):
    # :717-737
    n = means.shape[0]
    sampler.preprocess(means, u, cov, con, means)
    sample_u = sampler.sample_gaussians()
    ones = torch.ones((n, 1), device="cuda")
    sampler.preprocess(means, ones, cov, con, means)
    density = sampler.sample_gaussians()
    sampler.preprocess(prev_means, prev_u, prev_cov, prev_con, means)
    prev_sample_u = sampler.sample_gaussians()
    return torch_rule(sample_u, prev_sample_u, density, boundary_mask)


def leg_hip(sampler, *data):
    return refine.split_criterion(sampler, *data)


def timed(legs, reps, warmup):
    times = {name: [] for name, _ in legs}
    for it in range(warmup + reps):
        for name, leg in legs:                 # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e6)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 2, 65536, 1], help="pairs n c")
    args = ap.parse_args()
    result = {"tool": "bench_criterion", "reps": args.reps, "sizes": {}}
    print(f"{'n':>7} {'c':>2} {'leg':<40} {'median us':>10} {'p10':>9} {'p90':>9}")
    sampler = GaussianSampler(False)
    for n, c in zip(args.sizes[::2], args.sizes[1::2]):
        data = inputs(n, c)
        with torch.no_grad():
            sampler.preprocess(data[0], torch.cat((data[1], torch.ones((n, 1), device="cuda")), -1), data[2], data[3], data[0])
            both = sampler.sample_gaussians()
            sampler.preprocess(*data[4:8], data[0])
            fields = (both[:, :c].contiguous(), sampler.sample_gaussians(), both[:, c:].contiguous(), data[8])
            whole = (("a: torch lines :716-754", lambda: leg_torch(sampler, *data)),
                     ("b: split_criterion", lambda: leg_hip(sampler, *data)))
            rule = (("rule a: torch lines :733-754", lambda: torch_rule(*fields)),
                    ("rule b: split_mask", lambda: refine.split_mask(*fields)))
            differ = int((whole[0][1]() != whole[1][1]()).sum()), int((rule[0][1]() != rule[1][1]()).sum())
            assert differ[0] <= 2 and differ[1] == 0, differ       # the whole: rows at the quantile may round apart
            times = {**timed(whole, args.reps, args.warmup), **timed(rule, args.reps, args.warmup)}
        key = f"{n}x{c}"
        result["sizes"][key] = {"mask_rows_that_differ": differ[0]}
        for name in times:
            p10, med, p90 = np.percentile(times[name], [10, 50, 90])
            result["sizes"][key][name.split(":")[0]] = {"median_us": round(med, 1), "p10_us": round(p10, 1), "p90_us": round(p90, 1)}
            print(f"{n:>7} {c:>2} {name:<40} {med:>10.1f} {p10:>9.1f} {p90:>9.1f}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
