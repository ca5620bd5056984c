#!/usr/bin/env python3
"""Refinement, one Model.forward(split=True) worth of it, two ways in one process:

  (a) the reference's lines restated in stock torch: the prune by boolean indexing (model_pn.py:703-714), Model.split
      (:578-605: indices.sum().item(), torch.linalg.eig, gather, repeat_interleave, cat), boundaries / boundary_mask
      with them, then build_covariances;
  (b) pigs_amd.refine.split_gaussians twice (prune, split), boundaries / boundary_mask through source / child, then
      build_covariances ("Refinement").

Sizes N = 1 600 (the model's) and 65 536; 5 % pruned, 2 % of the rest split (the reference's 0.98 quantile).  The legs
alternate after a warm-up.  Timed with the HOST clock around work that ends in a synchronise: what (b) saves is mostly
host waits, which device events do not see.  Prints medians and p10-p90 and one JSON line.

    python tools/bench_refine.py [--reps 50] [--warmup 5]      # leg (a) can take 0.2 s per call: torch.linalg.eig
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_refine.py --reps 5 --warmup 2     # kernel times
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

from pigs_amd import refine  # noqa: E402
from pigs_amd.covariances import build_covariances, build_full_covariances  # noqa: E402


def inputs(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    means = (2 * torch.rand((N, 2), generator=g) - 1).cuda()
    scaling = torch.exp(torch.rand((N, 2), generator=g) * (np.log(0.5) - np.log(1e-4)) + np.log(1e-4)).cuda()
    transforms = torch.randn((N, 1), generator=g).cuda()
    u = torch.randn((N, 2), generator=g).cuda()
    keep = (torch.rand(N, generator=g) >= 0.05).cuda()
    split_of_kept = (torch.rand(int(keep.sum()), generator=g) < 0.02).cuda()       # a mask over the pruned arrays
    boundary_mask = torch.ones((N, 1), dtype=torch.bool, device="cuda")
    boundaries = torch.zeros((N, 1), device="cuda")
    return means, scaling, transforms, u, keep, split_of_kept, boundaries, boundary_mask


def leg_torch(means, scaling, transforms, u, keep, indices, boundaries, boundary_mask):
    # :705-714
    u, means, scaling, transforms = u[keep], means[keep], scaling[keep], transforms[keep]
    boundary_mask, boundaries = boundary_mask[keep], boundaries[keep]
    full, _ = build_full_covariances(scaling, transforms)
    # :578-605
    n = indices.sum().item()
    if n:
        with torch.no_grad():
            eigvals, eigvecs = torch.linalg.eig(full[indices])
            eigvals, max_idx = torch.max(eigvals.real.abs(), dim=-1, keepdim=True)
            eigvecs = eigvals.unsqueeze(-1) * torch.gather(eigvecs.real.transpose(-1, -2), 1, max_idx.unsqueeze(-1).expand(n, 1, 2))
            displacements = torch.cat((-eigvecs, eigvecs), dim=1)
        split_means = (means[indices].reshape(n, 1, 2) + displacements).reshape(-1, 2)
        split_scaling = scaling[indices].repeat_interleave(2, 0)
        split_transforms = transforms[indices].repeat_interleave(2, 0)
        split_u = u[indices].repeat_interleave(2, 0) / 2.0
        n = split_means.shape[0]
        means = torch.cat((means[~indices], split_means), dim=0)
        scaling = torch.cat((scaling[~indices], split_scaling), dim=0)
        transforms = torch.cat((transforms[~indices], split_transforms), dim=0)
        u = torch.cat((u[~indices], split_u), dim=0)
        boundaries = torch.cat((boundaries[~indices], torch.zeros((n, 1), device="cuda")), dim=0)
        boundary_mask = torch.cat((boundary_mask[~indices], torch.ones((n, 1), dtype=torch.bool, device="cuda")), dim=0)
    cov, con = build_covariances(scaling, transforms)
    return means, scaling, transforms, u, boundaries, boundary_mask, cov, con


def leg_hip(means, scaling, transforms, u, keep, indices, boundaries, boundary_mask):
    p = refine.split_gaussians(means, scaling, transforms, u, None, keep)
    boundary_mask, boundaries = boundary_mask.index_select(0, p.source), boundaries.index_select(0, p.source)
    r = refine.split_gaussians(p.means, p.scaling, p.transforms, p.values, indices)
    child = (r.child >= 0)[:, None]
    boundaries = torch.where(child, torch.zeros_like(boundaries[:1]), boundaries.index_select(0, r.source))
    boundary_mask = torch.where(child, torch.ones_like(boundary_mask[:1]), boundary_mask.index_select(0, r.source))
    cov, con = build_covariances(r.scaling, r.transforms)
    return r.means, r.scaling, r.transforms, r.values, boundaries, boundary_mask, cov, con


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    args = ap.parse_args()
    result = {"tool": "bench_refine", "reps": args.reps, "sizes": {}}
    print(f"{'N':>7} {'leg':<28} {'median us':>10} {'p10':>9} {'p90':>9}")
    for N in args.sizes:
        data = inputs(N)
        legs = (("a: torch lines (eig, cat)", leg_torch), ("b: split_gaussians", leg_hip))
        with torch.no_grad():
            outs = [leg(*data) for _, leg in legs]
            assert all(x.shape == y.shape for x, y in zip(*outs))
            assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][3], outs[1][3])     # scaling, u
            times = {name: [] for name, _ in legs}
            for it in range(args.warmup + args.reps):
                for name, leg in legs:                 # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    leg(*data)
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e6)
        result["sizes"][N] = {}
        for name, _ in legs:
            p10, med, p90 = np.percentile(times[name], [10, 50, 90])
            result["sizes"][N][name[0]] = {"median_us": round(med, 1), "p10_us": round(p10, 1), "p90_us": round(p90, 1)}
            print(f"{N:>7} {name:<28} {med:>10.1f} {p10:>9.1f} {p90:>9.1f}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
