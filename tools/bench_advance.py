#!/usr/bin/env python3
"""The model's state update (model_pn.py:270-273, 677-698, 878-882), several ways in one process:

  (a)   the reference's lines in torch, literally: four column slices of the network's output, six detach().clone(), the
        masked update, the wrap through two boolean-index writes, pigs_amd.covariances.build_full_covariances +
        flatten_covariances, four mean(x[mask] ** 2).  The boolean indexings wait for the host: eager only.
  (ac)  the same made capturable with what the parent commit offers: ``where`` for the wrap, masked sums over a device
        count for the penalties.  The best composition without the operator, and the one a graph can hold.
  (acg) (ac) inside a graph replay.
  (b)   pigs_amd.advance_gaussians (two launches forward, one backward).
  (bg)  (b) inside a graph replay.

Two tables: the forward alone, and forward + backward from given gradients on means', u', conics, full_covariances and
the penalty towards the state and the UNSLICED deltas leaf [1, N, 5 + c] (so the composition pays its slice backward).
Sizes N = 1 600 and 65 536, c = 1 and 2, float32, a boundary prefix of 50 rows.  The legs alternate after a warm-up; every
figure is taken with the HOST clock around work that ends in a synchronise and with HIP events around the same work.
Prints medians and p10-p90 and one JSON line.

    python tools/bench_advance.py [--reps 200] [--warmup 20] [--sizes 1600 65536] [--channels 1 2]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_advance.py --only b --reps 20 --sizes 1600 --channels 2
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_advance.py --only a --reps 20 --sizes 1600 --channels 2
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

from pigs_amd.advance import advance_gaussians  # noqa: E402
from pigs_amd.covariances import build_full_covariances, flatten_covariances  # noqa: E402

WRAP = (-1.0, 1.0)
BOUNDARY = 50


def problem(N, c, seed=0):
    """state, the network's output [1, N, 5 + c], the mask [N, 1] (True = free), gradients on the five outputs used"""
    g = torch.Generator().manual_seed(seed)
    means = (torch.rand((N, 2), generator=g) * 2 - 1).cuda()
    u = torch.randn((N, c), generator=g).cuda()
    scaling = torch.exp(torch.rand((N, 2), generator=g) * 3.0 - 4.0).cuda()
    transforms = (torch.rand((N, 1), generator=g) * 2.0 - 1.0).cuda()
    deltas = (0.1 * torch.randn((1, N, 5 + c), generator=g)).cuda()
    mask = (torch.arange(N) >= BOUNDARY)[:, None].cuda()
    gouts = tuple(torch.randn(s, generator=g).cuda() for s in ((N, 2), (N, c), (N, 3), (N, 2, 2), (4,)))
    return [means, u, scaling, transforms, deltas], mask, gouts


def reference_lines(means, u, scaling, transforms, deltas, boundary_mask):
    """leg (a)"""
    c = u.shape[1]
    dmeans = deltas[..., :2].squeeze(0)                           # model_pn.py:269-272
    dscaling = deltas[..., 2:4].squeeze(0)
    dtransforms = deltas[..., 4:5].squeeze(0)
    du = deltas[..., -c:].squeeze(0)
    mask = boundary_mask.squeeze()
    prev = [t.detach().clone() for t in (means, u, scaling, transforms)]      # :677-680
    new_means = means + dmeans * boundary_mask                    # :684-687
    new_scaling = scaling * torch.exp(dscaling * boundary_mask)
    new_transforms = transforms + dtransforms * boundary_mask
    new_u = u + du * boundary_mask
    oob = new_means > WRAP[1]                                     # :689-693
    new_means[oob] -= WRAP[1] - WRAP[0]
    oob = new_means < WRAP[0]
    new_means[oob] += WRAP[1] - WRAP[0]
    full_cov, full_con = build_full_covariances(new_scaling, new_transforms)      # :695-698
    cov, con = flatten_covariances(full_cov, full_con)
    prev += [cov.detach().clone(), con.detach().clone()]          # :681-682: the clones of the covariances, one step on
    penalty = torch.stack((torch.mean(dmeans[mask] ** 2), torch.mean(dscaling[mask] ** 2),      # :878-882
                           torch.mean(dtransforms[mask] ** 2), torch.mean(du[mask] ** 2)))
    return (new_means, new_u, con, full_cov, penalty), prev


def capturable_lines(means, u, scaling, transforms, deltas, boundary_mask):
    """leg (ac)"""
    c = u.shape[1]
    dmeans = deltas[..., :2].squeeze(0)
    dscaling = deltas[..., 2:4].squeeze(0)
    dtransforms = deltas[..., 4:5].squeeze(0)
    du = deltas[..., -c:].squeeze(0)
    m = boundary_mask.to(means.dtype)
    prev = [t.detach().clone() for t in (means, u, scaling, transforms)]
    new_means = means + dmeans * m
    new_scaling = scaling * torch.exp(dscaling * m)
    new_transforms = transforms + dtransforms * m
    new_u = u + du * m
    new_means = torch.where(new_means > WRAP[1], new_means - (WRAP[1] - WRAP[0]), new_means)
    new_means = torch.where(new_means < WRAP[0], new_means + (WRAP[1] - WRAP[0]), new_means)
    full_cov, full_con = build_full_covariances(new_scaling, new_transforms)
    cov, con = flatten_covariances(full_cov, full_con)
    prev += [cov.detach().clone(), con.detach().clone()]
    n_free = m.sum()
    penalty = torch.stack([((x * m) ** 2).sum() / (n_free * x.shape[1]) for x in (dmeans, dscaling, dtransforms, du)])
    return (new_means, new_u, con, full_cov, penalty), prev


def operator(means, u, scaling, transforms, deltas, boundary_mask):
    """leg (b): the inputs are the previous state, nothing is cloned"""
    out = advance_gaussians(means, u, scaling, transforms, deltas, boundary_mask, wrap=WRAP)
    return (out.means, out.u, out.conics, out.full_covariances, out.penalty), None


class Leg:
    def __init__(self, fn, N, c, backward):
        self.fn, self.backward = fn, backward
        self.leaves, self.mask, self.gouts = problem(N, c)
        self.result = None

    def make_leaves(self):
        self.leaves = [t.detach().clone().requires_grad_(True) for t in self.leaves]      # the model's forward runs under autograd

    def run(self):
        outs, prev = self.fn(*self.leaves, self.mask)
        if self.backward:
            self.result = torch.autograd.grad(outs, self.leaves, self.gouts)
        else:
            self.result = (outs, prev)

    def graphed(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.make_leaves()
            for _ in range(3):
                self.run()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.run()
        torch.cuda.current_stream().wait_stream(side)
        return self.graph.replay


def measure(legs, reps, warmup):
    """legs: [(name, callable)]; alternating; returns {name: {"host": [...us], "event": [...us]}}"""
    times = {name: {"host": [], "event": []} for name, _ in legs}
    for it in range(warmup + reps):
        for name, run in legs:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            run()
            stop.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name]["host"].append((time.perf_counter() - t0) * 1e6)
                times[name]["event"].append(start.elapsed_time(stop) * 1e3)
    return times


def report(table, N, c, times, result):
    for name, t in times.items():
        row = {}
        for clock in ("host", "event"):
            p10, med, p90 = np.percentile(t[clock], [10, 50, 90])
            row[clock] = {"median_us": round(float(med), 1), "p10_us": round(float(p10), 1), "p90_us": round(float(p90), 1)}
        result.setdefault(table, {}).setdefault(f"N={N},c={c}", {})[name] = row
        h, e = row["host"], row["event"]
        print(f"{table:<8} {N:>6} {c:>2} {name:<40} {h['median_us']:>9.1f} {h['p10_us']:>8.1f} {h['p90_us']:>8.1f}"
              f" {e['median_us']:>9.1f} {e['p10_us']:>8.1f} {e['p90_us']:>8.1f}", flush=True)


LEGS = (("a", "a: the reference's lines", reference_lines, False),
        ("ac", "ac: capturable composition", capturable_lines, False),
        ("acg", "acg: capturable composition, graph replay", capturable_lines, True),
        ("b", "b: advance_gaussians", operator, False),
        ("bg", "bg: advance_gaussians, graph replay", operator, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--only", choices=[k for k, _, _, _ in LEGS], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--tables", nargs="+", default=["forward", "fwd+bwd"], choices=["forward", "fwd+bwd"])
    args = ap.parse_args()
    result = {"tool": "bench_advance", "reps": args.reps, "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
    print(f"{'table':<8} {'N':>6} {'c':>2} {'leg':<40} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} {'p90':>8}   (us)")
    for table in args.tables:
        for N in args.sizes:
            for c in args.channels:
                legs, keep = [], []
                for key, name, fn, graphed in LEGS:
                    if args.only not in (None, key):
                        continue
                    leg = Leg(fn, N, c, backward=table == "fwd+bwd")
                    keep.append(leg)
                    if graphed:
                        legs.append((name, leg.graphed()))
                    else:
                        leg.make_leaves()
                        legs.append((name, leg.run))
                report(table, N, c, measure(legs, args.reps, args.warmup), result)
                del keep
    print(json.dumps(result))


if __name__ == "__main__":
    main()
