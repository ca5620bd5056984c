#!/usr/bin/env python3
"""The TEST problem's state terms (model_pn.py:851-861, 866-876), several ways in one process:

  (a)   the reference's lines in torch, literally: three ``if torch.any(...)`` and the boolean indexings, on the new
        state and the four column slices of the network's output.  They wait for the host: eager only.
  (ac)  the capturable torch composition: ``state_loss_recipe`` of tests/test_state_loss.py (``where`` and masked sums,
        no host decision).  The best composition without the operator, and the one a graph can hold.
  (acg) (ac) inside a graph replay.
  (b)   pigs_amd.state_loss_terms (one launch forward up to 4 096 rows, two above; one backward).
  (bg)  (b) inside a graph replay.

Every leg ends in the same scalar, the eight terms under the TEST problem's weights (pde 10, bc 2, conservation 0.5 x
dmean 4 / du 4), so the backward starts from one number.  Two tables: the forward alone, and forward + backward towards
the new means, the new u and the UNSLICED deltas leaf [1, N, 5 + c].  Sizes N = 56 (the reference's own), 1 600 and
65 536, c = 1, float32, a boundary prefix of 50 rows, heights over all three sets so that (a) takes every branch.  The
legs alternate after a warm-up; every figure is taken with the HOST clock around work that ends in a synchronise and
with HIP events around the same work.  Prints medians and p10-p90 and one JSON line.

    python tools/bench_state_loss.py [--reps 200] [--warmup 20] [--sizes 56 1600 65536]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_state_loss.py --only b --reps 20 --sizes 56
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pigs_amd.build import ensure_built  # noqa: E402

ensure_built()      # before anything touches the GPU

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pigs_amd.state_loss import state_loss_terms  # noqa: E402
from test_state_loss import state_loss_recipe  # noqa: E402

BOUNDARY = 50
PDE, BC, CONSERVATION, DMEAN, DU = 10.0, 2.0, 0.5, 4.0, 4.0      # model_pn.py:312-320
WEIGHTS = (PDE, BC, BC, CONSERVATION * DMEAN, CONSERVATION * DMEAN, CONSERVATION * DMEAN, CONSERVATION * DU, CONSERVATION * DU)


def problem(N, c, seed=0):
    """the new means and u, the network's output [1, N, 5 + c], the mask [N, 1] (True = free)"""
    g = torch.Generator().manual_seed(seed)
    means = torch.stack((torch.rand(N, generator=g) * 2 - 1, torch.rand(N, generator=g) * 2.2 - 1.1), -1).cuda()
    u = torch.randn((N, c), generator=g).cuda()
    deltas = (0.1 * torch.randn((1, N, 5 + c), generator=g)).cuda()
    mask = (torch.arange(N) >= BOUNDARY)[:, None].cuda()
    return [means, u, deltas], mask


def reference_lines(means, u, deltas, boundary_mask, weights):
    """leg (a)"""
    c = u.shape[1]
    dmeans = deltas[..., :2].squeeze(0)                           # model_pn.py:269, 272
    du = deltas[..., -c:].squeeze(0)
    mask = boundary_mask.squeeze()
    pde_loss = torch.mean((dmeans[mask, 1] - u[mask, 0] / 5.0) ** 2)      # :852
    bc_loss = torch.zeros(1, device="cuda")
    negative = means[mask, 1] < -0.8                              # :855-861
    if torch.any(negative):
        bc_loss += torch.mean((u[mask][negative] - 1.0) ** 2)
    positive = means[mask, 1] > 0.8
    if torch.any(positive):
        bc_loss += torch.mean((u[mask][positive] + 1.0) ** 2)
    conservation_loss = torch.zeros(1, device="cuda")
    conservation_loss += DMEAN * torch.mean(dmeans[mask, 0] ** 2)      # :867-876
    conservation_loss += DMEAN * torch.mean((dmeans[mask] - dmeans[mask].mean(0).reshape(1, -1)) ** 2)
    conservation_loss += DMEAN * torch.mean((means[mask, 1] - means[mask, 1].mean()) ** 2)
    in_range = means[mask, 1].abs() < 0.8
    if torch.any(in_range):
        conservation_loss += DU * torch.mean((u[mask, 0][in_range].abs() - 1.0) ** 2)
        conservation_loss += DU * torch.mean(du[mask][in_range] ** 2)
    return (PDE * pde_loss + BC * bc_loss + CONSERVATION * conservation_loss).reshape(())


def capturable_lines(means, u, deltas, boundary_mask, weights):
    """leg (ac)"""
    terms = state_loss_recipe(means, u, deltas.squeeze(0), boundary_mask.squeeze(-1))
    return (terms * weights).sum()


def operator(means, u, deltas, boundary_mask, weights):
    """leg (b)"""
    return (state_loss_terms(means, u, deltas, boundary_mask) * weights).sum()


class Leg:
    def __init__(self, fn, N, c, backward):
        self.fn, self.backward = fn, backward
        self.leaves, self.mask = problem(N, c)
        self.weights = torch.tensor(WEIGHTS, device="cuda")
        self.result = None

    def make_leaves(self):
        self.leaves = [t.detach().clone().requires_grad_(True) for t in self.leaves]      # the model's forward runs under autograd

    def run(self):
        loss = self.fn(*self.leaves, self.mask, self.weights)
        self.result = torch.autograd.grad(loss, self.leaves) if self.backward else loss

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
        print(f"{table:<8} {N:>6} {c:>2} {name:<42} {h['median_us']:>9.1f} {h['p10_us']:>8.1f} {h['p90_us']:>8.1f}"
              f" {e['median_us']:>9.1f} {e['p10_us']:>8.1f} {e['p90_us']:>8.1f}", flush=True)


LEGS = (("a", "a: the reference's lines", reference_lines, False),
        ("ac", "ac: capturable composition", capturable_lines, False),
        ("acg", "acg: capturable composition, graph replay", capturable_lines, True),
        ("b", "b: state_loss_terms", operator, False),
        ("bg", "bg: state_loss_terms, graph replay", operator, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[56, 1600, 65536])
    ap.add_argument("--channels", type=int, nargs="+", default=[1])
    ap.add_argument("--only", choices=[k for k, _, _, _ in LEGS], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--tables", nargs="+", default=["forward", "fwd+bwd"], choices=["forward", "fwd+bwd"])
    args = ap.parse_args()
    result = {"tool": "bench_state_loss", "reps": args.reps, "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
    print(f"{'table':<8} {'N':>6} {'c':>2} {'leg':<42} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} {'p90':>8}   (us)")
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
                if args.only is None and table == "fwd+bwd":      # the legs agree before they are timed
                    for _, run in legs:
                        run()
                    torch.cuda.synchronize()
                    base = keep[0].result
                    for leg in keep[1:]:
                        for a, b in zip(base, leg.result):
                            assert torch.allclose(a, b.reshape(a.shape), rtol=1e-3, atol=1e-6 * float(a.abs().max())), "legs differ"
                report(table, N, c, measure(legs, args.reps, args.warmup), result)
                del keep
    print(json.dumps(result))


if __name__ == "__main__":
    main()
