#!/usr/bin/env python3
"""The dynamics network's per-Gaussian nets (model_pn.py:154-174, 187-198, 203-226), four ways in one process:

  (t)   torch: the nn.Sequential of nn.Linear / nn.Tanh, eager.
  (tg)  (t) inside a graph replay.
  (f)   pigs_amd.fused_mlp through FusedMLP.from_sequential (one launch forward, two backward), eager.
  (fg)  (f) inside a graph replay.

Two tables: the forward alone (under autograd, as the model runs it), and forward + backward from a given gradient on the
output towards the input and every weight and bias.  The three nets (input_projection with in_dims = 18, one query / key
transform, delta_net with c = 2) at N = 1 600 and 65 536, float32, input [1, N, w] as the model passes it.  The legs
alternate after a warm-up; every figure is taken with the HOST clock around work that ends in a synchronise and with HIP
events around the same work.  Prints medians and p10-p90 and one JSON line.

    python tools/bench_mlp.py [--reps 200] [--warmup 20] [--sizes 1600 65536] [--nets input_projection query_key delta_net]

Launch counts: a profiler run of ONE leg at two repeat counts; the difference of the kernel calls divided by the
difference of the repeats is the launches per call, whatever the set-up launched:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mlp.py --only f --reps 10 --warmup 0 --sizes 1600 --nets delta_net
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mlp.py --only f --reps 30 --warmup 0 --sizes 1600 --nets delta_net
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

from pigs_amd.mlp import FusedMLP  # noqa: E402

NETS = {"input_projection": (18, 16, 32, 48, 16), "query_key": (16, 16, 16, 16, 16), "delta_net": (48, 32, 16, 16, 48, 32, 7)}


def sequential(widths, seed=0):
    torch.manual_seed(seed)
    mods = []
    for k, (w_in, w_out) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(torch.nn.Linear(w_in, w_out))
        if k + 2 < len(widths):
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).cuda()


class Leg:
    def __init__(self, fused, widths, N, backward):
        self.net = sequential(widths)
        if fused:
            self.net = FusedMLP.from_sequential(self.net)
        g = torch.Generator().manual_seed(1)
        self.x = torch.randn((1, N, widths[0]), generator=g).cuda()
        self.g_y = torch.randn((1, N, widths[-1]), generator=g).cuda()
        self.backward = backward
        self.result = None

    def make_leaves(self):
        self.x = self.x.detach().clone().requires_grad_(True)
        self.leaves = [self.x] + list(self.net.parameters())

    def run(self):
        y = self.net(self.x)
        self.result = torch.autograd.grad(y, self.leaves, self.g_y) if self.backward else y

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


def report(table, net, N, times, result):
    for name, t in times.items():
        row = {}
        for clock in ("host", "event"):
            p10, med, p90 = np.percentile(t[clock], [10, 50, 90])
            row[clock] = {"median_us": round(float(med), 1), "p10_us": round(float(p10), 1), "p90_us": round(float(p90), 1)}
        result.setdefault(table, {}).setdefault(f"{net},N={N}", {})[name] = row
        h, e = row["host"], row["event"]
        print(f"{table:<8} {net:<17} {N:>6} {name:<30} {h['median_us']:>9.1f} {h['p10_us']:>8.1f} {h['p90_us']:>8.1f}"
              f" {e['median_us']:>9.1f} {e['p10_us']:>8.1f} {e['p90_us']:>8.1f}", flush=True)


LEGS = (("t", "t: nn.Sequential", False, False),
        ("tg", "tg: nn.Sequential, graph replay", False, True),
        ("f", "f: fused_mlp", True, False),
        ("fg", "fg: fused_mlp, graph replay", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    ap.add_argument("--nets", nargs="+", default=list(NETS), choices=list(NETS))
    ap.add_argument("--only", choices=[k for k, _, _, _ in LEGS], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--tables", nargs="+", default=["forward", "fwd+bwd"], choices=["forward", "fwd+bwd"])
    args = ap.parse_args()
    result = {"tool": "bench_mlp", "reps": args.reps, "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
    print(f"{'table':<8} {'net':<17} {'N':>6} {'leg':<30} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} {'p90':>8}   (us)")
    for table in args.tables:
        for net in args.nets:
            for N in args.sizes:
                legs, keep = [], []
                for key, name, fused, graphed in LEGS:
                    if args.only not in (None, key):
                        continue
                    leg = Leg(fused, NETS[net], N, backward=table == "fwd+bwd")
                    keep.append(leg)
                    if graphed:
                        legs.append((name, leg.graphed()))
                    else:
                        leg.make_leaves()
                        legs.append((name, leg.run))
                report(table, net, N, measure(legs, args.reps, args.warmup), result)
                del keep
    print(json.dumps(result))


if __name__ == "__main__":
    main()
