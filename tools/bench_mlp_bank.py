#!/usr/bin/env python3
"""The attention front of DynamicsNetwork._compute_deltas (model_pn.py:259-261): the four query_transform / key_transform
nets (16 -> 16 -> 16 -> 16 -> 16) over one ``features`` [1, N, 16], leaving ``queries`` and ``keys`` [N, 2, 16].  Two
compositions, each eager and inside a graph replay, alternating in one process:

  (a)   four FusedMLP calls and two torch.stack calls, as INTEGRATION.md section 4 composed them before the bank.
  (ag)  (a) inside a graph replay.
  (b)   one FusedMLPBank over the same four nets, groups = 2: ``qk[0]`` / ``qk[1]``.
  (bg)  (b) inside a graph replay.

Two tables: the forward alone (under autograd, as the model runs it), and forward + backward with gradients arriving at
``queries`` and ``keys`` and leaving to ``features`` and all 32 parameters.  N = 1 600 and 65 536, float32.  The legs
alternate after a warm-up; every figure is taken with the HOST clock around work that ends in a synchronise and with HIP
events around the same work.  Prints medians and p10-p90 and one JSON line.  (b) is only ever compared with (a) of the
same run.

    python tools/bench_mlp_bank.py [--reps 200] [--warmup 20] [--sizes 1600 65536]

Launch counts: a profiler run of ONE leg at two repeat counts; the difference of the kernel calls divided by the
difference of the repeats is the launches per call, whatever the set-up launched:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mlp_bank.py --only b --reps 10 --warmup 0 --sizes 1600 --tables fwd+bwd
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mlp_bank.py --only b --reps 30 --warmup 0 --sizes 1600 --tables fwd+bwd
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pigs_amd.build import ensure_built  # noqa: E402

ensure_built()      # before anything touches the GPU

import torch  # noqa: E402

from bench_mlp import measure, report, sequential  # noqa: E402
from pigs_amd.mlp import FusedMLP, FusedMLPBank  # noqa: E402

WIDTHS, HEADS = (16, 16, 16, 16, 16), 2


class Leg:
    def __init__(self, banked, N, backward):
        self.nets = [sequential(WIDTHS, seed=b) for b in range(2 * HEADS)]          # (q0, q1, k0, k1)
        if banked:
            self.bank = FusedMLPBank(self.nets, groups=2)
        else:
            self.fused = [FusedMLP.from_sequential(net) for net in self.nets]
        self.banked = banked
        g = torch.Generator().manual_seed(1)
        self.x = torch.randn((1, N, WIDTHS[0]), generator=g).cuda()
        self.g_q = torch.randn((N, HEADS, WIDTHS[-1]), generator=g).cuda()
        self.g_k = torch.randn((N, HEADS, WIDTHS[-1]), generator=g).cuda()
        self.backward = backward
        self.result = None

    def make_leaves(self):
        self.x = self.x.detach().clone().requires_grad_(True)
        self.leaves = [self.x] + [p for net in self.nets for p in net.parameters()]

    def run(self):
        if self.banked:
            qk = self.bank(self.x)
            queries, keys = qk[0], qk[1]
        else:
            queries = torch.stack([net(self.x)[0] for net in self.fused[:HEADS]], dim=1)
            keys = torch.stack([net(self.x)[0] for net in self.fused[HEADS:]], dim=1)
        if self.backward:
            self.result = torch.autograd.grad((queries, keys), self.leaves, (self.g_q, self.g_k))
        else:
            self.result = (queries, keys)

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


LEGS = (("a", "a: 4 FusedMLP + 2 stack", False, False),
        ("ag", "ag: the same, graph replay", False, True),
        ("b", "b: FusedMLPBank", True, False),
        ("bg", "bg: the same, graph replay", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    ap.add_argument("--only", choices=[k for k, _, _, _ in LEGS], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--tables", nargs="+", default=["forward", "fwd+bwd"], choices=["forward", "fwd+bwd"])
    args = ap.parse_args()
    result = {"tool": "bench_mlp_bank", "reps": args.reps, "torch": torch.__version__,
              "device": torch.cuda.get_device_name(0)}
    print(f"{'table':<8} {'net':<17} {'N':>6} {'leg':<30} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} "
          f"{'p90':>8}   (us)")
    for table in args.tables:
        for N in args.sizes:
            legs, keep = [], []
            for key, name, banked, graphed in LEGS:
                if args.only not in (None, key):
                    continue
                leg = Leg(banked, N, backward=table == "fwd+bwd")
                keep.append(leg)
                if graphed:
                    legs.append((name, leg.graphed()))
                else:
                    leg.make_leaves()
                    legs.append((name, leg.run))
            report(table, "query_key x 4", N, measure(legs, args.reps, args.warmup), result)
            del keep
    print(json.dumps(result))


if __name__ == "__main__":
    main()
