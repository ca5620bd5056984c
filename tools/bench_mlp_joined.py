#!/usr/bin/env python3
"""The tail of DynamicsNetwork._compute_deltas and magnitude_loss of Model.compute_loss (model_pn.py:265-268, 892-901):
``features`` [1, N, 16] and the heads' neighbour features ``nf`` [N, 2, 16] into delta_net (48 -> 32 -> 16 -> 16 -> 48 ->
32 -> 7), and the mean square of each head's block.  Two compositions, each eager and inside a graph replay, alternating in
one process:

  (a)   torch.cat + FusedMLP + magnitude_loss in torch lines as the model writes them (a zeros, per head a slice, pow,
        mean and an indexed write, then sub, pow, mean), as INTEGRATION.md section 4 composed it before ``joined``.
  (ag)  (a) inside a graph replay.
  (b)   ``delta_net.joined((features, nf), block_means=(0, H))`` and ``((mags - 1) ** 2).mean()``.
  (bg)  (b) inside a graph replay.

``--blocks none`` leaves magnitude_loss out of both: the cat + FusedMLP against ``joined`` without block means.

Two tables: the forward alone (under autograd, as the model runs it), and forward + backward with gradients arriving at
``deltas`` and ``magnitude_loss`` and leaving to ``features``, ``nf`` and delta_net's 12 parameters.  N = 1 600 and 65 536,
float32.  The legs alternate after a warm-up; every figure is taken with the HOST clock around work that ends in a
synchronise and with HIP events around the same work.  Prints medians and p10-p90 and one JSON line.  (b) is only ever
compared with (a) of the same run.

    python tools/bench_mlp_joined.py [--reps 200] [--warmup 20] [--sizes 1600 65536] [--blocks heads|none]

Launch counts: a profiler run of ONE leg at two repeat counts; the difference of the kernel calls divided by the
difference of the repeats is the launches per call, whatever the set-up launched:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mlp_joined.py --only b --reps 10 --warmup 0 --sizes 1600 --tables fwd+bwd
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_mlp_joined.py --only b --reps 30 --warmup 0 --sizes 1600 --tables fwd+bwd
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
from pigs_amd.mlp import FusedMLP  # noqa: E402

WIDTHS, HEADS, LATENT = (48, 32, 16, 16, 48, 32, 7), 2, 16


class Leg:
    def __init__(self, joined, N, backward, blocks):
        self.net = FusedMLP.from_sequential(sequential(WIDTHS))
        self.joined, self.blocks, self.backward = joined, blocks, backward
        g = torch.Generator().manual_seed(1)
        self.features = torch.randn((1, N, LATENT), generator=g).cuda()
        self.nf = torch.randn((N, HEADS, LATENT), generator=g).cuda()
        self.g_y = torch.randn((1, N, WIDTHS[-1]), generator=g).cuda()
        self.result = None

    def make_leaves(self):
        self.features = self.features.detach().clone().requires_grad_(True)
        self.nf = self.nf.detach().clone().requires_grad_(True)
        self.leaves = [self.features, self.nf] + list(self.net.parameters())

    def run(self):
        magnitude_loss = None
        if self.joined:
            if self.blocks:
                deltas, mags = self.net.joined((self.features, self.nf), block_means=(0, HEADS))
                magnitude_loss = ((mags - 1.0) ** 2).mean()
            else:
                deltas = self.net.joined((self.features, self.nf))
        else:
            N = self.nf.shape[0]
            local_global_features = torch.cat((self.features, self.nf.reshape(1, N, -1)), dim=-1)      # :265-268
            deltas = self.net(local_global_features)
            if self.blocks:                                                                        # :892-901
                magnitudes = torch.zeros(HEADS, device=deltas.device)
                for i in range(HEADS):
                    block = local_global_features[:, :, LATENT * (i + 1):LATENT * (i + 2)]
                    magnitudes[i] = block.pow(2).mean()
                magnitude_loss = (magnitudes - 1.0).pow(2).mean()
        if not self.backward:
            self.result = (deltas, magnitude_loss)
        elif magnitude_loss is None:
            self.result = torch.autograd.grad(deltas, self.leaves, self.g_y)
        else:
            self.result = torch.autograd.grad((deltas, magnitude_loss), self.leaves, (self.g_y, torch.ones_like(magnitude_loss)))

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


LEGS = (("a", "a: cat + FusedMLP + torch", False, False),
        ("ag", "ag: the same, graph replay", False, True),
        ("b", "b: FusedMLP.joined", True, False),
        ("bg", "bg: the same, graph replay", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    ap.add_argument("--only", choices=[k for k, _, _, _ in LEGS], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--tables", nargs="+", default=["forward", "fwd+bwd"], choices=["forward", "fwd+bwd"])
    ap.add_argument("--blocks", default="heads", choices=["heads", "none"], help="none: without magnitude_loss")
    args = ap.parse_args()
    result = {"tool": "bench_mlp_joined", "reps": args.reps, "blocks": args.blocks, "torch": torch.__version__,
              "device": torch.cuda.get_device_name(0)}
    print(f"{'table':<8} {'net':<17} {'N':>6} {'leg':<30} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} "
          f"{'p90':>8}   (us)")
    what = "delta_net + mags" if args.blocks == "heads" else "delta_net"
    for table in args.tables:
        for N in args.sizes:
            legs, keep = [], []
            for key, name, joined, graphed in LEGS:
                if args.only not in (None, key):
                    continue
                leg = Leg(joined, N, backward=table == "fwd+bwd", blocks=args.blocks == "heads")
                keep.append(leg)
                if graphed:
                    legs.append((name, leg.graphed()))
                else:
                    leg.make_leaves()
                    legs.append((name, leg.run))
            report(table, what, N, measure(legs, args.reps, args.warmup), result)
            del keep
    print(json.dumps(result))


if __name__ == "__main__":
    main()
