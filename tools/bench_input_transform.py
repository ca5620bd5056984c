#!/usr/bin/env python3
"""The dynamics network's input transform (model_pn.py:51-152, :237-249), four ways in one process:

  (t)   torch: a module of the reference's shape (Conv1d latent net, mean, five TransformNets, seven broadcast matrix
        products, two cats) written here in torch ops, eager.
  (tg)  (t) inside a graph replay.
  (f)   pigs_amd.FusedInputTransform.from_module over the same module (three launches forward, five backward and what
        autograd adds for the two inputs that both Functions reach), eager.
  (fg)  (f) inside a graph replay.

Two tables: the forward alone (under autograd, as the model runs it), and forward + backward from a given gradient on
t_params towards means, full_covariances, u and every weight and bias.  c = 2, pde_size = 1 at N = 1 600 and 65 536,
float32.  The legs alternate after a warm-up; every figure is taken with the HOST clock around work that ends in a
synchronise and with HIP events around the same work.  Prints medians and p10-p90 and one JSON line.

    python tools/bench_input_transform.py [--reps 200] [--warmup 20] [--sizes 1600 65536]

Launch counts: a profiler run of ONE leg at two repeat counts; the difference of the kernel calls divided by the
difference of the repeats is the launches per call, whatever the set-up launched:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_input_transform.py --only f --reps 10 --warmup 0 --sizes 1600
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_input_transform.py --only f --reps 30 --warmup 0 --sizes 1600
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pigs_amd.build import ensure_built  # noqa: E402

ensure_built()      # before anything touches the GPU

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mlp import measure, report  # noqa: E402
from pigs_amd.input_transform import FusedInputTransform  # noqa: E402

nn = torch.nn


class Net(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = layers


class TorchInputTransform(nn.Module):
    """the input transform in torch ops, under the reference's child names; returns t_params [1, N, in_dims]"""

    def __init__(self, c, p):
        super().__init__()
        self.c, self.p = c, p
        self.latent_net = Net(nn.Sequential(nn.Conv1d(7 + 6 * c + p, 16, 1), nn.Tanh(), nn.Conv1d(16, 32, 1), nn.Tanh(),
                                            nn.Conv1d(32, 16, 1), nn.Tanh()))
        for name, k in (("transform_net", 2), ("transform_u_net", c), ("transform_ux_net", 2 * c), ("transform_uxx_net", 2 * c),
                        ("transform_pde_net", p)):
            setattr(self, name, Net(nn.Sequential(nn.Linear(16, 48), nn.Tanh(), nn.Linear(48, 32), nn.Tanh(), nn.Linear(32, k * k))))

    def matrix(self, net, latent):
        k = int(round(net.layers[4].out_features ** 0.5))
        return torch.eye(k, device=latent.device).unsqueeze(0) + net.layers(latent).reshape(-1, k, k)

    def forward(self, means, full_covariances, u, boundaries, sample_u, sample_ux, sample_uxx, sample_pde):
        N, c, p = means.shape[0], self.c, self.p
        boundaries = boundaries.reshape(1, -1, 1)
        x = torch.cat((means.unsqueeze(0), full_covariances.reshape(1, -1, 4), u.unsqueeze(0), boundaries, sample_u.unsqueeze(0),
                       sample_ux.unsqueeze(0), sample_uxx.unsqueeze(0), sample_pde.unsqueeze(0)), dim=-1).transpose(1, 2)
        latent = self.latent_net.layers(x).mean(-1)
        T = [self.matrix(getattr(self, name), latent) for name in ("transform_net", "transform_u_net", "transform_ux_net",
                                                                   "transform_uxx_net", "transform_pde_net")]
        t_means = T[0] @ means.reshape(-1, 2, 1)       # computed and unused, as in the reference
        parts = (T[0] @ full_covariances.reshape(-1, 2, 2), T[1] @ u.reshape(-1, c, 1), T[1] @ sample_u.reshape(-1, c, 1),
                 T[2] @ sample_ux.reshape(-1, 2 * c, 1), T[3] @ sample_uxx.reshape(-1, 2 * c, 1),
                 T[4] @ sample_pde.reshape(-1, p, 1))
        del t_means
        flat = [t.reshape(1, N, -1) for t in parts]
        return torch.cat((flat[0], flat[1], boundaries, flat[2], flat[3], flat[4], flat[5]), dim=-1)


class Leg:
    def __init__(self, fused, c, p, N, backward):
        torch.manual_seed(0)
        self.net = TorchInputTransform(c, p).cuda()
        if fused:
            self.net = FusedInputTransform.from_module(self.net)
        g = torch.Generator().manual_seed(1)
        widths = (2, 4, c, 1, c, 2 * c, 2 * c, p)
        self.rows = [torch.randn((N, w), generator=g).cuda() for w in widths]
        self.rows[1] = self.rows[1] * 0.3
        self.g_t = torch.randn((1, N, 5 + 6 * c + p), generator=g).cuda()
        self.backward = backward
        self.result = None

    def make_leaves(self):
        self.rows = [t.detach().clone().requires_grad_(k < 3) for k, t in enumerate(self.rows)]
        self.leaves = self.rows[:3] + list(self.net.parameters())

    def run(self):
        t = self.net(*self.rows)
        self.result = torch.autograd.grad(t, self.leaves, self.g_t) if self.backward else t

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


LEGS = (("t", "t: torch module", False, False),
        ("tg", "tg: torch module, graph replay", False, True),
        ("f", "f: FusedInputTransform", True, False),
        ("fg", "fg: FusedInputTransform, replay", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--pde-size", type=int, default=1)
    ap.add_argument("--only", choices=[k for k, _, _, _ in LEGS], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--tables", nargs="+", default=["forward", "fwd+bwd"], choices=["forward", "fwd+bwd"])
    args = ap.parse_args()
    result = {"tool": "bench_input_transform", "reps": args.reps, "torch": torch.__version__,
              "device": torch.cuda.get_device_name(0)}
    what = f"c={args.c},p={args.pde_size}"
    print(f"{'table':<8} {'net':<17} {'N':>6} {'leg':<30} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} {'p90':>8}   (us)")
    for table in args.tables:
        for N in args.sizes:
            legs, keep = [], []
            for key, name, fused, graphed in LEGS:
                if args.only not in (None, key):
                    continue
                leg = Leg(fused, args.c, args.pde_size, N, backward=table == "fwd+bwd")
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
