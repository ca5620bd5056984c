#!/usr/bin/env python3
"""The update of an MLP-free training step (the Gaussians are the parameters), several ways in one process:

  (a)  the composition around the sampler: tanh(raw_means) * scale, exp(raw_scaling),
       pigs_amd.covariances.build_covariances, the autograd backward of those from given d means / d values / d conics,
       torch.optim.Adam at its default, zero_grad(set_to_none=True);
  (af) the same with Adam(fused=True), where this torch build offers it;
  (b)  GaussianAdam.step() from the same gradients (one launch);
  (bg) GaussianAdam(capturable=True).step() inside a graph replay;
  (as) (a) plus the reference's four statistic ops on the raw gradients (test_no_mlp.py:149-155);
  (bs) GaussianAdam(grad_stats=True).step(): the same statistics kept in the one launch.

and, in a second table, the whole step -- sampler forward + mean-square loss + backward + update -- with (a), (b) and
(b) captured by pigs_amd.graphs.GraphedStep, at 1 024 sample points; and in a third the d = 1 update at N = 25 and 1 600,
c = 1, with statistics: the reference's chain (test_no_mlp_1d.py:109-111, 156-162, 189-190), GaussianAdam1D.step()
eager and in a graph replay.

Sizes N = 1 600 and 65 536, c = 1 and 2, float32.  The legs alternate after a warm-up.  Every figure is taken twice:
with the HOST clock around work that ends in a synchronise, and with HIP events around the same work.  Prints medians
and p10-p90 and one JSON line.

    python tools/bench_optim.py [--reps 200] [--warmup 20] [--sizes 1600 65536] [--channels 1 2] [--no-step] [--no-1d]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_optim.py --only a --reps 20 --no-step   # launches of (a)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_optim.py --only b --reps 20 --no-step   # launches of (b)
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

from pigs_amd.covariances import build_covariances  # noqa: E402
from pigs_amd.optim import GaussianAdam, GaussianAdam1D  # noqa: E402

SCALE, LR = 2.5, 1e-2


def parameters(N, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    raw_means = (0.8 * torch.randn((N, 2), generator=g)).cuda()
    values = torch.randn((N, c), generator=g).cuda()
    raw_scaling = (torch.rand((N, 2), generator=g) * 3.0 - 4.0).cuda()
    transform = (torch.rand((N, 1), generator=g) * 2.0 - 1.0).cuda()
    return raw_means, values, raw_scaling, transform


def gradients(N, c, seed=1):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(s, generator=g).cuda() for s in ((N, 2), (N, c), (N, 3)))      # d means, d values, d conics


class TorchLeg:
    """leg (a): the parent's composition"""

    def __init__(self, N, c, fused=False, stats=False):
        self.params = [p.requires_grad_(True) for p in parameters(N, c)]
        kw = {"fused": True} if fused else {}
        self.optim = torch.optim.Adam(self.params, lr=LR, **kw)
        self.stats = None
        if stats:       # mean_grad, mean_grad_norm, scale_grad, scale_grad_norm
            self.stats = [torch.zeros(N, 2).cuda(), torch.zeros(N).cuda(), torch.zeros(N, 2).cuda(), torch.zeros(N).cuda()]

    def statistics(self):
        if self.stats is not None:      # test_no_mlp.py:150-153
            mean_grad, mean_grad_norm, scale_grad, scale_grad_norm = self.stats
            mean_grad += self.params[0].grad
            mean_grad_norm += torch.norm(mean_grad, dim=-1)
            scale_grad += self.params[2].grad
            scale_grad_norm += torch.norm(scale_grad, dim=-1)

    def gaussians(self):
        raw_means, values, raw_scaling, transform = self.params
        cov, con = build_covariances(torch.exp(raw_scaling), transform)
        return torch.tanh(raw_means) * SCALE, values, cov, con

    def update(self, grads):
        means, values, _, con = self.gaussians()
        values.grad = grads[1]
        torch.autograd.backward((means, con), (grads[0], grads[2]))
        self.statistics()
        self.optim.step()
        self.optim.zero_grad(set_to_none=True)

    def whole(self, sampler, samples, target):
        means, values, cov, con = self.gaussians()
        sampler.preprocess(means, values, cov, con, samples)
        loss = torch.mean((sampler.sample_gaussians()[:, 0] - target) ** 2)
        loss.backward()
        self.optim.step()
        self.optim.zero_grad(set_to_none=True)
        return loss.detach()


class HipLeg:
    """leg (b): GaussianAdam"""

    def __init__(self, N, c, capturable=False, stats=False):
        self.opt = GaussianAdam(*parameters(N, c), lr=LR, means_map="tanh", scale=SCALE, capturable=capturable,
                                grad_stats=stats)

    def update(self, grads):
        g = self.opt.gaussians()
        g.means.grad, g.values.grad, g.conics.grad = grads
        self.opt.step()

    def whole(self, sampler, samples, target):
        g = self.opt.gaussians()
        sampler.preprocess(g.means, g.values, g.covariances, g.conics, samples)
        loss = torch.mean((sampler.sample_gaussians()[:, 0] - target) ** 2)
        loss.backward()
        self.opt.step()
        return loss.detach()


class Torch1dLeg:
    """d = 1: the reference's chain with its statistic ops"""

    def __init__(self, N, c):
        raw_means, values, raw_scaling, _ = parameters(N, c)
        self.params = [p.requires_grad_(True) for p in (raw_means[:, :1].contiguous(), values, raw_scaling[:, :1].contiguous())]
        self.optim = torch.optim.Adam(self.params, lr=LR)
        self.stats = [torch.zeros(N, 1).cuda(), torch.zeros(N).cuda(), torch.zeros(N, 1).cuda(), torch.zeros(N).cuda()]

    def update(self, grads):
        raw_means, values, scaling = self.params
        means = torch.tanh(raw_means) * SCALE
        covariances = torch.exp(scaling).reshape(-1, 1)
        conics = 1.0 / covariances
        values.grad = grads[1]
        torch.autograd.backward((means, conics), (grads[0], grads[2]))
        mean_grad, mean_grad_norm, scale_grad, scale_grad_norm = self.stats
        mean_grad += raw_means.grad
        mean_grad_norm += torch.norm(mean_grad, dim=-1)
        scale_grad += scaling.grad
        scale_grad_norm += torch.norm(scale_grad, dim=-1)
        self.optim.step()
        self.optim.zero_grad(set_to_none=True)


class Hip1dLeg(HipLeg):
    """d = 1: GaussianAdam1D with statistics"""

    def __init__(self, N, c, capturable=False):
        raw_means, values, raw_scaling, _ = parameters(N, c)
        self.opt = GaussianAdam1D(raw_means[:, :1].contiguous(), values, raw_scaling[:, :1].contiguous(), lr=LR,
                                  means_map="tanh", scale=SCALE, capturable=capturable, grad_stats=True)


def graphed_update(N, c, grads, leg=None):
    leg = leg or HipLeg(N, c, capturable=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            leg.update(grads)
        g = leg.opt.gaussians()
        g.means.grad, g.values.grad, g.conics.grad = grads
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        leg.opt.step()
    torch.cuda.current_stream().wait_stream(side)
    return graph.replay, (leg, graph)


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
        print(f"{table:<7} {N:>6} {c:>2} {name:<34} {h['median_us']:>9.1f} {h['p10_us']:>8.1f} {h['p90_us']:>8.1f}"
              f" {e['median_us']:>9.1f} {e['p10_us']:>8.1f} {e['p90_us']:>8.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1600, 65536])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--only", choices=["a", "af", "b", "bg", "as", "bs"], help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step table")
    ap.add_argument("--no-1d", action="store_true", help="skip the d = 1 table")
    ap.add_argument("--sizes-1d", type=int, nargs="+", default=[25, 1600])
    args = ap.parse_args()
    result = {"tool": "bench_optim", "reps": args.reps, "torch": torch.__version__}
    print(f"{'table':<7} {'N':>6} {'c':>2} {'leg':<34} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} {'p90':>8}   (us)")
    for N in args.sizes:
        for c in args.channels:
            grads = gradients(N, c)
            legs, keep = [], None
            if args.only in (None, "a"):
                a = TorchLeg(N, c)
                legs.append(("a: torch chain + Adam", lambda a=a: a.update(grads)))
            if args.only in (None, "af"):
                try:
                    af = TorchLeg(N, c, fused=True)
                    af.update(grads)
                    legs.append(("af: torch chain + Adam(fused)", lambda af=af: af.update(grads)))
                except (RuntimeError, TypeError, ValueError) as e:
                    result["fused"] = f"not measured: {str(e).splitlines()[0]}"
            if args.only in (None, "b"):
                b = HipLeg(N, c)
                legs.append(("b: GaussianAdam.step", lambda b=b: b.update(grads)))
            if args.only in (None, "bg"):
                replay, keep = graphed_update(N, c, grads)
                legs.append(("bg: GaussianAdam.step, graph replay", replay))
            if args.only in (None, "as"):
                a_s = TorchLeg(N, c, stats=True)
                legs.append(("as: torch chain + stats + Adam", lambda a_s=a_s: a_s.update(grads)))
            if args.only in (None, "bs"):
                bs = HipLeg(N, c, stats=True)
                legs.append(("bs: GaussianAdam(grad_stats).step", lambda bs=bs: bs.update(grads)))
            report("update", N, c, measure(legs, args.reps, args.warmup), result)
            del keep
    if not args.no_1d and not args.only:
        for N in args.sizes_1d:
            c = 1
            g = torch.Generator().manual_seed(3)
            grads = tuple(torch.randn((N, 1), generator=g).cuda() for _ in range(3))     # d means, d values, d conics
            a1, b1 = Torch1dLeg(N, c), Hip1dLeg(N, c)
            replay, keep = graphed_update(N, c, grads, Hip1dLeg(N, c, capturable=True))
            legs = [("a1: torch 1-D chain + stats + Adam", lambda: a1.update(grads)),
                    ("b1: GaussianAdam1D.step, stats", lambda: b1.update(grads)),
                    ("b1g: GaussianAdam1D, graph replay", replay)]
            report("1d", N, c, measure(legs, args.reps, args.warmup), result)
            del keep
    if not args.no_step and not args.only:
        from diff_gaussian_sampling import GaussianSampler
        from pigs_amd.graphs import GraphedStep
        for N in args.sizes:
            c = 1
            g = torch.Generator().manual_seed(2)
            samples = ((torch.rand((args.points, 2), generator=g) * 2 - 1) * SCALE).cuda()
            target = torch.exp(-0.5 * (samples ** 2).sum(-1) / 0.25)
            a, b = TorchLeg(N, c), HipLeg(N, c)
            sa, sb = GaussianSampler(False), GaussianSampler(False)
            holder = {}

            def make_inputs():
                holder["leg"], holder["sampler"] = HipLeg(N, c, capturable=True), GaussianSampler(False)
                return samples.clone(), target.clone()
            step = GraphedStep(lambda s, t: holder["leg"].whole(holder["sampler"], s, t), make_inputs)
            legs = [("a: sampler + torch chain + Adam", lambda: a.whole(sa, samples, target)),
                    ("b: sampler + GaussianAdam", lambda: b.whole(sb, samples, target)),
                    ("bg: the whole step, graph replay", step)]
            report("step", N, c, measure(legs, args.reps, args.warmup), result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
