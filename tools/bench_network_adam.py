#!/usr/bin/env python3
"""The optimiser step of the loop with the network (main_pn.py:59, 217-225), several ways in one process, on the
reference DynamicsNetwork's 90 trainable shapes at c = 2 (the 36 of the input transform, 8 + 16 + 16 + 12 of the Linear
nets, transform, distance_transform: some 30 000 elements), with the gradients given:

  (n)   NetworkAdam.step(): two launches;
  (nl)  NetworkAdam.step(loss=, decay=): the same two launches, the loss-weighted rate and the loss sums on the device;
  (ng)  NetworkAdam(capturable=True).step(loss=, decay=) in a graph replay;
  (t)   torch.optim.Adam at its default;
  (tf)  torch.optim.Adam(fused=True), where this torch build offers it;
  (tl)  (t) with the reference's rate lines around it: g["lr"] = prev_lr * loss_weight before the step,
        loss_weight *= exp(-epsilon * loss.item()) after it (a device read per step);
  (tg)  torch.optim.Adam(capturable=True) with a tensor lr in a graph replay.

Every leg hands the 90 gradients to the parameters before its step (a backward would), and the torch legs end with
zero_grad(set_to_none=True) as the reference's loop does; a replay does neither.  The legs alternate after a warm-up.
Every figure is taken twice: with the HOST clock around work that ends in a synchronise, and with HIP events around the
same work.  After the timing, one step of each leg runs under torch.profiler and the device kernels it launched are
counted (``launches``; "not measured" where the profiler does not deliver; torch's captured step is counted from the
same step issued eagerly, the profiler of this build seeing nothing of its replay).  Prints medians and p10-p90 and one JSON line.

    python tools/bench_network_adam.py [--reps 200] [--warmup 20] [--dtype float32] [--no-launches] [--reverse]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_network_adam.py --only n --reps 20 --no-launches
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pigs_amd.build import ensure_built  # noqa: E402

ensure_built()      # before anything touches the GPU

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pigs_amd.input_transform import param_shapes  # noqa: E402
from pigs_amd.network_adam import NetworkAdam  # noqa: E402

LR, EPSILON, C, P, LATENT, HEADS, EMBED = 1e-3, 1.0, 2, 1, 16, 2, 25
LEGS = ("n", "nl", "ng", "t", "tf", "tl", "tg")


def network_shapes(c=C, p=P):
    """the 90 trainable shapes of the reference's DynamicsNetwork (model_pn.py:176-231) at d = 2"""
    def mlp(widths):
        return [s for i, o in zip(widths[:-1], widths[1:]) for s in ((o, i), (o,))]
    shapes = [tuple(s) for s in param_shapes(c, p)]                                    # the input transform: 36
    shapes += mlp((5 + 6 * c + p, 16, 32, 48, LATENT))                                 # input_projection: 8
    for _ in range(2 * HEADS):                                                         # query and key nets: 16 + 16
        shapes += mlp((LATENT,) * 5)
    shapes += mlp((LATENT * (1 + HEADS), 32, 16, 16, 48, 32, 5 + c))                   # delta_net: 12
    shapes += [(HEADS, LATENT, LATENT), (HEADS, LATENT, 2 * EMBED)]                    # transform, distance_transform
    assert len(shapes) == 90
    return shapes


def tensors(shapes, dtype, seed, requires_grad=False):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=dtype).cuda().requires_grad_(requires_grad) for s in shapes]


def give(params, grads):
    for p, g in zip(params, grads):
        p.grad = g


class HipLeg:
    def __init__(self, shapes, dtype, grads, loss=None, capturable=False):
        self.params, self.grads, self.loss = tensors(shapes, dtype, 0, True), grads, loss
        self.opt = NetworkAdam(self.params, lr=LR, capturable=capturable)

    def __call__(self):
        give(self.params, self.grads)
        if self.loss is None:
            self.opt.step()
        else:
            self.opt.step(loss=self.loss, decay=EPSILON)


class TorchLeg:
    def __init__(self, shapes, dtype, grads, loss=None, **kw):
        self.params, self.grads, self.loss = tensors(shapes, dtype, 0, True), grads, loss
        self.opt = torch.optim.Adam(self.params, lr=kw.pop("lr", LR), **kw)
        self.loss_weight = 1.0

    def __call__(self):
        give(self.params, self.grads)
        if self.loss is not None:                      # main_pn.py:217-218
            for g in self.opt.param_groups:
                g["lr"] = LR * self.loss_weight
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        if self.loss is not None:                      # :225
            self.loss_weight *= math.exp(-EPSILON * self.loss.item())


def graphed(leg, step):
    """warm ``step`` up on a side stream, hand the gradients over and capture it alone; returns (replay, keep-alive)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            give(leg.params, leg.grads)
            step()
        give(leg.params, leg.grads)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
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


def launches(run):
    """device kernels of one call, counted by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset", "optimizer.step"))]      # the last: torch's own annotation
    if not kernels:
        raise RuntimeError("the profiler recorded no device kernel")
    names = {}
    for e in kernels:
        short = e.name.split("(")[0].split("<")[0][-48:]
        names[short] = names.get(short, 0) + 1
    return len(kernels), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dtype", choices=["float32", "float64"], default="float32")
    ap.add_argument("--only", choices=LEGS, help="one leg alone (for a rocprofv3 run)")
    ap.add_argument("--no-launches", action="store_true", help="skip the profiler's launch counts")
    ap.add_argument("--reverse", action="store_true", help="alternate the legs in the opposite order")
    args = ap.parse_args()
    dtype = getattr(torch, args.dtype)
    shapes = network_shapes()
    grads = tensors(shapes, dtype, 1)
    loss = torch.tensor(0.01, dtype=dtype).cuda()
    result = {"tool": "bench_network_adam", "reps": args.reps, "torch": torch.__version__, "dtype": args.dtype, "reverse": args.reverse,
              "tensors": len(shapes), "elements": int(sum(np.prod(s) for s in shapes))}
    want = lambda leg: args.only in (None, leg)
    legs, keep, counted = [], [], {}                   # counted: what the profiler runs for a leg, when not the leg itself
    if want("n"):
        legs.append(("n: NetworkAdam.step", HipLeg(shapes, dtype, grads)))
    if want("nl"):
        legs.append(("nl: NetworkAdam.step(loss, decay)", HipLeg(shapes, dtype, grads, loss)))
    if want("ng"):
        leg = HipLeg(shapes, dtype, grads, loss, capturable=True)
        replay, alive = graphed(leg, lambda: leg.opt.step(loss=loss, decay=EPSILON))
        keep.append(alive)
        legs.append(("ng: NetworkAdam.step(loss), replay", replay))
    if want("t"):
        legs.append(("t: torch Adam", TorchLeg(shapes, dtype, grads)))
    if want("tf"):
        try:
            tf = TorchLeg(shapes, dtype, grads, fused=True)
            tf()
            legs.append(("tf: torch Adam(fused)", tf))
        except (RuntimeError, TypeError, ValueError) as e:
            result["fused"] = f"not measured: {str(e).splitlines()[0]}"
    if want("tl"):
        legs.append(("tl: torch Adam + rate lines + .item()", TorchLeg(shapes, dtype, grads, loss)))
    if want("tg"):
        try:
            tg = TorchLeg(shapes, dtype, grads, capturable=True, lr=torch.tensor(LR).cuda())
            replay, alive = graphed(tg, tg.opt.step)
            keep.append(alive)
            legs.append(("tg: torch Adam(capturable), replay", replay))
            counted["tg: torch Adam(capturable), replay"] = tg       # the replay's kernels, issued eagerly
        except (RuntimeError, TypeError, ValueError) as e:
            result["capturable"] = f"not measured: {str(e).splitlines()[0]}"
    if args.reverse:
        legs.reverse()
    print(f"{'leg':<40} {'host med':>9} {'p10':>8} {'p90':>8} {'event med':>9} {'p10':>8} {'p90':>8}   (us)")
    for name, t in measure(legs, args.reps, args.warmup).items():
        row = {}
        for clock in ("host", "event"):
            p10, med, p90 = np.percentile(t[clock], [10, 50, 90])
            row[clock] = {"median_us": round(float(med), 1), "p10_us": round(float(p10), 1), "p90_us": round(float(p90), 1)}
        result.setdefault("step", {})[name] = row
        h, e = row["host"], row["event"]
        print(f"{name:<40} {h['median_us']:>9.1f} {h['p10_us']:>8.1f} {h['p90_us']:>8.1f}"
              f" {e['median_us']:>9.1f} {e['p10_us']:>8.1f} {e['p90_us']:>8.1f}", flush=True)
    if not args.no_launches:
        for name, run in legs:
            try:
                count, names = launches(counted.get(name, run))
            except Exception as e:  # noqa: BLE001  (whatever the profiler of this build raises: the figure is optional)
                count, names = f"not measured: {str(e).splitlines()[0] if str(e) else type(e).__name__}", {}
            result.setdefault("launches", {})[name] = {"count": count, "kernels": names}
            print(f"launches  {name:<40} {count}  {names}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
