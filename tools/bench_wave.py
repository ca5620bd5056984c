#!/usr/bin/env python3
"""What the one-launch coupled residual buys: per-step time of the reference's wave loss (test_no_mlp.py:127-139)

    ub   = tau prev + (1 - tau) current                      (tau: one random weight per point)
    res0 = (u[0] - pu[0]) / dt - ub[1]
    res1 = (u[1] - pu[1]) / dt - (10 lap ub[0] - 0.1 ub[1])
    loss = mean(res0^2) + 0.01 mean(res1^2)

of a two-channel field against a frozen previous level, and its gradients

  (a) "coupled"      through GaussianSampler.residual(couple0=, couple_lap=, couple_weight=): the previous level's part
                     as the target (one launch under no_grad), the current level's residual in one forward and one
                     backward launch; 4 accumulators and 8 bytes per point each way;
  (b) "composed_lap" the same loss from sample((0, "lap")) of both levels and torch elementwise kernels with their autograd;
  (c) "composed_19"  the same from sample((0, 1, "lap")), the call a user of the reference's recipe would write: the
                     compiled covering mask accumulates grad u although nothing reads it.

(b) and (c) run unchanged on a tree without the coupled residual: they are the baseline.  The three alternate in one
process, timed with HIP events (warm-ups first), medians and spreads.  The previous level is bound and evaluated in
every step by all three, as in the reference's loop (its points are drawn anew each step).  Two sizes:

  ref  the reference's training size: N = 1 600 lattice Gaussians (variance ~ e^-4), M = 1 024 uniform points, dense;
  c3   BASELINE configs[2] with two channels (kappa = 0.5: 65 536 Gaussians x 1024^2 grid), binned.

A step is preprocess (current level) + loss + gradients wrt means, values, conics ("step"); "fwd" is preprocess + loss
under no_grad.  Prints one JSON line per (size, what).  DESIGN.md 14 holds the recorded numbers.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pigs_amd import synthetic  # noqa: E402

DT = 0.01
Q0 = ((0.0, -1.0), (0.0, 0.1))
QL = ((0.0, 0.0), (-10.0, 0.0))
NEG = lambda q: tuple(tuple(-x for x in row) for row in q)      # noqa: E731


def ref_case(seed=1):
    gs = synthetic.lattice_gaussians(40, 40, 1.3, seed=seed, c=2)
    g = torch.Generator().manual_seed(seed)
    return gs, (torch.rand((1024, 2), generator=g) * 2 - 1).cuda(), "dense"


def c3_case():
    return synthetic.lattice_gaussians(256, 256, 0.5, c=2), synthetic.grid_samples(1024).float().cuda(), "binned"


def make_steps(gs, pts, backend, host):
    from diff_gaussian_sampling import GaussianSampler
    t = {k: v.float().cuda() for k, v in gs.items()}
    for k in ("means", "values", "conics"):
        t[k].requires_grad_(True)
    leaves = (t["means"], t["values"], t["conics"])
    M = pts.shape[0]
    g = torch.Generator().manual_seed(3)
    tau = torch.rand((M,), generator=g).cuda()
    one_minus_tau = 1 - tau
    prev = GaussianSampler(False, backend=backend, host=host)      # the frozen previous level: the same Gaussians, other values
    pm, pv, pc = t["means"].detach(), (torch.rand(t["values"].shape, generator=g) * 2 - 1).cuda(), t["conics"].detach()
    s = GaussianSampler(False, backend=backend, host=host)

    def loss_coupled():
        with torch.no_grad():
            prev.preprocess(pm, pv, None, pc, pts)
            T = prev.residual(a0=1 / DT, couple_weight=tau, couple0=NEG(Q0), couple_lap=NEG(QL))
        r = s.residual(a0=1 / DT, couple_weight=one_minus_tau, couple0=Q0, couple_lap=QL, target=T)
        return r[:, 0].pow(2).mean() + 0.01 * r[:, 1].pow(2).mean()

    def composed(orders):
        def loss():
            with torch.no_grad():
                prev.preprocess(pm, pv, None, pc, pts)
                p = prev.sample(orders)
                pu, plap = p[0], p[-1]
            o = s.sample(orders)
            u, lap = o[0], o[-1]
            ut = (u - pu) / DT
            ub = tau[:, None] * pu + one_minus_tau[:, None] * u
            lb = tau[:, None] * plap + one_minus_tau[:, None] * lap
            loss1 = torch.mean((ut[:, 1] - (10 * lb[:, 0] - 0.1 * ub[:, 1])) ** 2)
            loss2 = torch.mean((ut[:, 0] - ub[:, 1]) ** 2)
            return 0.01 * loss1 + loss2
        return loss

    def variant(loss_fn):
        def fwd():
            with torch.no_grad():
                s.preprocess(t["means"], t["values"], None, t["conics"], pts)
                return loss_fn()

        def step():
            s.preprocess(t["means"], t["values"], None, t["conics"], pts)
            loss = loss_fn()
            return (loss,) + torch.autograd.grad(loss, leaves)
        return fwd, step

    return s, {"coupled": variant(loss_coupled), "composed_lap": variant(composed((0, "lap"))),
               "composed_19": variant(composed((0, 1, "lap")))}


def time_once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * (len(xs) - 1) + 0.5))]      # noqa: E731
    return {"median_us": round(q(0.5), 2), "p10_us": round(q(0.1), 2), "p90_us": round(q(0.9), 2), "n": len(xs)}


def run(label, make_case, warmup, iters, host):
    gs, pts, backend = make_case()
    s, variants = make_steps(gs, pts, backend, host)
    # the three paths compute the same thing (at the size that is timed)
    outs = {k: [x.detach().clone() for x in v[1]()] for k, v in variants.items()}
    agree = max(float((a - b).abs().max() / b.abs().max()) for k in ("composed_lap", "composed_19")
                for a, b in zip(outs["coupled"], outs[k]))
    for name, pick in (("fwd", 0), ("step", 1)):
        times = {k: [] for k in variants}
        for _ in range(warmup):
            for v in variants.values():
                v[pick]()
        torch.cuda.synchronize()
        for _ in range(iters):       # alternating: all see the same drift of the machine
            for k, v in variants.items():
                times[k].append(time_once(v[pick]))
        res = {k: stats(x) for k, x in times.items()}
        print(json.dumps({"case": label, "what": name, "N": gs["means"].shape[0], "M": pts.shape[0], "host": host,
                          "backend": "binned" if s._plan is not None else "dense", **res,
                          "coupled_over_composed_lap": round(res["coupled"]["median_us"] / res["composed_lap"]["median_us"], 3),
                          "coupled_over_composed_19": round(res["coupled"]["median_us"] / res["composed_19"]["median_us"], 3),
                          "loss_and_gradients_agree_to": float(f"{agree:.3g}")}), flush=True)
    del s, variants
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", choices=("ref", "c3", "all"), default="all")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host", choices=("native", "ctypes"), default="native")
    a = ap.parse_args()
    import importlib
    importlib.import_module("pigs_amd.build").ensure_built()      # before anything touches the GPU
    if not torch.cuda.is_available():
        raise SystemExit("bench_wave.py needs a GPU")
    if a.size in ("ref", "all"):
        run("ref", ref_case, a.warmup, a.iters, a.host)
    if a.size in ("c3", "all"):
        run("c3", c3_case, max(3, a.warmup // 4), max(10, a.iters // 4), a.host)


if __name__ == "__main__":
    main()
