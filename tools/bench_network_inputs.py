#!/usr/bin/env python3
"""What GaussianSampler.network_inputs() buys: the no_grad front of the reference's Model.forward (model_pn.py:645-664),
sampled at the Gaussians' own means (M = N),

  (a) "fused"     preprocess + network_inputs(): one sampling launch that writes the four arrays;
  (b) "composed"  the best composition before it: preprocess + sample((0, 1, 2, 3)) for Navier-Stokes, sample((0, 1, 2))
                  otherwise, plus the reference's torch lines (slices, products, stack, reshape, cat),

on the same build, alternating in one process, timed with HIP events after warm-ups: medians and spreads.  Cases: N = M =
1 600 and 65 536 lattice Gaussians; diffusion at c = 1 and Navier-Stokes at c = 2; dense and binned.  Three measures per
case, one JSON line each:

  "eager"    the whole front, issued call by call;
  "replay"   the same captured in a hipGraph and replayed;
  "kernel"   the sampling launch alone on a bound sampler (binned: a built plan), REPEAT launches back to back in one
             graph so that no host time is in it: the new kernel against the sampler launch it subsumes (orders 0..2 or
             0..3).  ``new_over_parent`` is judged against the parent launch's own p10..p90.

``--trace fused|composed`` runs ten eager fronts of one case and nothing else, for a ``rocprofv3 --kernel-trace --stats``
run of its own: the launches per front are the stats' call counts over ten.  DESIGN.md 25 holds the recorded numbers.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pigs_amd import synthetic  # noqa: E402

NU, WAVE = 0.05, (10.0, 0.1)
KINDS = {"diffusion": 1, "navier_stokes": 2}      # right-hand side: channels


def reference_lines(pde, outs):
    """model_pn.py:650-664 on the sampler's outputs"""
    sample_u, sample_ux, sample_uxx = outs[0], outs[1], outs[2]
    n = sample_u.shape[0]
    if pde == "navier_stokes":
        sample_uxxx = outs[3]
        sample_wx = sample_uxx[..., 0, 1] - sample_uxx[..., 1, 0]
        sample_wxx = sample_uxxx[..., 0, 1] - sample_uxxx[..., 1, 0]
        sample_pde = (NU * (sample_wxx[:, 0, 0] + sample_wxx[:, 1, 1])
                      - (sample_u[:, 0] * sample_wx[:, 0] + sample_u[:, 1] * sample_wx[:, 1])).reshape(n, -1)
    else:
        sample_pde = (sample_uxx[:, 0, 0] + sample_uxx[:, 1, 1]).reshape(n, -1)
    sample_ux = sample_ux.reshape(n, -1)
    sample_uxx = torch.cat((sample_uxx[:, 0, 0], sample_uxx[:, 1, 1]), dim=-1).reshape(n, -1)
    return sample_u, sample_ux, sample_uxx, sample_pde


def make_case(n_side, pde, backend):
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(n_side, n_side, 1.0, seed=1, c=KINDS[pde])
    t = {k: v.float().cuda() for k, v in gs.items()}
    orders = (0, 1, 2, 3) if pde == "navier_stokes" else (0, 1, 2)
    s = GaussianSampler(False, backend=backend, host="ctypes")

    def bind():
        s.preprocess(t["means"], t["values"], None, t["conics"], t["means"])

    def fused():
        with torch.no_grad():
            bind()
            return tuple(s.network_inputs(pde, nu=NU, wave=WAVE))

    def composed():
        with torch.no_grad():
            bind()
            return reference_lines(pde, s.sample(orders))

    def kernels(repeat):
        """(the parent's launch, the new launch), each ``repeat`` times on the bound sampler"""
        from pigs_amd.sampler import forward_raw
        with torch.no_grad():
            bind()
            s.sample(orders)                          # binned: builds the plan that these orders run on
            core = s._core
            plan = core.plan3 if (3 in orders and core.plan3 is not None) else core.plan
            inputs = core.inputs()
            mask = sum(1 << o for o in orders)

        def parent():
            with torch.no_grad():
                for _ in range(repeat):
                    forward_raw(*inputs, mask, plan)

        def new():
            with torch.no_grad():
                for _ in range(repeat):
                    s.network_inputs(pde, nu=NU, wave=WAVE)
        return parent, new
    return s, t, fused, composed, kernels


def graphed(f, warmup=3):
    from pigs_amd.graphs import GraphedStep
    return GraphedStep(f, lambda: (), warmup=warmup)


def time_once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(xs, per=1):
    xs = sorted(x / per for x in xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * (len(xs) - 1) + 0.5))]      # noqa: E731
    return {"median_us": round(q(0.5), 2), "p10_us": round(q(0.1), 2), "p90_us": round(q(0.9), 2), "n": len(xs)}


def alternate(a, b, warmup, iters):
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):       # alternating: both see the same drift of the machine
        ta.append(time_once(a))
        tb.append(time_once(b))
    return ta, tb


def run(n_side, pde, backend, warmup, iters):
    s, t, fused, composed, kernels = make_case(n_side, pde, backend)
    N = n_side * n_side
    agree = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(fused(), composed()))
    head = {"N": N, "M": N, "pde": pde, "c": KINDS[pde], "backend": "binned" if s._plan is not None else "dense"}
    big = N > 10000
    it = max(10, iters // 10) if big and head["backend"] == "dense" else iters
    for what, fa, fb in (("eager", fused, composed), ("replay", graphed(fused), graphed(composed))):
        ta, tb = alternate(fa, fb, warmup, it)
        ra, rb = stats(ta), stats(tb)
        print(json.dumps({**head, "what": what, "fused": ra, "composed": rb,
                          "fused_over_composed": round(ra["median_us"] / rb["median_us"], 3),
                          "agree_to": float(f"{agree:.3g}")}), flush=True)
    repeat = 2 if big and head["backend"] == "dense" else 20
    parent, new = kernels(repeat)
    tp, tn = alternate(graphed(parent), graphed(new), warmup, it)
    rp, rn = stats(tp, repeat), stats(tn, repeat)
    print(json.dumps({**head, "what": "kernel", "launches_per_graph": repeat, "parent": rp, "new": rn,
                      "new_over_parent": round(rn["median_us"] / rp["median_us"], 3),
                      "new_within_parent_p90": rn["median_us"] <= rp["p90_us"]}), flush=True)
    del s
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sides", type=int, nargs="+", default=[40, 256], help="lattice sides: N = M = side^2")
    ap.add_argument("--backends", nargs="+", default=["dense", "binned"], choices=("dense", "binned"))
    ap.add_argument("--pdes", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--trace", choices=("fused", "composed"), help="ten eager fronts of the first case and nothing else")
    a = ap.parse_args()
    import importlib
    importlib.import_module("pigs_amd.build").ensure_built()      # before anything touches the GPU
    if not torch.cuda.is_available():
        raise SystemExit("bench_network_inputs.py needs a GPU")
    if a.trace:
        _, _, fused, composed, _ = make_case(a.sides[0], a.pdes[0], a.backends[0])
        for _ in range(10):
            (fused if a.trace == "fused" else composed)()
        torch.cuda.synchronize()
        return
    for side in a.sides:
        for pde in a.pdes:
            for backend in a.backends:
                run(side, pde, backend, a.warmup, a.iters)


if __name__ == "__main__":
    main()
