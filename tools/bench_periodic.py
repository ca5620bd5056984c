#!/usr/bin/env python3
"""What the periodic domain costs: the same workload with ``periodic=None`` and ``periodic=(-1, 1)``, alternating
in one process, timed with HIP events (warm-ups first), medians and spreads.  Two sizes:

  ns  the reference's Navier-Stokes size (main_pn.py:24, nx = ny = 20, and 40 x 40 after growth): N = 400 / 1 600
      lattice Gaussians (variance ~ e^-4, model_pn.py:344), M = 1 024 uniform points, c = 2: preprocess + orders
      0-3 forward ("fwd0-3"), and that plus a loss and its backward ("fwd0-3+bwd").
  c3  BASELINE configs[2] (pigs_amd.synthetic, kappa = 0.5, 65 536 Gaussians x 1024^2 grid), c = 1: preprocess +
      orders 0-2 without gradients ("pre+fwd0-2"), and the training step preprocess + orders 0-2 + loss + backward
      ("fwd0-2+bwd").

Prints one JSON line per (size, step) with the per-step times in microseconds.  The two new kernels' own times come
from a separate run under ``rocprofv3 --kernel-trace --stats`` (``--iters`` small); ``--bytes`` prints the
algorithmic bytes of the images kernel and the fold for both sizes and exits (no GPU needed).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pigs_amd import synthetic  # noqa: E402

BOX = (-1.0, 1.0)


def kernel_bytes(N, c, elem=4):
    """Algorithmic bytes: images reads N rows of (2 + 3 + c) and writes 9N; the fold reads 9N and writes N."""
    row = (2 + 3 + c) * elem
    return {"images": N * row + 9 * N * row, "fold": 9 * N * row + N * row, "images_write": 9 * N * row}


def ns_case(n, c=2, M=1024, seed=1):
    gs = synthetic.lattice_gaussians(n, n, 1.3, seed=seed, c=c)
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand((M, 2), generator=g) * 2 - 1).cuda()
    return gs, pts, (0, 1, 2, 3)


def c3_case():
    gs, pts = synthetic.CONFIGS["c3"](0.5)
    return gs, pts.float().cuda(), (0, 1, 2)


def make_steps(gs, pts, orders, periodic, host):
    from diff_gaussian_sampling import GaussianSampler
    t = {k: v.float().cuda() for k, v in gs.items()}
    for k in ("means", "values", "conics"):
        t[k].requires_grad_(True)
    s = GaussianSampler(False, host=host, periodic=periodic)
    g = torch.Generator().manual_seed(3)
    M, c = pts.shape[0], t["values"].shape[1]
    shapes = {0: (M, c), 1: (M, 2, c), 2: (M, 2, 2, c), 3: (M, 2, 2, 2, c)}
    ws = [(torch.rand(shapes[o], generator=g) * 2 - 1).cuda() for o in orders]

    def fwd():
        with torch.no_grad():
            s.preprocess(t["means"], t["values"], t["covariances"], t["conics"], pts)
            return s.sample(orders)

    def step():
        s.preprocess(t["means"], t["values"], t["covariances"], t["conics"], pts)
        loss = sum((o * w).sum() for o, w in zip(s.sample(orders), ws))
        return torch.autograd.grad(loss, (t["means"], t["values"], t["conics"]))

    return s, fwd, step


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


def run(label, make_case, warmup, iters, host, which=("none", "periodic")):
    gs, pts, orders = make_case()
    variants = {k: make_steps(gs, pts, orders, None if k == "none" else BOX, host) for k in which}
    fwd_name = "fwd0-3" if len(orders) == 4 else "pre+fwd0-2"
    bwd_name = "fwd0-3+bwd" if len(orders) == 4 else "fwd0-2+bwd"
    for name, pick in ((fwd_name, 1), (bwd_name, 2)):
        times = {k: [] for k in variants}
        for _ in range(warmup):
            for k, v in variants.items():
                v[pick]()
        torch.cuda.synchronize()
        for _ in range(iters):       # alternating: both see the same drift of the machine
            for k, v in variants.items():
                times[k].append(time_once(v[pick]))
        res = {k: stats(x) for k, x in times.items()}
        N = gs["means"].shape[0]
        line = {"case": label, "step": name, "N": N, "M": pts.shape[0], "c": gs["values"].shape[1], "host": host,
                "backend": {k: ("binned" if v[0]._plan is not None else "dense") for k, v in variants.items()}, **res}
        if len(res) == 2:
            line["ratio_median"] = round(res["periodic"]["median_us"] / res["none"]["median_us"], 3)
        print(json.dumps(line), flush=True)
    del variants
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", choices=("ns", "c3", "all"), default="all")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host", choices=("native", "ctypes"), default="native")
    ap.add_argument("--variant", choices=("both", "none", "periodic"), default="both",
                    help="one variant alone: for the rocprofv3 runs, whose per-kernel sums must not mix the two")
    ap.add_argument("--bytes", action="store_true", help="print the two kernels' algorithmic bytes and exit")
    a = ap.parse_args()
    if a.bytes:
        for label, N, c in (("ns400", 400, 2), ("ns1600", 1600, 2), ("c3", 65536, 1)):
            print(json.dumps({"case": label, "N": N, "c": c, "f32_bytes": kernel_bytes(N, c)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_periodic.py needs a GPU")
    which = ("none", "periodic") if a.variant == "both" else (a.variant,)
    if a.size in ("ns", "all"):
        for n in (20, 40):
            run(f"ns{n * n}", lambda n=n: ns_case(n), a.warmup, a.iters, a.host, which)
    if a.size in ("c3", "all"):
        run("c3", c3_case, max(3, a.warmup // 4), max(10, a.iters // 4), a.host, which)


if __name__ == "__main__":
    main()
