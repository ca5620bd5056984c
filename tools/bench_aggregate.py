#!/usr/bin/env python3
"""Timing of preprocess_aggregate / aggregate_neighbors (this repo's definition: DESIGN.md 9) at the
model's sizes (model_pn.py:44-49: L = K = 16, F = 6, E = 25) and beyond: HIP events around 50 calls.

    bench_aggregate.py                                  the table of profiles/r0*_aggregate.txt
    bench_aggregate.py --periodic LO HI [--sides 40 256] [--rounds 15] [--variants plain periodic]
        the periodic neighbour lists (GaussianSampler(periodic=(LO, HI), periodic_aggregate=True)) against the plain
        ones on the same periodic sampler: both variants alternate in one process, `rounds` times, each round a HIP-event
        timing of 20 calls; medians with p10-p90 of the rounds, for the list build, the forward and forward + backward.
        `--variants plain` times the plain lists alone and runs on a tree without the option too: the comparison of the
        non-periodic path with the parent commit (profiles/aggregate_periodic.txt).
    bench_aggregate.py --heads H [--sides 40 256] [--dtypes float32 float64] [--rounds 15] [--variants calls heads]
        all H attention heads of a layer: (calls) H calls of aggregate_neighbors against (heads) one call of
        aggregate_neighbors_heads on the same inputs, alternating in one process as above, forward and forward +
        backward.  `--variants calls` runs on a tree without the method too: the yardstick of the parent commit
        (profiles/aggregate_heads.txt)."""
import argparse, os, sys, math
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pigs_amd import synthetic
from diff_gaussian_sampling import GaussianSampler


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def table():
    for dtype in (torch.float32, torch.float64):
        for side, kappa in ((40, 1.3), (128, 1.3), (256, 0.5)):
            N, L, K, F = side * side, 16, 16, 6
            E = 4 * F + 1
            gs = synthetic.lattice_gaussians(side, side, kappa, seed=2)
            means, conics = gs["means"].to(dtype).cuda(), gs["conics"].to(dtype).cuda()
            values = gs["values"].to(dtype).cuda()
            g = torch.Generator(device="cpu").manual_seed(5)
            mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype).cuda().requires_grad_(True)
            args = [mk(N, L), mk(L, L), mk(N, K), mk(N, K), mk(F), mk(L, 2 * E)]
            s = GaussianSampler(False, unpinned_aggregate=True)
            s.preprocess(means, values, None, conics, means)
            t_lists = timed(s.preprocess_aggregate)
            nb = s._neighbors
            s2 = GaussianSampler(False, unpinned_aggregate=True, aggregate_cap=nb.cap)      # slab size given: one pass, no read-back
            s2.preprocess(means, values, None, conics, means)
            t_lists_cap = timed(s2.preprocess_aggregate)
            pairs = int(nb.row_counts.sum())
            with torch.no_grad():
                t_fwd = timed(lambda: s.aggregate_neighbors(*args))
            gout = torch.randn((N, L), dtype=dtype, device="cuda")

            def fb():
                out = s.aggregate_neighbors(*args)
                torch.autograd.grad(out, args, grad_outputs=gout)
            t_fb = timed(fb)
            print(f"{str(dtype)[6:]:8s} N={N:6d} kappa={kappa}: {pairs / N:6.1f} neighbours per Gaussian (cap {nb.cap}) | lists {t_lists:7.1f} us (cap given: {t_lists_cap:7.1f}) | "
                  f"forward {t_fwd:7.1f} us | forward + backward (all six gradients) {t_fb:7.1f} us", flush=True)


def torus_gaussians(side, kappa, box, seed=2):
    """side^2 Gaussians that fill the torus [lo, hi)^2 uniformly: one per cell of a side x side lattice, anywhere in its
    cell (synthetic.lattice_gaussians puts its first and last rows on the same seam line of a torus), with the shapes
    of synthetic.lattice_gaussians scaled to the box."""
    lo, hi = box
    gs = synthetic.lattice_gaussians(side, side, kappa, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    idx = torch.arange(side, dtype=torch.float64)
    gx, gy = torch.meshgrid((idx, idx), indexing="ij")
    cells = torch.stack((gx, gy), dim=-1).reshape(side * side, 2)
    means = lo + (cells + torch.rand((side * side, 2), generator=g, dtype=torch.float64)) * ((hi - lo) / side)
    return means, gs["conics"] / ((hi - lo) / 2.0) ** 2, gs["values"]


def setup(side, kappa, dtype, box, periodic_aggregate):
    N, L, K, F = side * side, 16, 16, 6
    E = 4 * F + 1
    means, conics, values = (t.to(dtype).cuda() for t in torus_gaussians(side, kappa, box))
    g = torch.Generator(device="cpu").manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype).cuda().requires_grad_(True)
    args = [mk(N, L), mk(L, L), mk(N, K), mk(N, K), mk(F), mk(L, 2 * E)]
    gout = torch.randn((N, L), dtype=dtype, device="cuda")
    opt = {"periodic_aggregate": True} if periodic_aggregate else {}        # plain: no keyword, so that a tree without it runs
    s = GaussianSampler(False, unpinned_aggregate=True, backend="dense", periodic=box, **opt)
    s.preprocess(means, values, None, conics, means[:16])
    s.preprocess_aggregate()

    def forward():
        with torch.no_grad():
            s.aggregate_neighbors(*args)

    def both():
        out = s.aggregate_neighbors(*args)
        torch.autograd.grad(out, args, grad_outputs=gout)
    return s, {"lists": s.preprocess_aggregate, "forward": forward, "forward + backward": both}


def compare(box, sides, rounds, names=("plain", "periodic")):
    """Plain and periodic lists, alternating in one process (a drift of the machine meets both alike)."""
    import numpy as np
    print(f"# neighbour lists of the torus [{box[0]}, {box[1]})^2 (periodic) against the non-periodic lists of the same "
          f"wrapped Gaussians (plain), both on GaussianSampler(periodic=({box[0]}, {box[1]}))")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one Gaussian per cell of a side x side lattice, "
          f"L = K = 16, F = 6; {rounds} alternating rounds of 20 calls by HIP events, native host", flush=True)
    for dtype in (torch.float32, torch.float64):
        for side in sides:
            kappa = 1.3 if side <= 128 else 0.5
            variants = {v: setup(side, kappa, dtype, box, v == "periodic") for v in names}
            times = {(v, w): [] for v in variants for w in variants[v][1]}
            for _ in range(rounds):
                for v, (_, fns) in variants.items():
                    for w, fn in fns.items():
                        times[v, w].append(timed(fn, 20))
            N = side * side
            for v, (s, _) in variants.items():
                nb = s._neighbors
                print(f"{str(dtype)[6:]:8s} N={N:6d} kappa={kappa} {v:8s}: {int(nb.row_counts.sum())} pairs, "
                      f"{int(nb.row_counts.sum()) / N:6.1f} per Gaussian, cap {nb.cap}", flush=True)
            for w in ("lists", "forward", "forward + backward"):
                med = {}
                for v in variants:
                    t = np.asarray(times[v, w])
                    med[v] = float(np.median(t))
                    print(f"    {w:18s} {v:8s} median {med[v]:8.1f} us  p10-p90 {np.percentile(t, 10):8.1f} - {np.percentile(t, 90):8.1f}")
                if len(med) == 2:
                    print(f"    {w:18s} periodic / plain = {med['periodic'] / med['plain']:.2f}", flush=True)


def setup_heads(side, kappa, dtype, H, names):
    N, L, K, F = side * side, 16, 16, 6
    E = 4 * F + 1
    gs = synthetic.lattice_gaussians(side, side, kappa, seed=2)
    means, conics, values = (gs[k].to(dtype).cuda() for k in ("means", "conics", "values"))
    g = torch.Generator(device="cpu").manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype).cuda().requires_grad_(True)
    # the model's parameters as it holds them; queries and keys per head, and stacked once (a projection's output)
    features, transforms, frequencies, dists = mk(N, L), mk(H, L, L), mk(F), mk(H, L, 2 * E)
    q_heads, k_heads = [mk(N, K) for _ in range(H)], [mk(N, K) for _ in range(H)]
    queries = torch.stack(q_heads, dim=1).detach().requires_grad_(True)
    keys = torch.stack(k_heads, dim=1).detach().requires_grad_(True)
    tr_heads = [transforms[h].detach().clone().requires_grad_(True) for h in range(H)]
    d_heads = [dists[h].detach().clone().requires_grad_(True) for h in range(H)]
    gout = torch.randn((N, H, L), dtype=dtype, device="cuda")
    gout_heads = [gout[:, h].contiguous() for h in range(H)]
    s = GaussianSampler(False, unpinned_aggregate=True, backend="dense")
    s.preprocess(means, values, None, conics, means[:16])
    s.preprocess_aggregate()

    def calls(backward):
        for h in range(H):
            args = (features, tr_heads[h], q_heads[h], k_heads[h], frequencies, d_heads[h])
            if backward:
                torch.autograd.grad(s.aggregate_neighbors(*args), args, grad_outputs=gout_heads[h])
            else:
                with torch.no_grad():
                    s.aggregate_neighbors(*args)

    def heads(backward):
        args = (features, transforms, queries, keys, frequencies, dists)
        if backward:
            torch.autograd.grad(s.aggregate_neighbors_heads(*args), args, grad_outputs=gout)
        else:
            with torch.no_grad():
                s.aggregate_neighbors_heads(*args)
    fns = {"calls": calls, "heads": heads}
    return s, {v: {"forward": (lambda f=fns[v]: f(False)), "forward + backward": (lambda f=fns[v]: f(True))} for v in names}


def compare_heads(H, sides, dtypes, rounds, names):
    """H calls of aggregate_neighbors and one call of aggregate_neighbors_heads, alternating in one process."""
    import numpy as np
    print(f"# {H} heads: (calls) {H} x aggregate_neighbors against (heads) one aggregate_neighbors_heads, same inputs")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; synthetic.lattice_gaussians(side, side, kappa, seed=2), "
          f"L = K = 16, F = 6; {rounds} alternating rounds of 20 calls by HIP events, native host", flush=True)
    for dtype in dtypes:
        for side in sides:
            kappa = 1.3 if side <= 128 else 0.5
            s, variants = setup_heads(side, kappa, dtype, H, names)
            times = {(v, w): [] for v in variants for w in variants[v]}
            for _ in range(rounds):
                for v, fns in variants.items():
                    for w, fn in fns.items():
                        times[v, w].append(timed(fn, 20))
            N = side * side
            nb = s._neighbors
            print(f"{str(dtype)[6:]:8s} N={N:6d} kappa={kappa}: {int(nb.row_counts.sum())} pairs, "
                  f"{int(nb.row_counts.sum()) / N:6.1f} per Gaussian, cap {nb.cap}", flush=True)
            for w in ("forward", "forward + backward"):
                med = {}
                for v in variants:
                    t = np.asarray(times[v, w])
                    med[v] = float(np.median(t))
                    print(f"    {w:18s} {v:6s} median {med[v]:8.1f} us  p10-p90 {np.percentile(t, 10):8.1f} - {np.percentile(t, 90):8.1f}")
                if len(med) == 2:
                    print(f"    {w:18s} heads / calls = {med['heads'] / med['calls']:.2f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--periodic", nargs=2, type=float, metavar=("LO", "HI"), default=None)
    ap.add_argument("--sides", nargs="+", type=int, default=[40, 256], help="lattice sides (N = side^2)")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--variants", nargs="+", choices=("plain", "periodic", "calls", "heads"), default=None)
    ap.add_argument("--heads", type=int, default=None, metavar="H", help="H calls against one call for all H heads")
    ap.add_argument("--dtypes", nargs="+", choices=("float32", "float64"), default=["float32", "float64"])
    a = ap.parse_args()
    if a.heads is not None:
        compare_heads(a.heads, a.sides, [getattr(torch, d) for d in a.dtypes], a.rounds,
                      tuple(dict.fromkeys(a.variants or ["calls", "heads"])))
    elif a.periodic is None:
        table()
    else:
        compare((a.periodic[0], a.periodic[1]), a.sides, a.rounds, tuple(dict.fromkeys(a.variants or ["plain", "periodic"])))
