#!/usr/bin/env python3
"""What the one-launch vorticity terms buy: per-step time of the reference's Navier-Stokes loss (model_pn.py:790-849,
IntegrationRule.TRAPEZOID: mean(div^2) + mean((w_t - dt (nu lap w - u . grad w))^2) on the blend of two time levels with
a random weight per point, the previous level frozen) and its gradients

  (a) "fused"     through GaussianSampler.vorticity_terms(): one forward launch writing [M, 7], one backward launch;
  (b) "composed"  the same loss from sample((0, 1, 2, 3)) and the reference's slicing lines with their autograd;
  (c) "residual"  through GaussianSampler.vorticity_residual(): one forward launch writing [M, 2] (and the [M, 4] record
                  of the blend when a backward follows), one backward launch, and ``out.pow(2).mean(0).sum()``,

and, for the step WITH the data term of main_pn.py:202-212 (``recon_loss``; (c) carries none and is the floor),

  (c') "residual_data"  what a user writes without the fused column: vorticity_residual() + vorticity_terms()[:, 3] on the
                  same plan (a second orders-0..3 launch each way) + the reference's three torch lines for the lookup;
  (d) "fit"       vorticity_residual(data=grid_lookup(image, samples), data_weight=sqrt(5)): one sampler launch each way
                  and one lookup launch,

on the same build, alternating in one process, timed with HIP events (warm-ups first), medians and spreads.  Sizes:

  ref  the reference's sizes: N = 400 and 1 600 lattice Gaussians (variance ~ e^-4), M = 1 024 and 4 096 uniform random
       points, periodic box (-1, 1) (the launches see the 9N images), dense;
  c2   pigs_amd.synthetic.lattice_gaussians(128, 64, 0.7, c=2) x the 256^2 grid, binned;
  fit  legs (c), (c') and (d) only: N = M = 1 600 (dense and binned, periodic and not) and N = M = 65 536 (binned,
       periodic and not), lattice Gaussians x uniform random points, eager and -- "graph": true -- as a hipGraph replay.

Three measures per size: "fwd" is preprocess + loss under no_grad; "step" is preprocess + loss + gradients wrt means,
values, conics; "issue" is the host's wall-clock time to issue one step (no synchronisation inside; the queue is drained
before each).  Prints one JSON line per (size, measure).  ``--bytes`` prints the bytes each path moves per point between
the sampler's kernels and the loss (no GPU needed) and exits.  DESIGN.md 13 and 15 hold the recorded numbers.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pigs_amd import synthetic  # noqa: E402

DT, NU = 0.01, 0.05


def point_bytes(elem=4):
    """Bytes per sample point that cross kernel boundaries, sampler side only (d = 2, c = 2, float32): what the forward
    writes and what the backward reads (the loss chain's own temporaries are not counted)."""
    full = (2 + 4 + 8 + 16) * elem
    # the residual: 8 B written forward (the record of the blend, 16 B more, only when a backward follows); the backward
    # reads the 8 B gradient and that 16 B record
    return {"fused_fwd": 7 * elem, "fused_bwd": 7 * elem, "composed_fwd": full, "composed_bwd": full,
            "residual_fwd": 2 * elem, "residual_bwd": 2 * elem + 4 * elem,
            # with the data term: (c') adds the [M, 7] row of vorticity_terms() each way; (d) a third word each way and the
            # data word the forward reads
            "residual_data_fwd": 2 * elem + 7 * elem, "residual_data_bwd": 2 * elem + 4 * elem + 7 * elem,
            "fit_fwd": 3 * elem + elem, "fit_bwd": 3 * elem + 4 * elem}


def ref_case(n, M, seed=1):
    def make():
        gs = synthetic.lattice_gaussians(n, n, 1.3, seed=seed, c=2)
        g = torch.Generator().manual_seed(seed)
        return gs, (torch.rand((M, 2), generator=g) * 2 - 1).cuda(), "dense", (-1.0, 1.0)
    return make


RES = 64          # the data image (main_pn.py: res x res)


def fit_case(n, backend, periodic, seed=1):
    """N = M = n * n: a lattice whose neighbours overlap as in ref_case, uniform random points"""
    def make():
        gs = synthetic.lattice_gaussians(n, n, 1.3, seed=seed, c=2)
        g = torch.Generator().manual_seed(seed)
        return gs, (torch.rand((n * n, 2), generator=g) * 2 - 1).cuda(), backend, (-1.0, 1.0) if periodic else None
    return make


def c2_case():
    gs = synthetic.lattice_gaussians(128, 64, 0.7, c=2)
    return gs, synthetic.grid_samples(256).float().cuda(), "binned", None


def make_steps(gs, pts, backend, periodic, host, legs=("fused", "composed", "residual")):
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd import grid_lookup
    t = {k: v.float().cuda() for k, v in gs.items()}
    for k in ("means", "values", "conics"):
        t[k].requires_grad_(True)
    leaves = (t["means"], t["values"], t["conics"])
    M = pts.shape[0]
    g = torch.Generator().manual_seed(3)
    tau = torch.rand((M,), generator=g).cuda()
    with torch.no_grad():          # the frozen previous level: the same Gaussians with other values
        s0 = GaussianSampler(False, backend=backend, host=host, periodic=periodic)
        s0.preprocess(t["means"].detach(), (torch.rand(t["values"].shape, generator=g) * 2 - 1).cuda(), None,
                      t["conics"].detach(), pts)
        prev = s0.vorticity_terms().clone()
        if "composed" in legs:
            pu, pux, puxx, puxxx = s0.sample((0, 1, 2, 3))
            # what the reference keeps of a level (model_pn.py:774-781)
            pu, pux, pw = pu.clone(), pux.clone(), (pux[:, 0, 1] - pux[:, 1, 0]).clone()
            pwx, pwxx = (puxx[..., 0, 1] - puxx[..., 1, 0]).clone(), (puxxx[..., 0, 1] - puxxx[..., 1, 0]).clone()
            del puxx, puxxx
        del s0
    image = (torch.rand((RES, RES), generator=g) * 2 - 1).cuda() * float(prev[:, 3].abs().max())
    s = GaussianSampler(False, backend=backend, host=host, periodic=periodic)
    tau1, tau2, tau3 = tau.reshape(-1, 1), tau.reshape(-1, 1, 1), tau.reshape(-1, 1, 1, 1)

    def loss_fused():
        now = s.vorticity_terms()
        u_x, u_y, div, _, w_x, w_y, lap_w = (tau1 * now + (1 - tau1) * prev).unbind(1)
        wt = now[:, 3] - prev[:, 3]
        rhs = DT * (NU * lap_w - (u_x * w_x + u_y * w_y))
        return torch.mean(div ** 2) + torch.mean((wt - rhs) ** 2)

    def loss_composed():
        u_now, ux_now, uxx_now, uxxx_now = s.sample((0, 1, 2, 3))
        w_now = ux_now[:, 0, 1] - ux_now[:, 1, 0]
        wx_now = uxx_now[..., 0, 1] - uxx_now[..., 1, 0]
        wxx_now = uxxx_now[..., 0, 1] - uxxx_now[..., 1, 0]
        u = tau1 * u_now + (1 - tau1) * pu
        ux = tau2 * ux_now + (1 - tau2) * pux
        wx = tau1 * wx_now + (1 - tau1) * pwx
        wxx = tau2 * wxx_now + (1 - tau2) * pwxx
        wt = w_now - pw
        rhs = DT * (NU * (wxx[:, 0, 0] + wxx[:, 1, 1]) - (u[:, 0] * wx[:, 0] + u[:, 1] * wx[:, 1]))
        return torch.mean((ux[:, 0, 0] + ux[:, 1, 1]) ** 2) + torch.mean((wt - rhs) ** 2)

    def loss_residual():
        return s.vorticity_residual(NU, DT, prev, tau).pow(2).mean(0).sum()

    def loss_residual_data():
        out = s.vorticity_residual(NU, DT, prev, tau)
        now = s.vorticity_terms()
        coords = ((pts + 1.0) / 2.0 * RES).to(torch.long).clamp(0, RES - 1)                  # main_pn.py:206-207
        coords = coords[:, 1] * RES + coords[:, 0]
        recon_loss = 5.0 * torch.mean((now[:, 3] - torch.take(image, coords)) ** 2)           # :209-210
        return out.pow(2).mean(0).sum() + recon_loss

    def loss_fit():
        data = grid_lookup(image, pts)
        return s.vorticity_residual(NU, DT, prev, tau, data=data, data_weight=5.0 ** 0.5).pow(2).mean(0).sum()

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

    fns = {"fused": loss_fused, "composed": loss_composed, "residual": loss_residual, "residual_data": loss_residual_data,
           "fit": loss_fit}
    return s, {k: variant(fns[k]) for k in legs}


def time_once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def issue_once(f):
    """The host's time to issue f's launches: the queue is empty when it starts, nothing waits for the GPU inside."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt * 1e6


def stats(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * (len(xs) - 1) + 0.5))]      # noqa: E731
    return {"median_us": round(q(0.5), 2), "p10_us": round(q(0.1), 2), "p90_us": round(q(0.9), 2), "n": len(xs)}


def run(label, make_case, warmup, iters, host):
    gs, pts, backend, periodic = make_case()
    s, variants = make_steps(gs, pts, backend, periodic, host)
    # the two paths compute the same thing (at the size that is timed)
    outs = {k: [x.detach().clone() for x in v[1]()] for k, v in variants.items()}
    agree = max(float((a - b).abs().max() / b.abs().max()) for k in ("fused", "residual")
                for a, b in zip(outs[k], outs["composed"]))
    for name, pick, timer in (("fwd", 0, time_once), ("step", 1, time_once), ("issue", 1, issue_once)):
        times = {k: [] for k in variants}
        for _ in range(warmup):
            for v in variants.values():
                v[pick]()
        torch.cuda.synchronize()
        for _ in range(iters):       # alternating: all see the same drift of the machine
            for k, v in variants.items():
                times[k].append(timer(v[pick]))
        res = {k: stats(x) for k, x in times.items()}
        print(json.dumps({"case": label, "what": name, "N": gs["means"].shape[0], "M": pts.shape[0], "host": host,
                          "backend": "binned" if s._plan is not None else "dense", "periodic": periodic is not None,
                          **res, "fused_over_composed": round(res["fused"]["median_us"] / res["composed"]["median_us"], 3),
                          "residual_over_fused": round(res["residual"]["median_us"] / res["fused"]["median_us"], 3),
                          "loss_and_gradients_agree_to": float(f"{agree:.3g}")}), flush=True)
    del s, variants
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", choices=("ref", "c2", "fit", "all"), default="all")
    ap.add_argument("--fit-n", type=int, nargs="*", default=(40, 256), help="fit: lattice sides (N = M = side^2)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host", choices=("native", "ctypes"), default="native")
    ap.add_argument("--bytes", action="store_true", help="print the bytes per point of both paths and exit")
    a = ap.parse_args()
    if a.bytes:
        print(json.dumps({"per_point_f32_c2_d2": point_bytes()}))
        return
    import importlib
    importlib.import_module("pigs_amd.build").ensure_built()      # before anything touches the GPU
    if not torch.cuda.is_available():
        raise SystemExit("bench_vorticity.py needs a GPU")
    if a.size in ("ref", "all"):
        for n in (20, 40):
            for M in (1024, 4096):
                run(f"ref N={n * n} M={M}", ref_case(n, M), a.warmup, a.iters, a.host)
    if a.size in ("c2", "all"):
        run("c2", c2_case, a.warmup, a.iters, a.host)
    if a.size in ("fit", "all"):
        for n in a.fit_n:
            # all pairs of 65 536 x 65 536 (nine times that on the torus) is not a size the dense path is for
            for backend in (("dense", "binned") if n * n <= 4096 else ("binned",)):
                for periodic in (False, True):
                    for graph in (False, True):
                        run_fit(f"fit N=M={n * n} {backend}{' periodic' if periodic else ''}", fit_case(n, backend, periodic),
                                a.warmup, a.iters if n * n <= 4096 else max(20, a.iters // 4), a.host, graph)


FIT_LEGS = ("residual", "residual_data", "fit")


def run_fit(label, make_case, warmup, iters, host, graph):
    """Legs (c), (c'), (d) alternating; eager, or each as a replay of its own hipGraph (the tensors a graph's step reads
    are made under its capture stream: a fresh make_steps per graph)."""
    from pigs_amd.graphs import GraphedStep
    gs, pts, backend, periodic = make_case()
    s, variants = make_steps(gs, pts, backend, periodic, host, FIT_LEGS)
    outs = {k: [x.detach().clone() for x in v[1]()] for k, v in variants.items()}
    agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs["fit"], outs["residual_data"]))
    for name, pick in (("fwd", 0), ("step", 1)):
        calls, keep = {k: v[pick] for k, v in variants.items()}, []
        if graph:
            for k in FIT_LEGS:
                holder = {}

                def make_inputs(holder=holder):
                    holder["s"], holder["v"] = make_steps(gs, pts, backend, periodic, host, FIT_LEGS)
                    return ()
                calls[k] = GraphedStep(lambda holder=holder, k=k: holder["v"][k][pick](), make_inputs)
                keep.append(holder)
        times = {k: [] for k in FIT_LEGS}
        for _ in range(warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        for _ in range(iters):       # alternating: all see the same drift of the machine
            for k, f in calls.items():
                times[k].append(time_once(f))
        res = {k: stats(x) for k, x in times.items()}
        print(json.dumps({"case": label, "what": name, "graph": bool(graph), "N": gs["means"].shape[0], "M": pts.shape[0],
                          "host": host, "backend": "binned" if s._plan is not None else "dense",
                          "periodic": periodic is not None, **res,
                          "fit_over_residual_data": round(res["fit"]["median_us"] / res["residual_data"]["median_us"], 3),
                          "fit_over_residual": round(res["fit"]["median_us"] / res["residual"]["median_us"], 3),
                          "loss_and_gradients_agree_to": float(f"{agree:.3g}")}), flush=True)
        del calls, keep
    del s, variants
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
