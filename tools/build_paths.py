"""Which launches do the builds of the binned path issue?  A fixed script of small scenarios that between them take
every launch shape of pigs_amd/csrc/build_choice.h (trusted, ahead with and without strips, the plain chain with and
without a row length, plan-only builds on a clean and an unclean workspace, coarse bins with the staged scatter,
deferred lists, a capture, the aggregation's grid), and a reducer that turns a kernel trace of that script into the
ordered list of launches.  Results never depend on the path a build takes, so this is what pins the paths: run it on
two commits and compare the lists line for line.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/build_paths.py
    python3 tools/build_paths.py --reduce OUT > profiles/build_paths_<commit>.txt

Every scenario has a point count of its own (the library's memories are keyed by size: they do not interact), and
every step ends in a synchronisation, so that a statistic a build asked for has landed before the next build of the
size looks: the sequence is deterministic.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETTINGS = ("PIGS_LATTICE", "PIGS_LATTICE_TRUST", "PIGS_GAUSS_STRIPS", "PIGS_SAMPLES_ORDER", "PIGS_STAGE",
            "PIGS_NO_FUSED_FIRST", "PIGS_NO_AHEAD", "PIGS_BBOX_BLOCKS")
STEPS = 12


def reduce_trace(out_dir):
    """The pigs:: kernels of the trace in start order as `kernel workgroups threads lds`, run-length encoded: `n x`
    in front of a launch, or of the block of launches that the lines `n x [` and `]` enclose."""
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        sys.exit(f"expected one kernel_trace.csv under {out_dir}, found {len(files)}")
    with open(files[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    lines = []
    for r in rows:
        name = r["Kernel_Name"]
        if "pigs::" not in name:
            continue
        name = name.split("(")[0].replace("void ", "")      # the instantiation without its argument list
        wg = int(r["Workgroup_Size_X"])
        lines.append(f"{name} wgs={int(r['Grid_Size_X']) // wg} threads={wg} lds={r['LDS_Block_Size']}")
    i = 0
    while i < len(lines):
        # the shortest block from here on that repeats at once, and how often
        period, reps = 1, 1
        for p in range(1, 13):
            n = 1
            while lines[i + n * p:i + (n + 1) * p] == lines[i:i + p]:
                n += 1
            if n > 1:
                period, reps = p, n
                break
        if period == 1:
            print(f"{reps} x {lines[i]}")
        else:
            print(f"{reps} x [")
            for line in lines[i:i + period]:
                print(f"    {line}")
            print("]")
        i += period * reps


def main():
    for k in SETTINGS:
        os.environ.pop(k, None)
    import importlib
    importlib.import_module("pigs_amd.build").ensure_built()      # (nothing is compiled behind a profiler)
    import torch
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd import synthetic
    from pigs_amd.graphs import GraphedStep
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize

    def gaussians(nx=32, ny=32, grad=False):
        gs = synthetic.lattice_gaussians(nx, ny, 0.5, seed=0)
        return [gs[k].float().to(dev).requires_grad_(grad) for k in ("means", "values", "conics")]

    def sampler(**kw):
        kw.setdefault("reuse_samples", False)
        return GaussianSampler(False, backend="binned", fuse="all", unpinned_aggregate=True, **kw)

    def cold_steps(points, steps=STEPS, grad=False, s=None, settings=None, **kw):
        """`steps` steps on the same sampler; a fresh copy of the points each time unless the sampler reuses them"""
        os.environ.update(settings or {})
        s = s or sampler(**kw)
        means, values, conics = gaussians(grad=grad)
        fixed = points.float().to(dev)
        for _ in range(steps):
            p = fixed if s.reuse_samples else fixed.clone()
            if grad:
                s.preprocess(means, values, None, conics, p)
                u, ux, uxx = s.sample((0, 1, 2))
                ((u ** 2).mean() + (uxx ** 2).mean()).backward()
            else:
                with torch.no_grad():
                    s.preprocess(means, values, None, conics, p)
                    s.sample((0, 1, 2))
            sync()
        for k in settings or {}:
            del os.environ[k]

    lattice = synthetic.grid_samples
    # twelve cold steps of a 128 x 128 lattice over 32 x 32 lattice Gaussians: the plain chain, then with a row length,
    # then the Gaussians one launch ahead, in strips (sort_in_count)
    cold_steps(lattice(128, 128))
    cold_steps(lattice(128, 136), settings={"PIGS_LATTICE_TRUST": "1"})      # trusted builds
    cold_steps(lattice(128, 144), settings={"PIGS_GAUSS_STRIPS": "0"})       # ahead, the Gaussians through the cells
    cold_steps(lattice(128, 152), reuse_samples=True)                        # plan-only builds
    # a differentiable call after a no_grad preprocess: a forward-only plan, then the full one on the same samples
    s = sampler()
    means, values, conics = gaussians(grad=True)
    pts = lattice(128, 160).float().to(dev)
    for _ in range(STEPS):
        p = pts.clone()
        with torch.no_grad():
            s.preprocess(means, values, None, conics, p)
        sync()
        u, ux, uxx = s.sample((0, 1, 2))
        ((u ** 2).mean() + (uxx ** 2).mean()).backward()
        sync()
    # points in no order: coarse bins, the staged scatter; forward + backward through the staging records
    rnd = torch.rand((20000, 2), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1
    cold_steps(rnd, steps=4, settings={"PIGS_SAMPLES_ORDER": "unordered"})
    cold_steps(rnd[:19968], steps=4, grad=True, settings={"PIGS_SAMPLES_ORDER": "unordered", "PIGS_STAGE": "1"})
    # 2^19 points: 512 workgroups in the first launch until a row length is known
    cold_steps(lattice(1024, 512), steps=4)
    # deferred lists: a forward (the fused first forward), a residual, a backward as the first sampling call
    dpts = lattice(128, 168)
    cold_steps(dpts, steps=4, defer_lists=True)
    s = sampler(defer_lists=True)
    means, values, conics = gaussians(grad=True)
    for _ in range(4):
        s.preprocess(means, values, None, conics, dpts.float().to(dev))
        (s.residual(1.0, lap=-0.1) ** 2).mean().backward()
        sync()
    cold_steps(dpts, steps=4, grad=True, defer_lists=True)
    # one capture and two replays
    gsampler = sampler()
    gpts = lattice(128, 176).float().to(dev)

    def fn(means, values, conics):
        gsampler.preprocess(means, values, None, conics, gpts)
        u, ux, lap = gsampler.sample((0, 1, "lap"))
        loss = ((u - 0.1 * lap) ** 2).mean() + (ux ** 2).mean()
        out = (loss,) + torch.autograd.grad(loss, (means, values, conics))
        if not torch.cuda.is_current_stream_capturing():
            sync()
        return out

    step = GraphedStep(fn, lambda: gaussians(grad=True))
    for _ in range(2):
        step()
        sync()
    # the aggregation's grid (48 x 48 Gaussians: up to 2 048 the neighbour lists test every pair and build no grid)
    s = sampler()
    means, values, conics = gaussians(48, 48)
    for _ in range(2):
        with torch.no_grad():
            s.preprocess(means, values, None, conics, lattice(64, 64).float().to(dev))
            s.preprocess_aggregate()
        sync()
    print("build_paths: done")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reduce":
        reduce_trace(sys.argv[2])
    else:
        main()
