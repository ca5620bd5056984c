#!/usr/bin/env python3
"""What a trusted cold build costs when its expectation fails: C3's Gaussians with 1024^2 uniform
random points, met by builds that take them for the 1024 x 1024 lattice the library remembers (PIGS_LATTICE_TRUST=1
after a few lattice builds) against builds that look first (=0): cold step by HIP events.  The trusted builds are
right and slow -- index tiles of random points span the domain, every list overflows into record ranges -- and there
are at most 8 of them before the guard's word is home.

    python tools/lattice_trust_worst_case.py [trust|verify]

Without an argument the two modes run one after the other, each in a process of its own under a time limit (a step of
tens of milliseconds is slow, not stuck; a mode that runs into its limit ends the run)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 4            # all trusted: the guard's word rides home with every 8th build of a size
LIMIT_S = 240


def run(mode):
    import ctypes
    import torch
    from pigs_amd import synthetic, _lib
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(256, 256, 0.5, seed=0)
    t = {k: v.float().cuda() for k, v in gs.items()}
    lat = synthetic.grid_samples(1024).float().cuda()
    M = lat.shape[0]
    rnd = [(torch.rand(lat.shape, generator=torch.Generator().manual_seed(k)) * 2 - 1).cuda() for k in range(STEPS)]
    lib = _lib.load()

    def info():
        buf = (ctypes.c_int64 * 4)()
        lib.pigs_samples_trust_info(M, buf)
        return list(buf)

    os.environ["PIGS_LATTICE_TRUST"] = "1" if mode == "trust" else "0"
    s = GaussianSampler(False, fuse="all", backend="binned", reuse_samples=False)
    with torch.no_grad():
        for _ in range(25):      # lattice builds: the row length, the box and the strips land in the library's memory
            s.preprocess(t["means"], t["values"], None, t["conics"], lat); s.sample((0, 1, 2))
            torch.cuda.synchronize()
        before = info()
        # (a plan's statistics ride home with every 8th build of its sizes: start right behind one)
        ms = []
        for k in range(STEPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.preprocess(t["means"], t["values"], None, t["conics"], rnd[k]); out = s.sample((0, 1, 2))
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            assert bool(torch.isfinite(out[0]).all())
        after = info()
    print(f"PIGS_LATTICE_TRUST={os.environ['PIGS_LATTICE_TRUST']}: cold steps on 1024^2 uniform random points after 25 lattice builds: "
          + ", ".join(f"{x * 1e3:.0f}" for x in ms) + f" us; trusted builds among them: {after[1] - before[1]}; "
          f"guard fired: {after[2] - before[2]}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        import importlib
        importlib.import_module("pigs_amd.build").ensure_built()
        for mode in ("verify", "trust"):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), mode], timeout=LIMIT_S).returncode
            if rc != 0:
                sys.exit(f"mode {mode}: exit status {rc}")
