"""The scripted sequence of cold builds behind tests/test_stats_home_gpu.py, run as a program in a process of its own
(the library's memories are process-global, and the way a plan's statistics come home -- PIGS_STATS_HOME -- is what
the test compares):

    python tests/stats_home_sequence.py <result.json>

Every step is a cold preprocess + forward (orders 0-2) followed by a stream synchronise; the result is one record per
step: phase, the four words of pigs_samples_trust_info, the samples' lattice, PlanParams::strips, the tiles per header
mode, and the outputs' error against oracle/dense_torch.py in float64."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDERS = (0, 1, 2)
# A cloud with thin outskirts: the shape of tests/test_strips_gpu.py (64 x 64 lattice Gaussians under 150 000 clamped
# normals), which has tiles in TILE_MODE_POINTS -- under 32 x 32 Gaussians no tile's lists grow long enough for the
# per-point walk.  The second cloud has 64 points more: another size for the plans' memory.
CLOUD = 150000


def grid(rx, ry):
    gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, rx), np.linspace(-1.0, 1.0, ry))
    return np.stack((gx, gy), -1).reshape(-1, 2)


def main(out_path):
    from diff_gaussian_sampling import GaussianSampler
    from oracle import dense_torch
    from pigs_amd import _lib, synthetic
    lib = _lib.load()
    dev = torch.device("cuda", 0)

    def gaussians(n, seed):
        gs = synthetic.lattice_gaussians(n, n, 0.5, seed=seed)
        return {k: gs[k].float().to(dev) for k in ("means", "values", "conics")}

    g32, g64 = gaussians(32, 0), gaussians(64, 5)
    rng = np.random.default_rng(61)

    def points(a):
        return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)

    def cloud(n):
        return points(np.clip(rng.normal(0, 0.15, (n, 2)), -1, 1))

    lattice = points(grid(64, 64))
    random = points(rng.uniform(-1, 1, (64 * 64, 2)))
    cloud_a, cloud_b = cloud(CLOUD), cloud(CLOUD + 64)
    # (phase, Gaussians, points, PIGS_GAUSS_STRIPS for the phase's first builds, how many of them, builds)
    phases = [("lattice", g32, lattice, None, 0, 32), ("random", g32, random, None, 0, 12), ("lattice again", g32, lattice, None, 0, 12),
              ("cloud, cells", g64, cloud_a, None, 0, 12), ("cloud, strips first", g64, cloud_b, "1", 2, 6)]
    exp = {}
    s = GaussianSampler(False, backend="binned", fuse="all", reuse_samples=False)
    info = (ctypes.c_int64 * 6)()
    records = []
    for name, t, pts, forced, nforced, builds in phases:
        if name not in exp:
            e = dense_torch.forward(t["means"].double(), t["conics"].double(), t["values"].double(), pts.double(), orders=ORDERS)
            exp[name] = {o: e[o] for o in ORDERS}
        M = pts.shape[0]
        for k in range(builds):
            if forced is not None and k < nforced:
                os.environ["PIGS_GAUSS_STRIPS"] = forced
            else:
                os.environ.pop("PIGS_GAUSS_STRIPS", None)
            with torch.no_grad():
                s.preprocess(t["means"], t["values"], None, t["conics"], pts.clone())
                outs = s.sample(ORDERS)
            torch.cuda.current_stream().synchronize()
            trust = (ctypes.c_int64 * 4)()
            assert lib.pigs_samples_trust_info(M, trust) == 0
            plan = s._plan
            ws, sws = plan.workspace, plan.samples.workspace
            off = lib.pigs_plan_strips_offset()
            strips = int(ws[off:off + 4].view(torch.int32).cpu()[0])
            off = lib.pigs_samples_lattice_offset()
            lat = sws[off:off + 8].view(torch.int32).cpu().tolist()
            assert lib.pigs_plan_layout_info(plan.N, plan.M, plan.c, info) == 0
            ntiles, off_hdr = info[0], info[2]
            hdr = ws[off_hdr:off_hdr + 32 * ntiles].view(torch.int32).cpu().numpy().astype(np.uint32).reshape(ntiles, 8)
            modes = np.bincount(hdr[:, 0] >> 30, minlength=4).tolist()
            err = []
            for o in ORDERS:
                want = exp[name][o]
                got = outs[o].double().reshape(want.shape)
                err.append(float((got - want).abs().max() / want.abs().max()) if bool(torch.isfinite(got).all()) else float("inf"))
            records.append({"phase": name, "build": k, "trust": list(trust), "lattice": lat, "strips": strips, "modes": modes, "err": err})
    with open(out_path, "w") as f:
        json.dump(records, f)


if __name__ == "__main__":
    main(sys.argv[1])
