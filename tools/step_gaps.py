"""Where a cold step's period goes on the device timeline of a rocprofv3 --kernel-trace output directory: the three
kernels' own durations and the gaps at the launch boundaries between them.

    python tools/step_gaps.py <output dir> [--skip 90]

A step runs from the start of a plan_count_kernel launch (the pack) to the start of the next one; only steps of exactly
three launches -- pack, plan_lists_kernel, tile_forward_kernel: the trusted cold step of tools/prof_step.py -- count.
Printed per quantity: median, mean, p10, p90 over those steps (us)."""
import argparse
import csv
import glob

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--skip", type=int, default=90, help="steps left out at the start (warm-up: untrusted builds)")
a = ap.parse_args()
f = glob.glob(a.dir + "/**/*kernel_trace.csv", recursive=True)
assert f, "no kernel_trace.csv under " + a.dir
rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
steps, cur = [], None
for r in rows:
    if "plan_count_kernel" in r["Kernel_Name"]:
        cur = []
        steps.append(cur)
    if cur is not None:
        cur.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
cols = {k: [] for k in ("period", "pack", "lists", "forward", "kernels", "period - kernels", "pack -> lists", "lists -> forward",
                        "forward -> next pack")}
used = 0
for i in range(a.skip, len(steps) - 1):
    s, nxt = steps[i], steps[i + 1][0][1]
    if len(s) != 3 or "plan_lists_kernel" not in s[1][0] or "tile_forward_kernel" not in s[2][0]:
        continue
    used += 1
    d = [(e - b) / 1e3 for _, b, e in s]
    cols["period"].append((nxt - s[0][1]) / 1e3)
    cols["pack"].append(d[0]); cols["lists"].append(d[1]); cols["forward"].append(d[2])
    cols["kernels"].append(sum(d))
    cols["period - kernels"].append((nxt - s[0][1]) / 1e3 - sum(d))
    cols["pack -> lists"].append((s[1][1] - s[0][2]) / 1e3)
    cols["lists -> forward"].append((s[2][1] - s[1][2]) / 1e3)
    cols["forward -> next pack"].append((nxt - s[2][2]) / 1e3)
print(f"{used} three-launch steps of {len(steps) - 1 - a.skip} behind the first {a.skip}")
for k, v in cols.items():
    if v:
        v = np.array(v)
        print(f"  {k:22s} median {np.median(v):6.2f}  mean {v.mean():6.2f}  p10 {np.percentile(v, 10):6.2f}  p90 {np.percentile(v, 90):6.2f}")
