"""Step periods on the device timeline of a rocprofv3 --kernel-trace output directory, steps that hold a
runtime copy kernel (__amd_rocclr_copyBuffer: a build memory's blit) apart from those that hold none:

    python tools/step_periods.py <output dir> [--key plan_count] [--skip 20]

A step runs from the start of a launch whose name contains --key to the start of the next one.  (The cold step of
tools/prof_step.py is trusted from its 85th build or so on: --skip 90 leaves the three-launch steps alone.)"""
import argparse
import csv
import glob

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--key", default="plan_count")
ap.add_argument("--skip", type=int, default=20, help="steps left out at the start (warm-up: untrusted builds)")
a = ap.parse_args()
f = glob.glob(a.dir + "/**/*kernel_trace.csv", recursive=True)
assert f, "no kernel_trace.csv under " + a.dir
rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
steps, cur = [], None
for r in rows:
    name = r["Kernel_Name"]
    if a.key in name:
        cur = {"start": int(r["Start_Timestamp"]), "copy": 0, "copy_ns": 0, "launches": 0}
        steps.append(cur)
    if cur is None:
        continue
    cur["launches"] += 1
    if "copyBuffer" in name:
        cur["copy"] += 1
        cur["copy_ns"] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
per = np.diff([s["start"] for s in steps]) / 1e3
steps = steps[:-1]
sel = range(a.skip, len(steps))


def line(tag, idx):
    p = np.array([per[i] for i in idx])
    if not len(p):
        print(f"{tag}: none")
        return
    la = np.mean([steps[i]["launches"] for i in idx])
    print(f"{tag}: {len(p)} steps, period median {np.median(p):.2f} us, mean {p.mean():.2f}, p10 {np.percentile(p, 10):.2f}, "
          f"p90 {np.percentile(p, 90):.2f}; launches per step {la:.2f}")


line("all steps", list(sel))
line("steps with a copy kernel", [i for i in sel if steps[i]["copy"]])
line("steps without", [i for i in sel if not steps[i]["copy"]])
cp = [steps[i]["copy_ns"] / 1e3 for i in sel if steps[i]["copy"]]
if cp:
    print(f"copy kernels in those steps: mean {np.mean(cp):.2f} us")
