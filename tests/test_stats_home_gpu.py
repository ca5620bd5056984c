"""GPU: the plans' statistics come home by the list launch's own stores (plan_lists.h, ListArgs::home; build_memory.h,
home / sent) and say what the copy of the workspace header said (PIGS_STATS_HOME=0, the blit behind the build).

One scripted sequence of cold builds (tests/stats_home_sequence.py) runs twice, each time in a fresh process -- the
library's memories are process-global -- with PIGS_LATTICE_TRUST=1 (trust without the 64-build streak) and a stream
synchronise behind every step, so that whatever a build sent home has landed before the next build asks:

  1. 32 builds of a 64 x 64 lattice of points over 32 x 32 lattice Gaussians (kappa = 0.5): strips and trust set in,
     `strip_cover` and `strips` come home;
  2. 12 builds of 4 096 uniform random points, the same count: a trusted build's guard fires (`lattice_broken`);
  3. 12 builds of the lattice again;
  4. 12 builds of a clamped-normal cloud (sigma = 0.15; 150 000 points over 64 x 64 Gaussians, the shape of
     tests/test_strips_gpu.py) through the cells: tiles in TILE_MODE_POINTS (`n_points`);
  5. 6 builds of a second such cloud of another size, the first two with the strips forced: `points_wanted` is the
     only word that can send the builds behind them back to the cells.

The two runs must tell the same story step for step, every step's outputs are held against oracle/dense_torch.py at
the tolerance of tests/test_strips_gpu.py, and the random points turn the samples' memory around within the bound
tests/test_lattice_trust_gpu.py states (1 + 8 + 1 builds)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-5                     # tests/test_strips_gpu.py
TURN_AROUND_BUILDS = 1 + 8 + 1     # tests/test_lattice_trust_gpu.py, test_the_expectation_breaks
HERE = os.path.dirname(os.path.abspath(__file__))


def run_sequence(tmp_path, home):
    out = tmp_path / f"home{home}.json"
    env = dict(os.environ)
    for k in ("PIGS_LATTICE", "PIGS_GAUSS_STRIPS", "PIGS_NO_AHEAD", "PIGS_SAMPLES_ORDER"):
        env.pop(k, None)
    env["PIGS_STATS_HOME"] = home
    env["PIGS_LATTICE_TRUST"] = "1"
    proc = subprocess.run([sys.executable, os.path.join(HERE, "stats_home_sequence.py"), str(out)], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-4000:]
    return json.load(open(out))


@pytest.fixture(scope="module")
def runs(hip_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stats_home")
    return {home: run_sequence(tmp, home) for home in ("1", "0")}


def landed(rec):
    """Both memories of the lattice's sizes have landed: the samples' says trust, the plans' says strips."""
    return rec["trust"][0] == 1 and rec["strips"] == 1


def test_both_ways_home_tell_the_same_story(runs):
    a, b = runs["1"], runs["0"]
    assert len(a) == len(b) == 32 + 12 + 12 + 12 + 6
    first = next((k for k in range(len(a)) if landed(a[k]) and landed(b[k])), None)
    # (two builds send their words, the third is the first into a recycled workspace: a handful at the most)
    assert first is not None and first <= 8, first
    for k in range(first, len(a)):
        ra, rb = dict(a[k]), dict(b[k])
        ra.pop("err"), rb.pop("err")
        assert ra == rb, (k, ra, rb)


@pytest.mark.parametrize("home", ["1", "0"])
def test_every_step_is_the_oracles(runs, home):
    for k, r in enumerate(runs[home]):
        assert max(r["err"]) < TOL, (k, r)


@pytest.mark.parametrize("home", ["1", "0"])
def test_every_word_comes_home(runs, home):
    recs = runs[home]
    by = {}
    for r in recs:
        by.setdefault(r["phase"], []).append(r)
    lat = by["lattice"]
    # strip_cover, strips: the lattice keeps the caller's order and is trusted, build after build
    assert lat[0]["strips"] == 0 and lat[-1]["strips"] == 1 and lat[-1]["lattice"] == [64, 64]
    assert lat[-1]["trust"][0] == 1 and lat[-1]["trust"][1] > lat[15]["trust"][1] > 0, lat[-1]
    assert lat[-1]["trust"][2] == 0
    # lattice_broken: the guard fires on the random points and the memory turns around within the bound
    rnd = by["random"]
    turned = next((k for k, r in enumerate(rnd) if r["lattice"] == [0, 0] and r["trust"][2] >= 1 and r["trust"][0] == 0), None)
    assert turned is not None and turned < TURN_AROUND_BUILDS, [(r["trust"], r["lattice"]) for r in rnd]
    assert rnd[-1]["lattice"] == [0, 0]
    # n_points: the cloud has tiles in TILE_MODE_POINTS and stays with the cells
    cells = by["cloud, cells"]
    assert all(r["strips"] == 0 and r["modes"][3] > 0 for r in cells), [(r["strips"], r["modes"]) for r in cells]
    # points_wanted: two forced strips builds (no tile in TILE_MODE_POINTS: they hold no grid to walk) say that the
    # cells are wanted, and the builds behind them take the cells
    forced = by["cloud, strips first"]
    assert [r["strips"] for r in forced] == [1, 1, 0, 0, 0, 0], [r["strips"] for r in forced]
    assert forced[0]["modes"][3] == 0 and forced[-1]["modes"][3] > 0, [r["modes"] for r in forced]
