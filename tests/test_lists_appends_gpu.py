"""GPU: the forward-only appends of the list build (pigs_amd/csrc/plan_lists.h, append_group): a forward-only plan
forms no group masks -- every group's ballot is taken where its compare is made and its entries are appended at once,
on the product path and on the general path alike.  Which entry goes where, and in which order, must not move.

Every case is built forward-only FOUR times in one process, one sampler with the samples half reused (the same sorted
points in every build): PIGS_LISTS_PRODUCT = 1 and = 0, each under PIGS_STORE_THROUGH = 1 and = 0, PIGS_GAUSS_STRIPS = 1
throughout (one kind of walk: one order of the entries).

  * Two builds under the same PIGS_LISTS_PRODUCT are equal WORD FOR WORD (tests/test_store_through_gpu.py, same_words:
    the five header words of every tile, every list up to the length its header states, record ranges, records,
    boxes, the way back) and their outputs bit-equal.
  * A product build against a general build: tests/test_lists_product_gpu.py, same_lists -- the same header modes, the
    same entries in the same order, with that test's one exception and no other (an entry of the product build alone
    lies within 1e-5 q of the cut-off in float64, at most 1 in 10^4 entries of a case); a tile that keeps record
    ranges has the same header and the same ranges in both; where no entry is extra the two builds are equal word for
    word and their outputs bit-equal.
  * Every build's outputs meet the float64 dense oracle (oracle/c_oracle) at 1e-5 of the largest entry on at most
    2 048 sampled points, the bar of the existing list tests.  (With a NaN conic in the scene: on the sampled points
    whose output is finite, against the oracle without that Gaussian; the builds agree bit for bit on which are not.)

Cases: <1, ...> (64 x 64 points, one tile per wave) at kappa = 0.5 over 16 x 16 Gaussians, plain and with one NaN centre
and one rho = 0.9999 conic; <4, ...> (520 x 512 points: 4 160 tiles > LISTS_SMALL_TILES, 65 tile columns -- odd, so the
sixteen 1 x 4 blocks at the turning edges take the general path inside a product build) at kappa = 0.5 and at kappa =
1.3 (several flushes per block: counts carried over flushes, the last step of a flush partly empty); a ragged last
tile (60 x 60 points, no multiple of 64: sorted points, the general path, three groups of the last tile empty);
capacity (a sparse lattice of Gaussians and 600 more within 0.02 of one point: the group lists around it pass
list_cap, those tiles keep record ranges in every build, every other tile its lists), in <1> and in <4>; a full plan
of the <1> and the <4> scene (its group lists are the forward-only plan's word for word -- strips, LIST tiles: the
narrow cut-off is the same -- and its tile list passes check_plan under both PIGS_LISTS_PRODUCT settings and is equal
entry for entry between them).

Survivors per block, a condition on the inputs that was chosen on the CPU with oracle/plan_lists.py (min_q_rect over the
blocks' group boxes: 64 x 64 at kappa 0.5 21-50 distinct Gaussians per block; 520 x 512 at kappa 0.5 46-88, at kappa 1.3
86-246) and is asserted from the built lists, each class in the case that supplies it: there are blocks with at most
64 (64 x 64), with 65-128 (520 x 512 at kappa 0.5) and with more than 128 (kappa 1.3).
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle, plan_lists as PL
from test_binned_matrix_gpu import round32
from test_lists_product_gpu import Built, same_lists, structural
from test_plan_lists_gpu import env, lattice_of
from test_store_through_gpu import (ORDERS, SAMPLED, TOL, Runs, lattice_scene, meets_oracle, modes, same_outputs,
                                     same_words, written)

pytestmark = pytest.mark.gpu

SMALL = dict(nx=64, ny=64, gx=16, gy=16, kappa=0.5, seed=1)
LARGE = dict(nx=520, ny=512, gx=128, gy=128, kappa=0.5, seed=2)
LARGE_WIDE = dict(nx=520, ny=512, gx=64, gy=64, kappa=1.3, seed=3)

def distinct_per_block(snap):
    """[blocks] distinct Gaussians named by the group lists of a block (one tile, or four where the launch takes four
    tiles per wave: build_choice.h, LISTS_SMALL_TILES)"""
    w = written(snap)
    tiles = snap["tiles"]
    tpw = 4 if tiles > 4096 else 1
    out = []
    for b in range(tiles // tpw):
        named = [w["glist"][t, g, :w["hdr"][t, 1 + g]] for t in range(b * tpw, (b + 1) * tpw) for g in range(4)]
        out.append(len(np.unique(np.concatenate(named))))
    return np.array(out)


def finite_points_meet_oracle(x, outs, without, label):
    """a scene with a NaN conic: the sampled points whose outputs are finite, against the oracle without that Gaussian"""
    M = len(x["pts"])
    idx = np.unique(np.random.default_rng(5).integers(0, M, SAMPLED)) if M > SAMPLED else np.arange(M)
    keep = np.setdiff1d(np.arange(len(x["means"])), without)
    exp = c_oracle.forward(x["means"][keep], x["conics"][keep], x["values"][keep], x["pts"][idx], orders=ORDERS)
    fin = np.ones(len(idx), dtype=bool)
    for out in outs:
        fin &= np.isfinite(out.cpu().double().numpy()[idx].reshape(len(idx), -1)).all(1)
    assert fin.sum() >= len(idx) // 2, (label, int(fin.sum()))
    for o, out in zip(ORDERS, outs):
        got = out.cpu().double().numpy()[idx].reshape(len(idx), -1)[fin]
        want = exp[o].reshape(len(idx), -1)[fin]
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{label}: order {o} against c_oracle on {int(fin.sum())} finite points of {len(idx)}: {err:.2e}")
        assert err < TOL, (label, o, err)


def four_builds(hip_lib, x, label, nan_gaussians=None):
    """forward-only under PIGS_LISTS_PRODUCT x PIGS_STORE_THROUGH; returns {(product, through): (snapshot, outputs,
    Built)} and the sampler's Runs"""
    r = Runs(x, True)
    got = {}
    for product in ("1", "0"):
        for through in ("1", "0"):
            with env("PIGS_LISTS_PRODUCT", product):
                snap, outs = r.build(hip_lib, through)
            name = f"{label}, PIGS_LISTS_PRODUCT={product} PIGS_STORE_THROUGH={through}"
            if nan_gaussians is None:
                meets_oracle(x, outs, name)
            else:
                finite_points_meet_oracle(x, outs, nan_gaussians, name)
            got[product, through] = (snap, outs, Built(r.s, r.s._plan, hip_lib, x))
    for product in ("1", "0"):
        a, b = got[product, "1"], got[product, "0"]
        same_words(a[0], b[0], f"{label}, PIGS_LISTS_PRODUCT={product}: PIGS_STORE_THROUGH 1 against 0")
        same_outputs(a[1], b[1], f"{label}, PIGS_LISTS_PRODUCT={product}: PIGS_STORE_THROUGH 1 against 0")
    P, G = got["1", "1"], got["0", "1"]
    _, extra, same_points = same_lists(P[2], G[2], x, label, forward_only=True)
    assert same_points, label
    ranges = np.flatnonzero(G[0]["hdr"].reshape(-1, 8)[:, 0] >> 30 == PL.RANGES)
    wp, wg = written(P[0]), written(G[0])
    for k in ("hdr", "tlist"):           # a tile of record ranges: the header and the ranges, word for word
        assert np.array_equal(wp[k][ranges], wg[k][ranges]), (label, k)
    if extra == 0:
        same_words(P[0], G[0], f"{label}: PIGS_LISTS_PRODUCT 1 against 0")
        same_outputs(P[1], G[1], f"{label}: PIGS_LISTS_PRODUCT 1 against 0")
    return got, r


# ---- <1, ...>
def test_small_lattice(hip_lib):
    got, r = four_builds(hip_lib, lattice_scene(**SMALL), "64 x 64")
    snap = got["1", "1"][0]
    assert lattice_of(r.s._plan, hip_lib) == (64, 64) and modes(snap)[0] == 64
    d = distinct_per_block(snap)
    print(f"64 x 64: distinct Gaussians per block {d.min()} .. {d.max()}")
    assert (d <= 64).any()                                  # one step of a flush


def test_small_lattice_nan_and_near_singular_conics(hip_lib):
    x = lattice_scene(**SMALL)
    x["means"], x["conics"] = x["means"].copy(), x["conics"].copy()
    x["means"][5, 0] = np.nan
    a, c = x["conics"][7, 0], x["conics"][7, 2]
    x["conics"][7, 1] = round32(0.9999 * np.sqrt(a * c))               # rho = 0.9999
    got, _ = four_builds(hip_lib, x, "64 x 64, NaN and rho 0.9999", nan_gaussians=[5])
    snap = got["1", "1"][0]
    w = written(snap)
    listed = [t for t in range(snap["tiles"]) for g in range(4) if (w["glist"][t, g, :w["hdr"][t, 1 + g]] == 7).any()]
    assert listed, "the near-singular Gaussian is in no list"


# ---- <4, ...>
def test_large_lattice(hip_lib):
    got, r = four_builds(hip_lib, lattice_scene(**LARGE), "520 x 512")
    snap = got["1", "1"][0]
    assert snap["tiles"] == 4160 and modes(snap)[0] == 4160 and lattice_of(r.s._plan, hip_lib) == (520, 512)
    d = distinct_per_block(snap)
    print(f"520 x 512: distinct Gaussians per block {d.min()} .. {d.max()}")
    assert ((d > 64) & (d <= 128)).any()                    # two steps, the second partly empty


def test_large_lattice_wide_gaussians_several_flushes(hip_lib):
    got, _ = four_builds(hip_lib, lattice_scene(**LARGE_WIDE), "520 x 512, kappa 1.3")
    snap = got["1", "1"][0]
    assert snap["tiles"] == 4160 and modes(snap)[0] == 4160
    d = distinct_per_block(snap)
    print(f"520 x 512, kappa 1.3: distinct Gaussians per block {d.min()} .. {d.max()}")
    assert (d > 128).any()                                  # several flushes


# ---- a ragged last tile
def test_ragged_last_tile(hip_lib):
    x = lattice_scene(**dict(SMALL, nx=60, ny=60))
    got, r = four_builds(hip_lib, x, "60 x 60, ragged")
    B = got["1", "1"][2]
    assert B.lat == (0, 0) and len(x["pts"]) % 64 == 16 and ((B.groups[-1] >= 0).sum(1) == [16, 0, 0, 0]).all()
    assert not written(got["1", "1"][0])["hdr"][-1, 2:5].any()          # the empty groups list nothing


# ---- capacity
def capacity_scene(nx, ny):
    """a sparse lattice of Gaussians, and 600 more (sigma about 0.02) within 0.02 of one point: the groups within
    reach of it are handed more than list_cap = 512 entries, every other group a few dozen"""
    x = lattice_scene(nx=nx, ny=ny, gx=24, gy=24, kappa=0.5, seed=4)
    rng = np.random.default_rng(8)
    n = 600
    rad, th = 0.02 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    means = np.stack((-0.4 + rad * np.cos(th), 0.3 + rad * np.sin(th)), -1)
    s = 0.02 * np.exp(0.1 * rng.standard_normal(n))
    conics = np.stack((1 / s**2, np.zeros(n), 1 / s**2), -1)
    x["means"] = np.concatenate((x["means"], round32(means)))
    x["conics"] = np.concatenate((x["conics"], round32(conics)))
    x["values"] = np.concatenate((x["values"], round32(rng.uniform(-1, 1, (n, 1)))))
    return x


@pytest.mark.parametrize("nx,ny", [(64, 64), (520, 512)])
def test_group_lists_reach_capacity(hip_lib, nx, ny):
    got, _ = four_builds(hip_lib, capacity_scene(nx, ny), f"capacity {nx} x {ny}")
    snap = got["1", "1"][0]
    m = modes(snap)
    print(f"capacity {nx} x {ny}: list_cap {snap['cap']}, LIST / RANGES / GROUPS / POINTS {m.tolist()}")
    assert m[1] > 0 and m[0] > 0 and m[0] + m[1] == snap["tiles"]
    # (the tiles that fit: four_builds held their lists to the general build's and every build to the oracle)


# ---- full plans
@pytest.mark.parametrize("case", ["small", "large"])
def test_full_plan_keeps_its_lists(hip_lib, case):
    x = lattice_scene(**(SMALL if case == "small" else LARGE))
    fwd = Runs(x, True)
    with env("PIGS_LISTS_PRODUCT", "1"):
        fsnap, fouts = fwd.build(hip_lib, "1")
    full = Runs(x, False)
    built = {}
    for product in ("1", "0"):
        with env("PIGS_LISTS_PRODUCT", product):
            snap, outs = full.build(hip_lib, "1")
        meets_oracle(x, outs, f"{case}, full plan, PIGS_LISTS_PRODUCT={product}")
        built[product] = (snap, outs, Built(full.s, full.s._plan, hip_lib, x))
        structural(built[product][2], x, f"{case}, full plan, PIGS_LISTS_PRODUCT={product}", stride=1 if case == "small" else 32)
    same_lists(built["1"][2], built["0"][2], x, f"{case}, full plan")
    snap, outs, _ = built["1"]
    assert modes(snap)[0] == snap["tiles"]
    wf, wp = written(fsnap), written(snap)
    assert np.array_equal(wf["hdr"][:, 1:5], wp["hdr"][:, 1:5]) and np.array_equal(wf["glist"], wp["glist"]), case
    assert (wp["hdr"][:, 0] & ((1 << 30) - 1)).min() > 0 and not (wf["hdr"][:, 0] & ((1 << 30) - 1)).any()
    same_outputs(fouts, outs, f"{case}: forward-only against the full plan")
