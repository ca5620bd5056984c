"""GPU: the tile lists of the binned path (pigs_amd/csrc/plan_lists.h, grid_walk.h, the Gaussian half of plan_build.h)
against the brute-force oracle of oracle/plan_lists.py.

plan.h: "a (point, Gaussian) pair is evaluated iff the Gaussian's ellipse q <= q_max reaches the bounding box of the
point's 16-point group".  Every other test of the build is end-to-end at q_max = 36, where a pair at the cut-off carries
e^-18 = 1.5e-8 of its term's scale under bars of 1e-5: a build that lost the outer fifth of every ellipse would pass
them all.  Two layers here, on the scenes of tests/test_binned_matrix_gpu.py (which produce each tile mode and assert it):

STRUCTURAL.  A plan is read back (headers, tile lists, group lists, g2o; the sorted points through
pigs_samples_layout_info, or the index arithmetic of a lattice) and oracle.plan_lists.check_plan must find nothing:
every list holds every pair whose minimum q over the group's box is <= q (1 - DELTA) and none beyond q (1 + DELTA), for
the wide and the narrow cut-off, masks and group lists agree, ranges are disjoint and cover what the tile needs, ...
(the list in check_plan's docstring).  The pairs in between, the BAND, may go either way: they must stay below 1 % of
the must-have pairs of every plan.  DELTA = 2e-5 is four times the worst disagreement of the closed form in float32 and
in float64 on these scenes (tests/test_plan_lists.py measures it: 4.45e-6, scene G).

BEHAVIOURAL.  The same scenes with every conic divided by 9 and the sampler at q_max = Q / 9, q_max_backward =
(Q + 4) / 9, q_max_order3 = (Q + 8) / 9 (Q = 36, or 60 for scene P): the same ellipses, so the same lists and modes
(asserted), but a pair at the cut-off now carries e^-2 = 0.135 of its term's peak.  Outputs and gradients against
oracle/dense_numpy under oracle.plan_lists.pair_mask: the pairs each tile mode evaluates in each direction.

What plan.h's sentence does not say and the code deliberately does (written down there and in check_plan): a GROUPS
tile's group lists hold the wide set, so its forward evaluates pairs up to q_b; RANGES have no upper condition.

A finding of the behavioural layer, written down in plan.h and in pair_mask: which cut-off a backward takes is decided
by the instantiation that runs it, and a request runs its covering instantiation (launch.h, covering_mask_of) -- the
backward of sample((0, 1)) runs the (0, 1, 2) kernel and reads the WIDE masks (gradients 1.6e4 ... 1.9e5 of the bar
against a narrow mask, within it against the wide one); only order 0 or order 1 alone is narrow: sample((1,)) is here
for that.

Measured on an MI355X (28 tests, 18 s together, 2.5 s the longest), DELTA = 2e-5.  Structural layer, nothing found:
                                       q_f / q_b  LIST RANGES GROUPS POINTS  longest list  must-have pairs  band share
  L-lattice, orders 0..2               36 / 40      64    0      0      0        132            37 184      2.7e-5
  L-lattice, order 3                   44 / 44      64    0      0      0        143            41 560      4.8e-5
  L-sorted, orders 0..2                36 / 40      24    0      0      0        216            19 347      0
  L-sorted, order 3                    44 / 44      24    0      0      0        229            21 006      0
  R, orders 0..2                       36 / 40       0    7      0      0          -             4 590      0       ranges hold 1.07 x what they need
  R, order 3                           44 / 44       0    7      0      0          -             4 620      0       1.06 x
  G, orders 0..2                       36 / 40       2    1     13      0        500            27 887      0       1.11 x
  G, order 3                           44 / 44       2    1     13      0        502            28 100      0       1.11 x
  P, orders 0..2 / order 3             60 / 64, 68   0    0      0      8          -                 0      0
  L-lattice, strips                    36 / 40      64    0      0      0        132            37 184      2.7e-5
  L-sorted, strips                     36 / 40      24    0      0      0        205            19 269      0
  37 Gaussians, strips (72 x 72 pts)   36 / 40      81    0      0      0         21             7 497      0
  very wide Gaussians, strips          36 / 40       0   47      0      0          -            69 611      0       1.01 x
  L-sorted, points ordered             36 / 40      24    0      0      0        206            19 245      0
  L-sorted, points unordered           36 / 40      24    0      0      0        201            17 504      5.7e-5
  L-sorted, forward-only               36           22    0      0      2        151             8 565      0
  G, forward-only                      36           14    2      0      0        472            24 244      0       1.15 x
  L-sorted / R / G, fused first launch 36 / 40      as the ordinary builds; longest lists 223 / - / 496
  large, strips on and off             36 / 40    4160    0      0      0         97         2 178 259      3.7e-5
  (each build of L-sorted sorts the points anew -- ties in a cell fall differently --, hence its differing counts)
Behavioural layer, the worst error over its bar, forward / backward (c = 1, c = 2); band share at most 9.6e-5:
  L-lattice  list    0.052 / 0.057,  0.047 / 0.044        G  groups  0.163 / 0.752,  0.135 / 0.730
  L-sorted   list    0.050 / 0.282,  0.061 / 0.175        P  points  0.014 / 0.141,  0.021 / 0.145
  R          ranges  0.128 / 0.107,  0.114 / 0.176

It catches what it is for -- three value-only edits of plan_lists.h (which entries are written, never an address or a
loop bound), each built and run once, never committed; beside them what tests/test_binned_gpu.py,
test_binned_matrix_gpu.py and test_fuzz_gpu.py (111 tests) say under the same edit:
  (a) the group test of build_block_lists' flush compares against 0.8 q_f: 20 of the 28 tests here fail (every
      structural test with a LIST tile; the loud L and G scenes by 2e3 ... 2e4 of the bar; R and P, which hold no lists,
      pass).  The expectation that the existing tests see nothing is REFUTED for this edit: 14 of the 111 fail, by 1.0 to
      4.9 of their bars (q = 28.8 drops terms of 5.6e-7, a q^2 prefactor away from the 1e-5 bars).
  (b) the tile-list entry is written with gf and gm exchanged: 18 of the 28 tests here fail (every structural test of a
      plan with a tile list -- the forward-only plans, which have none, pass -- and the backward of the loud L and G
      scenes); none of the 111 existing tests fails.  CONFIRMED.
  (c) the GROUPS rebuild tests against a.q_f instead of pv.q_max: 4 of the 28 tests here fail, the four that hold GROUPS tiles: the
      ordinary build and the fused first launch of G (missing from the wide set) and G's loud scene for c = 1 and 2;
      none of the 111 existing tests fails.  CONFIRMED.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_binned_matrix_gpu as BM
from oracle import dense_numpy, plan_lists as PL
from test_binned_matrix_gpu import SCENES, assert_mode, geometry, headers, round32, seed_of
from host_program import covering as covering_mask      # covering_mask_of, asked of the library's own function
from test_dense_matrix_gpu import A0, A1, AL, Worst, np64
from test_plan_lists import STRIPS_CASES, strips_geometry

pytestmark = pytest.mark.gpu

FIVE = ("L-lattice", "L-sorted", "R", "G", "P")
BAND_SHARE = 0.01
TOL = BM.TOL


class env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


# ------------------------------------------------------------------------------------------
# reading a plan back
# ------------------------------------------------------------------------------------------
def words(ws, off, n):
    return ws[off:off + 4 * n].view(torch.int32).cpu().numpy().view(np.uint32)


def read_plan(plan, hip_lib):
    """hdr [tiles, 8], tlist [tiles, cap], glist [tiles, 4, cap], g2o [N] of a built plan"""
    info = (ctypes.c_int64 * 6)()
    assert hip_lib.pigs_plan_layout_info(plan.N, plan.M, plan.c, info) == 0
    tiles, cap, off_hdr, off_tlist, off_g2o, off_glist = (int(x) for x in info)
    torch.cuda.synchronize()
    ws = plan.workspace
    return (words(ws, off_hdr, 8 * tiles).reshape(tiles, 8), words(ws, off_tlist, tiles * cap).reshape(tiles, cap),
            words(ws, off_glist, tiles * 4 * cap).reshape(tiles, 4, cap), words(ws, off_g2o, plan.N))


def lattice_of(plan, hip_lib):
    off = hip_lib.pigs_samples_lattice_offset()
    return tuple(plan.samples.workspace[off:off + 8].view(torch.int32).cpu().tolist())


def strips_of(plan, hip_lib):
    off = hip_lib.pigs_plan_strips_offset()
    return int(plan.workspace[off:off + 4].view(torch.int32).cpu()[0])


def read_groups(plan, hip_lib, pts32=None):
    """groups_of() of the plan's samples workspace.  Sorted points: their m words must be a permutation of 0..M-1 and
    their coordinates bit-equal to the caller's (``pts32`` [M, 2] float32)."""
    lat = lattice_of(plan, hip_lib)
    if lat != (0, 0):
        return PL.groups_of(plan.M, lat), lat
    info = (ctypes.c_int64 * 4)()
    assert hip_lib.pigs_samples_layout_info(plan.M, info) == 0
    tiles, off, stride, zero = (int(x) for x in info)
    assert tiles == -(-plan.M // 64) and stride == 12 and zero == 0
    sp = words(plan.samples.workspace, off, 3 * plan.M).reshape(plan.M, 3)
    m = sp[:, 2].astype(np.int64)
    assert np.array_equal(np.sort(m), np.arange(plan.M)), "the sorted points' indices are no permutation of 0..M-1"
    if pts32 is not None:
        assert np.array_equal(sp[:, :2], np.ascontiguousarray(pts32, dtype=np.float32).view(np.uint32)[m]), \
            "a sorted point's coordinates are not the caller's"
    return PL.groups_of(plan.M, lat, m), lat


def structural(plan, hip_lib, means, con, pts, label, tiles=None, forward_only=False):
    """check_plan finds nothing; the band is small.  Prints the line of the table; returns the stats."""
    hdr, tlist, glist, g2o = read_plan(plan, hip_lib)
    groups, lat = read_groups(plan, hip_lib, pts)
    assert bool(plan.forward_only) == forward_only
    stats = {}
    found = PL.check_plan(hdr, tlist, glist, g2o, means, con, pts, groups, plan.q_max, plan.q_max_backward,
                          strips=strips_of(plan, hip_lib) == 1, forward_only=forward_only, tiles=tiles, stats=stats)
    share = stats["band"] / max(stats["must"], 1)
    ranges = f", ranges hold {stats['ranges_held'] / stats['ranges_needed']:.2f} x what they need" if stats["ranges_needed"] else ""
    print(f"{label}: q_f {plan.q_max:g} q_b {plan.q_max_backward:g} lattice {lat} strips {strips_of(plan, hip_lib)}: tiles in "
          f"LIST / RANGES / GROUPS / POINTS {stats['tiles']}, longest list {stats['longest']}, must-have pairs "
          f"{stats['must']}, band share {share:.2e}{ranges}")
    assert not found, (label, len(found), found[:8])
    assert stats["band"] <= BAND_SHARE * stats["must"], (label, stats)
    return stats


class Inputs:
    """float32-rounded inputs in float64 and their device tensors (fresh leaves)"""

    def __init__(self, means, con, pts, c=1, key="values"):
        values = np.random.default_rng(seed_of(key, len(means), c)).uniform(-1, 1, (len(means), c))
        self.means, self.con, self.values, self.pts = (round32(a) for a in (means, con, values, pts))
        self.N, self.M, self.c = len(means), len(pts), c

    def leaves(self):
        dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")
        self.t = [dev(self.means).requires_grad_(True), dev(self.values).requires_grad_(True),
                  dev(self.con).requires_grad_(True), dev(self.pts)]
        return self.t

    def bind(self, s):
        m, v, c, p = self.leaves()
        s.preprocess(m, v, None, c, p)
        assert s._plan is not None, "not the binned path"
        return s


def scene_inputs(name, c=1):
    return Inputs(*geometry(name), c=c, key=("values", name))


def sampler_for(name, **kw):
    from diff_gaussian_sampling import GaussianSampler
    q = SCENES[name][5] if name in SCENES else 36.0
    return GaussianSampler(True, backend="binned", fuse="none", q_max=q, **kw)


class NamedScene:
    """what assert_mode reads of a scene"""

    def __init__(self, name):
        self.name, self.mode, self.order, self.N, self.M, self.claims, self.q_max = (name,) + SCENES[name]


# ------------------------------------------------------------------------------------------
# the structural layer
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIVE)
def test_ordinary_builds(hip_lib, name):
    """The plan of orders (0, 1, 2) (two cut-offs: 36 / 40, scene P 60 / 64) and the order-3 plan (one: 44 / 68)."""
    x = scene_inputs(name)
    s = x.bind(sampler_for(name))
    s.sample((3,))                                # builds the order-3 plan
    assert s._plan3 is not None and s._plan3.q_max == s.q_max_order3
    for label, plan in (("orders 0..2", s._plan), ("order 3", s._plan3)):
        assert_mode(NamedScene(name), plan, hip_lib, s)
        st = structural(plan, hip_lib, x.means, x.con, x.pts, f"{name}, {label}")
        assert st["tiles"][BM.MODE_CODES[SCENES[name][0]]] > 0


@pytest.mark.parametrize("name", ("L-lattice", "L-sorted") + STRIPS_CASES)
def test_strips_builds(hip_lib, name):
    """PIGS_GAUSS_STRIPS=1: traverse_strips; g2o is the identity.  The two cases of tests/test_strips_gpu.py add a
    ragged strip and the RANGES branch with merged runs of strips."""
    x = scene_inputs(name) if name in SCENES else Inputs(*strips_geometry(name), key=("values", name))
    with env("PIGS_GAUSS_STRIPS", "1"):
        s = x.bind(sampler_for(name))
        assert strips_of(s._plan, hip_lib) == 1
        st = structural(s._plan, hip_lib, x.means, x.con, x.pts, f"{name}, strips")
    if name in SCENES:
        assert_mode(NamedScene(name), s._plan, hip_lib, s)
    if "record ranges" in name:
        assert st["tiles"][PL.RANGES] > 0, st


@pytest.mark.parametrize("order", ("ordered", "unordered"))
def test_both_sorts_of_the_points(hip_lib, order):
    """PIGS_SAMPLES_ORDER: the one-pass sort and the coarse-bin sort.  read_groups asserts that the m words are a
    permutation and the coordinates bit-equal to the caller's."""
    x = scene_inputs("L-sorted")
    with env("PIGS_SAMPLES_ORDER", order):
        s = x.bind(sampler_for("L-sorted"))
        assert lattice_of(s._plan, hip_lib) == (0, 0)
        structural(s._plan, hip_lib, x.means, x.con, x.pts, f"L-sorted, points {order}")
    assert_mode(NamedScene("L-sorted"), s._plan, hip_lib, s)


@pytest.mark.parametrize("name", ("L-sorted", "G"))
def test_forward_only_plans(hip_lib, name):
    """preprocess under no_grad (tests/test_forward_only_gpu.py): group lists under the one cut-off, LIST with count 0."""
    x = scene_inputs(name)
    s = sampler_for(name)
    with torch.no_grad():
        x.bind(s)
        assert s._plan.forward_only
        st = structural(s._plan, hip_lib, x.means, x.con, x.pts, f"{name}, forward-only", forward_only=True)
    assert st["tiles"][PL.GROUPS] == 0 and st["tiles"][PL.LIST] > 0


@pytest.mark.parametrize("name", ("L-sorted", "R", "G"))
def test_fused_first_launch(hip_lib, name, monkeypatch):
    """defer_lists=True and sample((0, 1, 2)) as the first call: plan_lists_forward_kernel builds the lists
    (build_block_lists<4> at these sizes; R's 7 tiles leave a ragged block of four).  The fused launch is taken as
    tests/test_binned_matrix_gpu.py::test_fused_first arranges it: PIGS_NO_FUSED_FIRST unset, and no plan of these sizes
    has held POINTS tiles."""
    monkeypatch.delenv("PIGS_NO_FUSED_FIRST", raising=False)
    x = scene_inputs(name)
    s = x.bind(sampler_for(name, defer_lists=True))
    s.sample((0, 1, 2))
    assert_mode(NamedScene(name), s._plan, hip_lib, s)
    structural(s._plan, hip_lib, x.means, x.con, x.pts, f"{name}, fused first launch")


@pytest.mark.parametrize("strips", ("1", "0"))
def test_the_large_scene(hip_lib, strips):
    """A 520 x 512 lattice of points in row order (4 160 tiles > LISTS_SMALL_TILES: plan_lists_kernel<4, strips>; ntx = 65,
    an odd tile-column count: the 1 x 4 blocks at the turning edge) under synthetic.lattice_gaussians(48, 40, 0.8).
    Every tile is checked: 32 M pairs."""
    from test_plan_lists import large_geometry
    x = Inputs(*large_geometry(), key=("values", "large"))
    with env("PIGS_GAUSS_STRIPS", strips):
        s = x.bind(sampler_for("large"))
        assert strips_of(s._plan, hip_lib) == int(strips)
        assert lattice_of(s._plan, hip_lib) == (520, 512)
        st = structural(s._plan, hip_lib, x.means, x.con, x.pts, f"large, strips {strips}")
    assert sum(st["tiles"]) == 4160 and st["tiles"][PL.LIST] == 4160


# ------------------------------------------------------------------------------------------
# the behavioural layer
# ------------------------------------------------------------------------------------------
SCALE = 9.0


class Loud:
    """A scene with every conic divided by 9 under cut-offs divided by 9: the same ellipses, loud at the cut-off."""

    def __init__(self, name, c):
        means, con, pts = geometry(name)
        self.name, self.c, self.Q = name, c, SCENES[name][5]
        self.x = Inputs(means, con / SCALE, pts, c=c, key=("values", name))
        self.full = dense_numpy.full_from_flat(self.x.con, 2)

    def sampler(self):
        from diff_gaussian_sampling import GaussianSampler
        Q = self.Q
        return GaussianSampler(True, backend="binned", fuse="none", q_max=Q / SCALE, q_max_backward=(Q + 4) / SCALE,
                               q_max_order3=(Q + 8) / SCALE)

    def forward(self, orders, mask, absolute=False):
        x = self.x
        return dense_numpy.forward(x.means, self.full, x.values, x.pts, orders=orders, pair_mask=mask, absolute=absolute)

    def backward(self, grads, mask, absolute=False):
        x = self.x
        gm, gc, gv = dense_numpy.backward(x.means, self.full, x.values, x.pts, grads, pair_mask=mask, absolute=absolute)
        return gm, dense_numpy.flat_grad_from_full(gc, 2), gv


def run_loud(hip_lib, name, c):
    from oracle import c_oracle
    sc = Loud(name, c)
    x, w, rng = sc.x, Worst("float32"), np.random.default_rng(seed_of("loud", name, c))
    s = sc.sampler()
    M, N = x.M, x.N
    bands = []

    def draw(shape):
        r = torch.as_tensor(rng.uniform(-1, 1, shape), dtype=torch.float32, device="cuda")
        return r, np64(r)

    def masks(plan, wide):
        """the forward's and the backward's (mask, band) on the plan that launched"""
        assert_mode(NamedScene(name), plan, hip_lib, s)
        mode = headers(plan, hip_lib)[0]
        groups, _ = read_groups(plan, hip_lib, x.pts)
        f = PL.pair_mask(mode, groups, x.means, x.con, x.pts, plan.q_max, plan.q_max_backward)
        b = PL.pair_mask(mode, groups, x.means, x.con, x.pts, plan.q_max, plan.q_max_backward, backward=True, wide=wide)
        for m_, b_ in (f, b):
            bands.append(b_.sum() / max(m_.sum(), 1))
            assert b_.sum() <= BAND_SHARE * m_.sum(), (name, c, int(b_.sum()), int(m_.sum()))
        return f, b

    def check_outputs(what, outs, want, mag):
        """within TOL of the largest output plus the band terms of that entry"""
        for o, got in outs.items():
            got = np64(got).reshape(want[o].shape)
            w.require(np.isfinite(got).all(), (what, o, "not finite"))
            bar = TOL * np.abs(want[o]).max() + mag[o]
            w.note(f"{SCENES[name][0]} forward", (what, "output", o), (np.abs(got - want[o]) / bar).max())

    def check_grads(what, got, grads, bmask, bband):
        want = sc.backward(grads, bmask)
        mag = sc.backward(grads, bband, absolute=True)
        _, bound = c_oracle.accumulation_bound(x.means, x.con, x.values, x.pts, grads)      # all pairs: slightly looser
        for k, nm in enumerate(("means", "conics", "values")):
            g = np64(got[k]).reshape(want[k].shape)
            w.require(np.isfinite(g).all(), (what, nm, "not finite"))
            w.note(f"{SCENES[name][0]} backward", (what, nm), (np.abs(g - want[k]) / (bound[k] + mag[k])).max())

    # ---- sample(): (0, 1, 2), wide backward; (0, 1, 2, 3) on the order-3 plan; (0, 1), whose backward runs the covering
    # instantiation (0, 1, 2) and is therefore wide as well; (1,), the narrow backward
    for orders in ((0, 1, 2), (0, 1, 2, 3), (0, 1), (1,)):
        x.bind(s)
        leaves = (x.t[0], x.t[2], x.t[1])
        outs = s.sample(orders)
        plan = s._plan3 if 3 in orders else s._plan
        (fm, fb), (bm, bb) = masks(plan, wide=covering_mask(sum(1 << o for o in orders)) & (4 | 8 | 16) != 0)
        check_outputs(orders, dict(zip(orders, outs)), sc.forward(orders, fm), sc.forward(orders, fb, absolute=True))
        r = {o: draw(tuple(out.shape)) for o, out in zip(orders, outs)}
        got = torch.autograd.grad(sum((out * r[o][0]).sum() for o, out in zip(orders, outs)), leaves)
        check_grads(orders, got, {o: r[o][1] for o in orders}, bm, bb)

    # ---- residual() with float coefficients: forward of orders 0, 1, trace; its backward reads the wide masks
    x.bind(s)
    leaves = (x.t[0], x.t[2], x.t[1])
    res = s.residual(a0=A0, a1=A1, lap=AL)
    (fm, fb), (bm, bb) = masks(s._plan, wide=True)
    compose = lambda e: A0 * e[0] + A1[0] * e[1][:, 0] + A1[1] * e[1][:, 1] + AL * (e[2][:, 0, 0] + e[2][:, 1, 1])
    mag = sc.forward((0, 1, 2), fb, absolute=True)
    mag = abs(A0) * mag[0] + abs(A1[0]) * mag[1][:, 0] + abs(A1[1]) * mag[1][:, 1] + abs(AL) * (mag[2][:, 0, 0] + mag[2][:, 1, 1])
    check_outputs("residual", {"residual": res}, {"residual": compose(sc.forward((0, 1, 2), fm))}, {"residual": mag})
    wr, wr64 = draw((M, c))
    got = torch.autograd.grad((res * wr).sum(), leaves)
    g1 = np.stack((A1[0] * wr64, A1[1] * wr64), 1)
    g2 = np.zeros((M, 2, 2, c))
    g2[:, 0, 0] = g2[:, 1, 1] = AL * wr64
    check_grads("residual", got, {0: A0 * wr64, 1: g1, 2: g2}, bm, bb)
    print(f"{name} c={c}: largest band share {max(bands):.2e}")
    w.report()


@pytest.mark.parametrize("name,c", [(n, c) for n in FIVE for c in (1, 2)], ids=[f"{n}-c{c}" for n in FIVE for c in (1, 2)])
def test_loud_cutoff(hip_lib, name, c):
    run_loud(hip_lib, name, c)
