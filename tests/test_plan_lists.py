"""CPU: the tile-list oracle and checker of oracle/plan_lists.py, before tests/test_plan_lists_gpu.py relies on them.

  * min_q_rect (0 inside, otherwise the least of four clamped edge parabolas) against a dense sampling of the rectangle
  * the Python restatement of the index-tiled order (plan.h: lattice_tile_xy, lattice_index)
  * check_plan finds nothing in a plan built from the oracle itself, and finds each planted defect where it was planted
  * DELTA, the half-width of the band in which float32 and float64 may disagree about a pair, is measured here
  * oracle/dense_numpy's pair_mask= against its own dense sums
"""
import numpy as np
import pytest

from oracle import dense_numpy, plan_lists as PL

Q_F, Q_B = 36.0, 40.0


# ------------------------------------------------------------------------------------------
# min_q_rect
# ------------------------------------------------------------------------------------------
def random_pairs(rng, n):
    """n ellipse / rectangle pairs, one rectangle per ellipse: widths over two decades, |rho| up to 0.99, a third of the
    rectangles a point or a segment, centres inside, beside and far from the rectangle."""
    sig = 10.0 ** rng.uniform(-2, 0, (n, 2))
    rho = rng.uniform(-0.99, 0.99, n)
    rho[: n // 20] = np.where(rng.random(n // 20) < 0.5, -0.99, 0.99)
    s0, s1 = sig[:, 0], sig[:, 1]
    det = (s0 * s1) ** 2 * (1 - rho ** 2)
    con = np.stack((s1 ** 2 / det, -rho * s0 * s1 / det, s0 ** 2 / det), -1)
    lo = rng.uniform(-1, 1, (n, 2))
    size = 10.0 ** rng.uniform(-2.5, 0, (n, 2))
    kind = rng.integers(0, 6, n)
    size[kind == 0] = 0.0                      # a point
    size[kind == 1, 0] = 0.0                   # a vertical segment
    size[kind == 2, 1] = 0.0                   # a horizontal segment
    boxes = np.concatenate((lo, lo + size), -1)
    where = rng.integers(0, 3, n)
    inside = lo + size * rng.uniform(0, 1, (n, 2))
    near = inside + sig * rng.normal(0, 4, (n, 2))
    far = inside + rng.uniform(-3, 3, (n, 2))
    means = np.where((where == 0)[:, None], inside, np.where((where == 1)[:, None], near, far))
    return means, con, boxes


def test_min_q_rect_against_a_sampled_minimum():
    """120 000 pairs.  The closed statement is never above the minimum over 65 x 17 samples of the rectangle (edges and
    corners included) and at most the sampling's resolution below it: the minimiser is a corner (a sample), or a point
    of an edge where q's derivative along the edge vanishes, or the centre -- in each case a sample lies within half a
    spacing (hx / 2, hy / 2) of it along the directions in which q is stationary, so the sampled minimum exceeds the
    true one by at most a (hx/2)^2 + 2 |b| (hx/2)(hy/2) + c (hy/2)^2."""
    rng = np.random.default_rng(11)
    n, nx, ny = 120_000, 65, 17
    means, con, boxes = random_pairs(rng, n)
    worst_above, worst_below, inside = 0.0, 0.0, 0
    for s in range(0, n, 4000):
        m, c, bx = means[s:s + 4000], con[s:s + 4000], boxes[s:s + 4000]
        closed = PL.min_q_rect(m, c, bx, paired=True)
        tx, ty = np.linspace(0, 1, nx), np.linspace(0, 1, ny)
        dx = (bx[:, 0, None] + (bx[:, 2] - bx[:, 0])[:, None] * tx - m[:, 0, None])[:, :, None]
        dy = (bx[:, 1, None] + (bx[:, 3] - bx[:, 1])[:, None] * ty - m[:, 1, None])[:, None, :]
        a, b, cc = (c[:, k, None, None] for k in range(3))
        sampled = (a * dx * dx + 2 * b * dx * dy + cc * dy * dy).reshape(len(m), -1).min(1)
        hx, hy = (bx[:, 2] - bx[:, 0]) / (nx - 1) / 2, (bx[:, 3] - bx[:, 1]) / (ny - 1) / 2
        res = c[:, 0] * hx * hx + 2 * np.abs(c[:, 1]) * hx * hy + c[:, 2] * hy * hy
        scale = np.maximum(sampled, 1.0)
        worst_above = max(worst_above, float(((closed - sampled) / scale).max()))
        worst_below = max(worst_below, float(((sampled - closed - res) / scale).max()))
        inside += int((closed == 0).sum())
    print(f"min_q_rect over {n} pairs: above the sampled minimum by {worst_above:.3g}, below it beyond the resolution by "
          f"{worst_below:.3g} (relative to max(q, 1)); {inside} centres inside")
    assert worst_above <= 1e-12 and worst_below <= 1e-12
    assert n // 5 < inside < n // 2


def test_min_q_rect_of_an_inverted_box_and_a_dense_table():
    rng = np.random.default_rng(12)
    means, con, boxes = random_pairs(rng, 300)
    boxes[7] = (np.inf, np.inf, -np.inf, -np.inf)
    full = PL.min_q_rect(means, con, boxes, chunk_pairs=1000)            # several chunks
    assert full.shape == (300, 300) and np.isinf(full[7]).all() and np.isfinite(np.delete(full, 7, 0)).all()
    assert np.array_equal(full, PL.min_q_rect(means, con, boxes))
    # a point rectangle: the pair's own q
    pts = rng.uniform(-1, 1, (50, 2))
    q = PL.min_q_rect(means, con, np.concatenate((pts, pts), -1))
    assert np.allclose(q, PL.pair_q(means, con, pts), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------
# the index-tiled order
# ------------------------------------------------------------------------------------------
def kernel_lattice_tile_xy(tile, ntx, nty):
    """plan.h, lattice_tile_xy, line by line (the oracle states the same order as a walk)"""
    pair, full = 2 * ntx, (nty >> 1) * 2 * ntx
    if tile < full:
        pr = tile // pair
        k = tile - pr * pair
        txs = k >> 1
        return (ntx - 1 - txs if pr & 1 else txs), 2 * pr + (k & 1)
    k = tile - full
    return (ntx - 1 - k if (nty >> 1) & 1 else k), nty - 1


@pytest.mark.parametrize("rf,rs", [(8, 8), (64, 64), (24, 40), (40, 24), (8, 200), (264, 8), (520, 512)])
def test_lattice_restatement(rf, rs):
    ntx, nty, M = rf // 8, rs // 8, rf * rs
    groups = PL.groups_of(M, (rf, rs))
    assert groups.shape == (M // 64, 4, 16)
    assert np.array_equal(np.sort(groups.reshape(-1)), np.arange(M))                     # a bijection
    row, col = groups // rf, groups % rf
    assert ((row.max(2) - row.min(2) == 3) & (col.max(2) - col.min(2) == 3)).all()       # every group a 4 x 4 patch
    assert (row.min(2) % 4 == 0).all() and (col.min(2) % 4 == 0).all()
    trow, tcol = row.reshape(-1, 64), col.reshape(-1, 64)
    assert ((trow.max(1) - trow.min(1) == 7) & (tcol.max(1) - tcol.min(1) == 7)).all()   # every tile 8 x 8
    txy = PL.lattice_tiles(ntx, nty)
    assert np.array_equal(txy[:, 0], tcol.min(1) // 8) and np.array_equal(txy[:, 1], trow.min(1) // 8)
    assert [tuple(t) for t in txy] == [kernel_lattice_tile_xy(t, ntx, nty) for t in range(ntx * nty)]
    full = (nty // 2) * 2 * ntx                 # tiles in pair-rows; an odd nty leaves one last row behind them
    columns = 0
    for t0 in range(0, full - 3, 4):
        w = txy[t0:t0 + 4, 0].max() - txy[t0:t0 + 4, 0].min() + 1
        h = txy[t0:t0 + 4, 1].max() - txy[t0:t0 + 4, 1].min() + 1
        assert (w, h) in ((2, 2), (1, 4)), (t0, txy[t0:t0 + 4].tolist())                 # 16 x 16 points, or 8 x 32
        if (w, h) == (1, 4):
            columns += 1
            assert ntx % 2 == 1 and txy[t0, 0] in (0, ntx - 1)                           # at the turning edge only
    assert columns == (0 if ntx % 2 == 0 else (nty // 2) // 2)
    last = txy[full:]
    assert len(last) == (ntx if nty % 2 else 0) and (last[:, 1] == nty - 1).all()
    assert (np.abs(np.diff(last[:, 0])) == 1).all()


# ------------------------------------------------------------------------------------------
# the checker checks
# ------------------------------------------------------------------------------------------
def cell_sorted(pts, per=16):
    """a permutation that puts the points of a square cell next to each other (about ``per`` points a cell)"""
    k = np.sqrt(len(pts) / per) / 2.0
    return np.lexsort((pts[:, 0], np.floor(pts[:, 0] * k), np.floor(pts[:, 1] * k)))


class SyntheticPlan:
    """A correct plan built from the oracle: six tiles -- LIST, LIST, GROUPS, RANGES, LIST and a ragged last LIST tile
    with one populated group --, Gaussians in a shuffled sorted order."""
    MODES = (PL.LIST, PL.LIST, PL.GROUPS, PL.RANGES, PL.LIST, PL.LIST)

    def __init__(self):
        rng = np.random.default_rng(5)
        self.N, self.M, self.cap = 240, 64 * 5 + 9, 240
        self.means = rng.uniform(-1, 1, (self.N, 2))
        sig = np.exp(rng.normal(-3.0, 0.4, (self.N, 2)))
        rho = rng.uniform(-0.9, 0.9, self.N)
        det = (sig[:, 0] * sig[:, 1]) ** 2 * (1 - rho ** 2)
        self.conics = np.stack((sig[:, 1] ** 2 / det, -rho * sig[:, 0] * sig[:, 1] / det, sig[:, 0] ** 2 / det), -1)
        self.points = rng.uniform(-1, 1, (self.M, 2))
        self.groups = PL.groups_of(self.M, (0, 0), cell_sorted(self.points))
        self.g2o = rng.permutation(self.N)
        o2g = np.argsort(self.g2o)
        gb = PL.group_boxes(self.points, self.groups)
        self.qmin = PL.min_q_rect(self.means, self.conics, gb.reshape(-1, 4)).reshape(6, 4, self.N)
        self.qtile = PL.min_q_rect(self.means, self.conics, PL.tile_boxes(gb))
        self.hdr = np.zeros((6, 8), dtype=np.uint32)
        self.tlist = np.zeros((6, self.cap), dtype=np.uint32)
        self.glist = np.zeros((6, 4, self.cap), dtype=np.uint32)
        for t, md in enumerate(self.MODES):
            wide, narrow = self.qmin[t] <= Q_B, self.qmin[t] <= Q_F
            if md == PL.RANGES:
                pos = np.sort(o2g[self.qtile[t] <= Q_B])
                cuts = np.flatnonzero(np.diff(pos) > 2) + 1               # runs of needed records, small gaps merged
                runs = [(r[0], r[-1] - r[0] + 1) for r in np.split(pos, cuts)]
                assert 2 <= len(runs) <= self.cap // 2
                self.tlist[t, :2 * len(runs)] = np.asarray(runs).reshape(-1)
                self.hdr[t, 0] = len(runs) | md << 30
                continue
            for g in range(4):
                lst = o2g[np.flatnonzero(wide[g] if md == PL.GROUPS else narrow[g])]
                self.glist[t, g, :len(lst)] = lst
                self.hdr[t, 1 + g] = len(lst)
            self.hdr[t, 0] = md << 30
            if md == PL.LIST:
                ns = np.flatnonzero(wide.any(0))
                wm = sum(wide[g, ns].astype(np.uint32) << g for g in range(4))
                nm = sum(narrow[g, ns].astype(np.uint32) << g for g in range(4))
                self.tlist[t, :len(ns)] = o2g[ns].astype(np.uint32) | wm << 24 | nm << 28
                self.hdr[t, 0] |= len(ns)
        band = (np.abs(self.qmin - Q_B) <= Q_B * PL.DELTA) | (np.abs(self.qmin - Q_F) <= Q_F * PL.DELTA)
        assert not band.any()                   # nothing in this scene is a matter of rounding

    def check(self, **kw):
        return PL.check_plan(self.hdr, self.tlist, self.glist, self.g2o, self.means, self.conics, self.points,
                             self.groups, Q_F, Q_B, **kw)

    def entry_of(self, t, n):
        idx, _, _ = PL.decode_entries(self.tlist[t, :self.hdr[t, 0] & PL.COUNT_MASK])
        return int(np.flatnonzero(self.g2o[idx] == n)[0])

    def pick(self, t, cond):
        """(group, Gaussian) of tile t with cond(qmin) true, the first such"""
        g, n = np.argwhere(cond(self.qmin[t]))[0]
        return int(g), int(n)


def reported(found, tile, group, gaussian, word):
    return any(f[1] == tile and f[2] == group and f[3] == gaussian and word in f[0] for f in found)


def test_the_checker_accepts_a_plan_built_from_the_oracle():
    p = SyntheticPlan()
    stats = {}
    assert p.check(stats=stats) == []
    assert stats["tiles"] == [4, 1, 1, 0] and stats["band"] == 0 and stats["must"] > 1000
    assert stats["ranges_held"] >= stats["ranges_needed"] > 0
    assert (p.groups[5, 1:] == -1).all() and (p.hdr[5, 2:5] == 0).all()          # the ragged tile
    assert p.check(tiles=[0, 3]) == []
    # a POINTS header and what breaks it
    p.hdr[4, :5] = (PL.POINTS << 30, 0, 0, 0, 0)
    assert p.check() == []
    p.hdr[4, 2] = 3
    assert reported(p.check(), 4, -1, -1, "POINTS")


def test_the_checker_accepts_forward_only_and_single_cutoff_plans():
    p = SyntheticPlan()
    p.hdr[:, 0] &= ~np.uint32(PL.COUNT_MASK) | np.where(np.array(p.MODES) == PL.LIST, 0, PL.COUNT_MASK).astype(np.uint32)
    p.hdr[2, 0] = PL.LIST << 30                          # a forward-only build has no GROUPS tile: narrow group lists
    for g in range(4):
        lst = np.argsort(p.g2o)[np.flatnonzero(p.qmin[2, g] <= Q_F)]
        p.glist[2, g, :len(lst)] = lst
        p.hdr[2, 1 + g] = len(lst)
    assert p.check(forward_only=True) == []
    p.tlist[0] = 0xFFFFFFFF                              # the tile list is not read
    assert p.check(forward_only=True) == []
    g, n = p.pick(1, lambda q: q <= Q_F / 2)
    k = int(np.flatnonzero(p.g2o[p.glist[1, g, :p.hdr[1, 1 + g]]] == n)[0])
    p.glist[1, g, k:-1] = p.glist[1, g, k + 1:].copy()
    p.hdr[1, 1 + g] -= 1
    assert reported(p.check(forward_only=True), 1, g, n, "missing")


DEFECTS = ("tile list entry removed", "group list entry removed", "far Gaussian added", "duplicate", "wide bit cleared",
           "masks swapped", "range shortened", "ranges overlap", "GROUPS tile keeps the narrow set", "g2o", "strips g2o")


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_checker_reports_a_planted_defect(defect):
    p = SyntheticPlan()
    cnt = lambda t: int(p.hdr[t, 0] & PL.COUNT_MASK)
    if defect == "tile list entry removed":
        g, n = p.pick(1, lambda q: q <= Q_F / 2)
        e = p.entry_of(1, n)
        p.tlist[1, e:cnt(1) - 1] = p.tlist[1, e + 1:cnt(1)].copy()
        p.hdr[1, 0] -= 1
        found = p.check()
        assert reported(found, 1, g, n, "missing from the wide") and reported(found, 1, g, n, "missing from the narrow")
        assert reported(found, 1, g, n, "without its narrow bit")
        assert {f[1] for f in found} == {1} and {f[3] for f in found} == {n}
    elif defect == "group list entry removed":
        g, n = p.pick(0, lambda q: q <= Q_F / 2)
        k = int(np.flatnonzero(p.g2o[p.glist[0, g, :p.hdr[0, 1 + g]]] == n)[0])
        p.glist[0, g, k:-1] = p.glist[0, g, k + 1:].copy()
        p.hdr[0, 1 + g] -= 1
        found = p.check()
        assert found and all(f[1:] == (0, g, n) and "without an entry in the group list" in f[0] for f in found)
    elif defect == "far Gaussian added":
        n = int(np.flatnonzero((p.qmin[4] > 4 * Q_B).all(0))[0])
        p.tlist[4, cnt(4)] = np.uint32(np.argsort(p.g2o)[n]) | np.uint32(1 << 2) << 24
        p.hdr[4, 0] += 1
        found = p.check()
        assert found and all(f[1:] == (4, 2, n) and "without reaching the group" in f[0] for f in found)
    elif defect == "duplicate":
        g, n = p.pick(0, lambda q: q <= Q_F / 2)
        p.tlist[0, cnt(0)] = p.tlist[0, p.entry_of(0, n)]
        p.hdr[0, 0] += 1
        found = p.check()
        assert found and all(f[1:] == (0, -1, n) and "duplicate in the tile list" in f[0] for f in found)
        q = SyntheticPlan()
        q.glist[2, 1, q.hdr[2, 2]] = q.glist[2, 1, 0]
        q.hdr[2, 2] += 1
        assert reported(q.check(), 2, 1, int(q.g2o[q.glist[2, 1, 0]]), "duplicate in the group list")
    elif defect == "wide bit cleared":
        g, n = p.pick(4, lambda q: q <= Q_F / 2)
        p.tlist[4, p.entry_of(4, n)] &= ~(np.uint32(1 << g) << 24)
        found = p.check()
        assert reported(found, 4, g, n, "narrow bit without its wide bit") and reported(found, 4, g, n, "missing from the wide")
        assert all(f[1:] == (4, g, n) for f in found)
    elif defect == "masks swapped":
        g, n = p.pick(0, lambda q: (q > Q_F * 1.01) & (q <= Q_B * 0.99))      # reaches under q_b = 40 only
        e = p.tlist[0, :cnt(0)]
        p.tlist[0, :cnt(0)] = (e & PL.IDX_MASK) | ((e >> 28) & 15) << 24 | ((e >> 24) & 15) << 28
        found = p.check()
        assert reported(found, 0, g, n, "narrow bit without its wide bit")
        assert reported(found, 0, g, n, "missing from the wide") and reported(found, 0, g, n, "in the narrow set without")
        assert {f[1] for f in found} == {0}
    elif defect == "range shortened":
        first, length = int(p.tlist[3, 2]), int(p.tlist[3, 3])                # the builder's runs end at a needed record
        n = int(p.g2o[first + length - 1])
        p.tlist[3, 3] -= 1
        found = p.check()
        assert found and all(f[1:] == (3, -1, n) and "no range holds it" in f[0] for f in found)
    elif defect == "ranges overlap":
        first, length = int(p.tlist[3, 0]), int(p.tlist[3, 1])
        p.tlist[3, 2 * cnt(3):2 * cnt(3) + 2] = (first + length - 1, 1)
        p.hdr[3, 0] += 1
        found = p.check()
        assert found and all(f[1:] == (3, -1, int(p.g2o[first + length - 1])) and "overlap" in f[0] for f in found)
    elif defect == "GROUPS tile keeps the narrow set":
        g, n = p.pick(2, lambda q: (q > Q_F * 1.01) & (q <= Q_B * 0.99))
        lst = np.argsort(p.g2o)[np.flatnonzero(p.qmin[2, g] <= Q_F)]
        p.glist[2, g, :len(lst)] = lst
        p.hdr[2, 1 + g] = len(lst)
        found = p.check()
        assert reported(found, 2, g, n, "missing from the wide") and all(f[1:3] == (2, g) for f in found)
    elif defect == "g2o":
        p.g2o[3] = p.g2o[4]
        assert [f[0] for f in p.check()] == ["g2o is no permutation of 0..N-1"]
    else:
        assert any("identity" in f[0] for f in p.check(strips=True))


# ------------------------------------------------------------------------------------------
# DELTA
# ------------------------------------------------------------------------------------------
STRIPS_CASES = ("37 Gaussians: one ragged strip", "very wide Gaussians (record ranges)")


def strips_geometry(name):
    """means, flat conics, points of a case of tests/test_strips_gpu.py, drawn as its test draws them"""
    from test_strips_gpu import CASES
    gauss, points = next((g, p) for n, g, p in CASES if n == name)
    rng = np.random.default_rng(41)
    means, con, _ = gauss(rng)
    return np.asarray(means), np.asarray(con), np.asarray(points(rng))


def large_geometry():
    """the large scene of tests/test_plan_lists_gpu.py: lattice Gaussians under a 520 x 512 lattice of points in row order"""
    from pigs_amd import synthetic
    gs = synthetic.lattice_gaussians(48, 40, 0.8)
    gx, gy = np.meshgrid(np.linspace(-1, 1, 520), np.linspace(-1, 1, 512), indexing="xy")
    return gs["means"].numpy(), gs["conics"].numpy(), np.stack((gx, gy), -1).reshape(-1, 2)


def test_delta_is_four_times_the_measured_disagreement():
    """grid_walk.h's closed form in numpy float32 (true division, no contraction) against the same in float64, on the
    float32-rounded inputs of every scene of tests/test_plan_lists_gpu.py -- the five of tests/test_binned_matrix_gpu.py,
    the two strips cases and the large lattice -- against the boxes of 16 cell-sorted points (the lattice: of its 4 x 4
    index patches), over the pairs whose minimum q lies in [q_max / 2, 2 q_max].  The device adds v_rcp_f32's 1 ulp
    and FMA contraction, which this emulation has not: hence the factor four."""
    from test_binned_matrix_gpu import SCENES, geometry, round32
    worst = {}
    for name in ("L-lattice", "L-sorted", "R", "G", "P") + STRIPS_CASES + ("large",):
        geo = geometry(name) if name in SCENES else large_geometry() if name == "large" else strips_geometry(name)
        means, con, pts = (round32(a) for a in geo)
        q_max = SCENES[name][5] if name in SCENES else 36.0
        if name == "large":
            boxes = PL.group_boxes(pts, PL.groups_of(len(pts), (520, 512))[::7]).reshape(-1, 4)
        else:
            boxes = PL.group_boxes(pts, PL.groups_of(len(pts), (0, 0), cell_sorted(pts))).reshape(-1, 4)
        boxes = boxes[boxes[:, 0] <= boxes[:, 2]]
        q64 = PL.closed_form_min_q(means, con, boxes, np.float64)
        q32 = PL.closed_form_min_q(means, con, boxes, np.float32).astype(np.float64)
        sel = (q64 >= q_max / 2) & (q64 <= 2 * q_max)
        rel = np.abs(q32 - q64)[sel] / q64[sel]
        k = np.argwhere(sel)[rel.argmax()]
        a, b, c = con[k[1]]
        worst[name] = (float(rel.max()), int(sel.sum()), float(b / np.sqrt(a * c)))
        # and the closed form is the oracle's independent statement (float64 against float64)
        ind = PL.min_q_rect(means, con, boxes)
        assert np.abs(q64 - ind)[sel].max() <= 1e-9 * q_max, name
    for name, (w, n, rho) in worst.items():
        print(f"{name}: float32 against float64 over {n} pairs: {w:.3g} relative (the worst pair's b / sqrt(a c) = {rho:.4f})")
    measured = max(w for w, _, _ in worst.values())
    print(f"measured {measured:.3g}; DELTA = {PL.DELTA:g} = {PL.DELTA / measured:.2f} x")
    assert PL.DELTA >= 4 * measured
    assert PL.DELTA <= 16 * measured, "DELTA is wider than the measurement warrants: measure again and write it down"


# ------------------------------------------------------------------------------------------
# pair_mask and the masked oracle
# ------------------------------------------------------------------------------------------
def test_pair_mask_per_mode_and_direction():
    p = SyntheticPlan()
    mode = np.array([PL.LIST, PL.GROUPS, PL.RANGES, PL.POINTS, PL.LIST, PL.LIST])
    qpair = PL.pair_q(p.means, p.conics, p.points)
    table = {}
    for backward, wide in ((False, False), (True, False), (True, True)):
        mask, band = PL.pair_mask(mode, p.groups, p.means, p.conics, p.points, Q_F, Q_B, backward=backward, wide=wide)
        assert mask.shape == band.shape == (p.M, p.N) and not band.any()
        table[backward, wide] = mask
        for t in range(6):
            for g in range(4):
                mem = p.groups[t, g][p.groups[t, g] >= 0]
                cut = Q_B if mode[t] == PL.GROUPS or (backward and wide) else Q_F
                for m in mem[:3]:
                    want = (qpair[m] if mode[t] == PL.POINTS else p.qmin[t, g]) <= cut
                    assert np.array_equal(mask[m], want), (t, g, backward, wide)
    assert np.array_equal(table[False, False], table[True, False])
    assert (table[True, True] >= table[True, False]).all() and (table[True, True] != table[True, False]).any()
    assert (table[False, False] >= (qpair <= Q_F)).all()          # a point's own pairs are always inside


def test_the_masked_oracle_zeroes_the_unmasked_pairs():
    rng = np.random.default_rng(3)
    N, M, c = 23, 41, 2
    means, pts, values = rng.uniform(-1, 1, (N, 2)), rng.uniform(-1, 1, (M, 2)), rng.uniform(-1, 1, (N, c))
    A = rng.normal(size=(N, 2, 2))
    con = A @ A.transpose(0, 2, 1) + np.eye(2)
    full = dense_numpy.forward(means, con, values, pts)
    gr = {o: rng.normal(size=full[o].shape) for o in full}
    everything = np.ones((M, N), dtype=bool)
    for o, out in dense_numpy.forward(means, con, values, pts, pair_mask=everything).items():
        assert np.allclose(out, full[o], rtol=1e-12, atol=1e-12)
    for a, b in zip(dense_numpy.backward(means, con, values, pts, gr, pair_mask=everything),
                    dense_numpy.backward(means, con, values, pts, gr)):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12)
    # a random mask: pair by pair through the dense sums of 1 x 1 problems
    mask = rng.random((M, N)) < 0.3
    mask[5] = False
    mask[:, 7] = False
    got_f = dense_numpy.forward(means, con, values, pts, pair_mask=mask)
    got_b = dense_numpy.backward(means, con, values, pts, gr, pair_mask=mask)
    abs_f = dense_numpy.forward(means, con, values, pts, pair_mask=mask, absolute=True)
    abs_b = dense_numpy.backward(means, con, values, pts, gr, pair_mask=mask, absolute=True)
    want_f = {o: np.zeros_like(full[o]) for o in full}
    mag_f = {o: np.zeros_like(full[o]) for o in full}
    want_b = [np.zeros((N, 2)), np.zeros((N, 2, 2)), np.zeros((N, c))]
    mag_b = [np.zeros((N, 2)), np.zeros((N, 2, 2)), np.zeros((N, c))]
    for m, n in np.argwhere(mask):
        one = dense_numpy.forward(means[n:n + 1], con[n:n + 1], values[n:n + 1], pts[m:m + 1])
        for o in one:
            want_f[o][m] += one[o][0]
            mag_f[o][m] += np.abs(one[o][0])
        back = dense_numpy.backward(means[n:n + 1], con[n:n + 1], values[n:n + 1], pts[m:m + 1],
                                    {o: gr[o][m:m + 1] for o in gr})
        for k in range(3):
            want_b[k][n] += back[k][0]
            mag_b[k][n] += np.abs(back[k][0])
    for o in full:
        assert np.allclose(got_f[o], want_f[o], rtol=1e-12, atol=1e-12) and not got_f[o][5].any()
        assert np.allclose(abs_f[o], mag_f[o], rtol=1e-12, atol=1e-12)
    for k in range(3):
        assert np.allclose(got_b[k], want_b[k], rtol=1e-12, atol=1e-12) and not got_b[k][7].any()
        assert np.allclose(abs_b[k], mag_b[k], rtol=1e-12, atol=1e-12)
