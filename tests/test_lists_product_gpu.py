"""GPU: the product path of the list build's flush (pigs_amd/csrc/plan_lists.h, ellipse_rect.h) against the general
path, the brute-force list oracle (oracle/plan_lists.py) and the float64 dense oracle (oracle/c_oracle).

A block whose 4 TPW group boxes are the product of x- and y-intervals tests every survivor of the walk against all its
groups at once, from shared axis terms; every other block keeps the per-tile filter and the group tests.  Both form
bit-identical minima for the same (ellipse, box); the product path drops only the tile pre-filter.  Every case is built
twice in one process, PIGS_LISTS_PRODUCT = 1 and = 0 (PIGS_GAUSS_STRIPS = 1 in both: one kind of walk, so one order of
the entries), and

  * both plans are held against check_plan at the bar of tests/test_plan_lists_gpu.py (nothing found, band <= 1 % of
    the must-have pairs); plans of more than a few hundred tiles on every STRIDE-th tile -- the comparison below
    covers every tile;
  * group lists and tile lists of the two builds are equal ENTRY FOR ENTRY (same order).  The exception: an entry, or a
    mask bit, present only in the product build must have a float64 minimum q over its group box within 1e-5 q of its
    cut-off (the tile test failed by rounding where the group test passed), and at most 1 in 10^4 entries of a case
    may be such; an entry present only in the general build is an error;
  * outputs on <= 2 048 sampled points against c_oracle at 1e-5; one backward on a full plan within
    grads_within_accumulation_bound; forward-only and full plans of cases 1 and 2 give bit-equal outputs;
  * which blocks ARE products is restated here from the float32 boxes (product_blocks): all of them in cases 1 and 2,
    all but the moved ones in case 3, none in case 4.  The kernel's own decision is not read back: with every block
    rejected the two builds run the same code, and with a block accepted that should not be, its lists would be wrong
    and check_plan would say so.

Measured on an MI355X (8 tests, 7.3 s together): nothing found by check_plan in any build; 0 entries in the product
build alone in 7.3 M compared (case 2 at kappa = 1.3 alone 3.5 M, a median of 183 entries in a block's longest group
list); outputs against c_oracle 0.8e-7 ... 5.3e-7; forward-only and full plans bit-equal.  Points that the build sorts
(case 4, random and ragged) fall into their cells differently at every build: 0 of 313 and 1 of 65 tiles held the same
points in both builds, so those two cases rest on check_plan and the oracle, not on the comparison.
"""
import numpy as np
import pytest
import torch

from conftest import grads_within_accumulation_bound
from oracle import c_oracle, plan_lists as PL
from pigs_amd import synthetic
from test_binned_matrix_gpu import round32
from test_plan_lists_gpu import BAND_SHARE, env, lattice_of, read_groups, read_plan, strips_of

pytestmark = pytest.mark.gpu

SAMPLED = 2048
EXTRA_REL = 1e-5        # an entry of the product build alone: |min q - cut| <= EXTRA_REL * cut in float64
EXTRA_SHARE = 1e-4      # ... and at most this share of a case's entries


def lattice_points(nx, ny, angle=0.0):
    gx, gy = np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-1, 1, ny), indexing="xy")
    p = np.stack((gx, gy), -1).reshape(-1, 2)
    if angle:
        c, s = np.cos(angle), np.sin(angle)
        p = p @ np.array([[c, s], [-s, c]]) / (abs(c) + abs(s))      # rotated, still inside [-1, 1]^2
    return p


def gaussians(nx, ny, kappa, seed, c=1):
    gs = synthetic.lattice_gaussians(nx, ny, kappa, seed=seed, c=c)
    return [round32(gs[k].numpy()) for k in ("means", "conics", "values")]


def product_blocks(pts32, groups, tpw):
    """[blocks] bool: the kernel's product test restated on the float32 boxes.  Group g of tile t of a block sits in
    column 2 (t >> 1) + (g & 1) and row 2 (t & 1) + (g >> 1); a product: every group holds a point, a column's groups
    have bit-equal x0 and x1, a row's bit-equal y0 and y1."""
    gb = PL.group_boxes(pts32.astype(np.float64), groups).astype(np.float32)        # exact: min / max of float32 values
    tiles = gb.shape[0]
    nb = -(-tiles // tpw)
    pad = np.full((nb * tpw, 4, 4), np.nan, dtype=np.float32)
    pad[:tiles] = gb
    pad = pad.reshape(nb, tpw, 4, 4)
    ok = np.isfinite(pad).all((1, 2, 3))
    t, g = np.arange(tpw)[:, None], np.arange(4)[None, :]
    col, row = 2 * (t >> 1) + (g & 1), 2 * (t & 1) + (g >> 1)
    bits = np.nan_to_num(pad, nan=0.0, posinf=0.0, neginf=0.0).view(np.uint32)
    for axis, where in ((0, col), (1, row)):
        for k in range(int(where.max()) + 1):
            sel = bits[:, where == k]                      # [blocks, groups of this column / row, 4]
            for comp in (axis, axis + 2):
                ok &= (sel[:, :, comp] == sel[:, :1, comp]).all(1)
    return ok


class Built:
    def __init__(self, s, plan, hip_lib, x):
        self.plan = plan
        self.hdr, self.tlist, self.glist, self.g2o = read_plan(plan, hip_lib)
        self.groups, self.lat = read_groups(plan, hip_lib, x["pts"])
        self.strips = strips_of(plan, hip_lib)


def build(hip_lib, x, product, forward_only=False, orders=(0, 1, 2), backward=False):
    """One build under PIGS_LISTS_PRODUCT = product; returns (Built, outputs, gradients or None)."""
    from diff_gaussian_sampling import GaussianSampler
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")
    m, c, v, p = dev(x["means"]), dev(x["conics"]), dev(x["values"]), dev(x["pts"])
    s = GaussianSampler(True, backend="binned", fuse="none", q_max=x.get("q_max", 36.0))
    grads = None
    with env("PIGS_LISTS_PRODUCT", "1" if product else "0"), env("PIGS_GAUSS_STRIPS", "1"):
        if forward_only:
            with torch.no_grad():
                s.preprocess(m, v, None, c, p)
                outs = s.sample(orders)
        else:
            for t in (m, c, v):
                t.requires_grad_(True)
            s.preprocess(m, v, None, c, p)
            outs = s.sample(orders)
            if backward:
                rng = np.random.default_rng(11)
                rs = [rng.uniform(-1, 1, tuple(o.shape)).astype(np.float32) for o in outs]
                got = torch.autograd.grad(sum((o * dev(r)).sum() for o, r in zip(outs, rs)), (m, c, v))
                grads = (got, {o: r.astype(np.float64) for o, r in zip(orders, rs)})
        torch.cuda.synchronize()
    assert s._plan is not None and bool(s._plan.forward_only) == forward_only
    return Built(s, s._plan, hip_lib, x), [o.detach() for o in outs], grads


def structural(b, x, label, stride=1, forward_only=False):
    tiles = None if stride == 1 else range(0, b.hdr.shape[0], stride)
    stats = {}
    found = PL.check_plan(b.hdr, b.tlist, b.glist, b.g2o, x["means"], x["conics"], x["pts"], b.groups, b.plan.q_max,
                          b.plan.q_max_backward, strips=b.strips == 1, forward_only=forward_only, tiles=tiles, stats=stats)
    print(f"{label}: lattice {b.lat} strips {b.strips}: tiles in LIST / RANGES / GROUPS / POINTS {stats['tiles']}, longest list "
          f"{stats['longest']}, must-have pairs {stats['must']}, band share {stats['band'] / max(stats['must'], 1):.2e}")
    assert not found, (label, len(found), found[:8])
    assert stats["band"] <= BAND_SHARE * stats["must"], (label, stats)
    return stats


def same_lists(P, G, x, label, forward_only=False):
    """The product build P against the general build G, entry for entry; returns (entries, extras, every tile compared)."""
    assert np.array_equal(P.g2o, G.g2o) and P.lat == G.lat
    modeP, countP, ngP = PL.decode_headers(P.hdr)
    modeG, countG, ngG = PL.decode_headers(G.hdr)
    assert np.array_equal(modeP, modeG), label
    cap = P.tlist.shape[1]
    listed = (modeG == PL.LIST) | (modeG == PL.GROUPS)
    entries = int(ngG[listed].sum()) + (0 if forward_only else int(countG[modeG == PL.LIST].sum()))
    gboxes = PL.group_boxes(x["pts"], P.groups)
    q_f, q_b = float(P.plan.q_max), float(P.plan.q_max if forward_only else P.plan.q_max_backward)
    extras = []                      # (tile, group, sorted Gaussian, cut-off)

    def diff(t, g, lp, lg, cut):
        """lp must be lg with a few entries more, in the same order"""
        keep = np.isin(lp, lg)
        assert np.array_equal(lp[keep], lg), (label, "an entry of the general build is missing or out of order", t, g)
        extras.extend((t, g, int(j), cut) for j in lp[~keep])

    col = np.arange(cap)
    same_g = (ngP == ngG).all(1) & (np.where(col < ngP[:, :, None], P.glist, 0) == np.where(col < ngG[:, :, None], G.glist, 0)).all((1, 2))
    same_t = (countP == countG) & (np.where(col < countP[:, None], P.tlist, 0) == np.where(col < countG[:, None], G.tlist, 0)).all(1)
    # (points that the build sorted fall into their cells in another order at every build: such a tile is compared only
    # where both builds grouped the same points; a lattice's tiles are index arithmetic, all of them are compared)
    same_points = (P.groups == G.groups).all((1, 2))
    if P.lat != (0, 0):
        assert same_points.all()
    print(f"{label}: {int(same_points.sum())} of {len(same_points)} tiles hold the same points in both builds")
    for t in np.flatnonzero(listed & same_points & ~(same_g & (same_t | forward_only | (modeG != PL.LIST)))):
        for g in range(4):
            diff(t, g, P.glist[t, g, :ngP[t, g]].astype(np.int64), G.glist[t, g, :ngG[t, g]].astype(np.int64), q_f)
        if forward_only or modeG[t] != PL.LIST:
            continue
        ip, wp, npp = PL.decode_entries(P.tlist[t, :countP[t]])
        ig, wg, ngg = PL.decode_entries(G.tlist[t, :countG[t]])
        keep = np.isin(ip, ig)
        assert np.array_equal(ip[keep], ig), (label, "a tile-list entry of the general build is missing or out of order", t)
        assert not (wg & ~wp[keep]).any() and not (ngg & ~npp[keep]).any(), (label, "a mask bit of the general build is missing", t)
        more_w, more_n = wp.copy(), npp.copy()
        more_w[keep] &= ~wg
        more_n[keep] &= ~ngg
        for g in range(4):
            extras.extend((t, g, int(j), q_b) for j in ip[(more_w >> g & 1) == 1])
            extras.extend((t, g, int(j), q_f) for j in ip[(more_n >> g & 1) == 1])
    for t, g, j, cut in extras:
        n = P.g2o[j]
        q = PL.min_q_rect(x["means"][n:n + 1], x["conics"][n:n + 1], gboxes[t, g][None], paired=True)[0]
        assert abs(q - cut) <= EXTRA_REL * cut, (label, "an entry of the product build alone is not at the cut-off", t, g, int(n), q, cut)
    print(f"{label}: {entries} entries, {len(extras)} in the product build alone")
    assert len(extras) <= EXTRA_SHARE * entries, (label, len(extras), entries)
    return entries, len(extras), bool(same_points.all())


def outputs_match_oracle(x, outs, label, orders=(0, 1, 2)):
    M = len(x["pts"])
    idx = np.unique(np.random.default_rng(5).integers(0, M, SAMPLED)) if M > SAMPLED else np.arange(M)
    exp = c_oracle.forward(x["means"], x["conics"], x["values"], x["pts"][idx], orders=orders)
    for o, out in zip(orders, outs):
        got = out.cpu().double().numpy()[idx]
        err = np.abs(got - exp[o].reshape(got.shape)).max() / np.abs(exp[o]).max()
        print(f"{label}: order {o} against c_oracle on {len(idx)} points: {err:.2e}")
        assert err < 1e-5, (label, o, err)


def both(hip_lib, x, label, expect, stride=1, forward_only=False, backward=False, oracle=True):
    """The case built with the product path and without; ``expect``: 'all' / 'none' / a function of the product flags."""
    P, outP, gradP = build(hip_lib, x, True, forward_only=forward_only, backward=backward)
    G, outG, _ = build(hip_lib, x, False, forward_only=forward_only)
    tpw = 4 if P.hdr.shape[0] > 4096 else 1                # build_choice.h, LISTS_SMALL_TILES
    flags = product_blocks(x["pts"].astype(np.float32), P.groups, tpw)
    print(f"{label}: {int(flags.sum())} of {len(flags)} blocks of {tpw} tile(s) are products")
    if expect == "all":
        assert flags.all(), label
    elif expect == "none":
        assert not flags.any(), label
    else:
        expect(flags)
    structural(P, x, f"{label}, product", stride, forward_only)
    structural(G, x, f"{label}, general", stride, forward_only)
    _, extra, same_points = same_lists(P, G, x, label, forward_only)
    if oracle:
        outputs_match_oracle(x, outP, label)
    if extra == 0 and same_points:
        for a, b in zip(outP, outG):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (label, "same lists, other outputs")
    if backward:
        got, rs = gradP
        bad = grads_within_accumulation_bound(got, (x["means"], x["conics"], x["values"], x["pts"]), rs)
        assert not bad, (label, bad)
    return P, outP


def scene(pts, nx, ny, kappa, seed, **kw):
    m, c, v = gaussians(nx, ny, kappa, seed)
    return dict(means=m, conics=c, values=v, pts=round32(pts), **kw)


LARGE = (520, 512)          # 4 160 tiles > LISTS_SMALL_TILES: four tiles per wave


def straddling(lat):
    """[blocks] bool: with an odd count of tile columns (65 here) the block at every second turning edge of the
    serpentine is a 1 x 4 column of tiles, not 2 x 2: no product under the kernel's arrangement -- the general path"""
    txy = PL.lattice_tiles(lat[0] // 8, lat[1] // 8)
    return txy[0::4, 1] != txy[2::4, 1]


def all_but_straddling(flags):
    assert np.array_equal(flags, ~straddling(LARGE)) and straddling(LARGE).sum() == 16


# ---- case 1: TPW = 1, a product of 2 x 2
def test_small_lattice_full_and_forward_only(hip_lib):
    x = scene(lattice_points(64, 64), 32, 32, 0.5, seed=1)
    _, full = both(hip_lib, x, "case 1, full plan", "all", backward=True)
    _, fwd = both(hip_lib, x, "case 1, forward-only", "all", forward_only=True)
    for a, b in zip(full, fwd):
        assert torch.equal(a, b)


# ---- case 2: TPW = 4, a product of 4 x 4
def test_large_lattice_full_and_forward_only(hip_lib):
    x = scene(lattice_points(*LARGE), 128, 128, 0.5, seed=2)
    P, full = both(hip_lib, x, "case 2, full plan", all_but_straddling, stride=32)
    assert P.lat == LARGE and P.hdr.shape[0] == 4160
    _, fwd = both(hip_lib, x, "case 2, forward-only", all_but_straddling, stride=32, forward_only=True)
    for a, b in zip(full, fwd):
        assert torch.equal(a, b)


def test_large_lattice_wide_gaussians_several_flushes(hip_lib):
    """kappa = 1.3 on a 64 x 64 lattice of Gaussians: more than 128 survivors per block (SURV_CAP), several flushes."""
    x = scene(lattice_points(*LARGE), 64, 64, 1.3, seed=3)
    P, _ = both(hip_lib, x, "case 2, kappa 1.3", all_but_straddling, stride=8)
    _, _, ng = PL.decode_headers(P.hdr)
    per_block = ng.reshape(-1, 16).max(1)                  # a block's survivors are at least its longest group list
    print(f"case 2, kappa 1.3: longest group list per block: median {np.median(per_block):.0f}, max {per_block.max()}")
    assert np.median(per_block) > 128


# ---- case 3: product and general blocks side by side
def test_moved_points_mix_the_paths(hip_lib):
    pts = lattice_points(*LARGE)
    groups = PL.groups_of(len(pts), LARGE)
    moved = np.arange(0, groups.shape[0], 37)
    pts[groups[moved, 1, 7], 0] += 0.25 * 2.0 / (LARGE[0] - 1)          # a quarter of the spacing along x, a point of the group's right edge
    x = scene(pts, 128, 128, 0.5, seed=2)

    def expect(flags):
        want = ~straddling(LARGE)
        want[np.unique(moved // 4)] = False
        assert np.array_equal(flags, want)

    P, _ = both(hip_lib, x, "case 3", expect, stride=32)
    assert P.lat == LARGE


# ---- case 4: the general path only
def test_rotated_lattice_is_no_product(hip_lib):
    x = scene(lattice_points(*LARGE, angle=0.3), 48, 40, 0.8, seed=4)
    both(hip_lib, x, "case 4, rotated", "none", stride=8)


def test_random_points_are_no_product(hip_lib):
    pts = np.random.default_rng(6).uniform(-1, 1, (20000, 2))
    both(hip_lib, scene(pts, 48, 40, 0.8, seed=4), "case 4, random", "none", stride=2)


def test_ragged_last_tile_is_no_product(hip_lib):
    """4 097 points: the last tile holds one point, three of its groups none"""
    pts = np.random.default_rng(7).uniform(-1, 1, (4097, 2))
    P, _ = both(hip_lib, scene(pts, 48, 40, 0.8, seed=4), "case 4, ragged", "none")
    assert (P.groups[-1] >= 0).sum() == 1


# ---- case 5: degenerate conics
def test_nan_and_near_singular_conics_alike(hip_lib):
    x = scene(lattice_points(64, 64), 32, 32, 0.5, seed=1)
    x["conics"] = x["conics"].copy()
    x["conics"][5] = np.nan
    a, c = x["conics"][7, 0], x["conics"][7, 2]
    x["conics"][7, 1] = round32(0.9999 * np.sqrt(a * c))               # rho = 0.9999
    P, _ = both(hip_lib, x, "case 5", "all", oracle=False)      # (outputs: bit-equal between the builds, NaN included)
    # both accept the NaN conic wherever the walk hands it over, and the near-singular one is listed on both paths alike
    where = np.flatnonzero(P.g2o == 5)[0]
    _, _, ng = PL.decode_headers(P.hdr)
    assert any((P.glist[t, g, :ng[t, g]] == where).any() for t in range(P.hdr.shape[0]) for g in range(4))
