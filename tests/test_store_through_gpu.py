"""GPU: the write-through stores of the list launch (pigs_amd/csrc/plan.h, store_through; PIGS_STORE_THROUGH) change
how a word leaves the compute unit, never which word goes where.

Every case is built twice in one process, PIGS_STORE_THROUGH = 1 and = 0, and read back through pigs_plan_layout_info /
pigs_plan_records_info.  With = 1 the headers and group lists of a forward-only build of more than LISTS_SMALL_TILES
tiles leave by `sc0 sc1` vector stores (plan_lists_kernel<4, STRIPS, true, true>: the two large forward-only cases
below, strips and cells, lists and record ranges); every other build takes the plain instantiation under either
setting -- the strips pack, full plans and small point sets had such stores while this was built and lost them again
 -- and its cases hold the setting to changing nothing there.

  * hdr, glist, tlist, rec, pbox, sbox and g2o of the two builds are equal WORD FOR WORD -- every word a build writes:
    the five header words of a tile, a list up to the length its header states (record ranges: two words each), all
    records with the zero record N, every strip and super-strip box, the whole way back.  (A plan's workspace is fresh
    memory at every preprocess, so what lies behind a list's end is nobody's.)  Both builds read the same sorted points
    (one sampler, the samples half reused: points that a build sorts fall into their cells differently at every build,
    tests/test_plan_lists_gpu.py).  Builds that keep the caller's order (PIGS_GAUSS_STRIPS=1) are deterministic to the
    word: one wave per block of tiles, entries in ballot order.  The one build through the cells ranks the Gaussians of
    a cell by atomics, so it is compared in the form that does not depend on the ranks: records and lists mapped
    through g2o to the caller's indices, every list sorted;
  * the outputs of orders 0-2 are bit-equal between the two builds (the same lists in the same order: the same sums);
    between two builds through the cells, whose lists hold the same entries in another order, within 2e-6 of the
    largest entry (the bar of tests/test_strips_gpu.py for one order of the entries against another);
  * the outputs of EVERY build meet the float64 dense oracle (oracle/c_oracle) at 1e-5 of the largest entry, the bar
    of tests/test_binned_gpu.py, on at most 2 048 sampled points -- which also says that neither build left its arrays
    as it found them.

Cases: the 64 x 64 lattice of points over 16 x 16 lattice Gaussians at kappa = 0.5 forward-only (product path,
plan_lists_kernel<1, ...>) and as a full plan (tile list, wide masks); kappa = 1.3 (every tile meets more than SURV_CAP
= 128 survivors: several flushes); 72 x 64 points; 4 096 uniform random points (general flush); scenes R and G of
tests/test_binned_matrix_gpu.py as full plans (a list that overflows: RANGES; a tile list that overflows while the
group lists fit under two cut-offs: the GROUPS rebuild) -- both asserted from the headers; one build through the cells
(PIGS_GAUSS_STRIPS=0: plan_lists_kernel<..., false, ...>, the walk through the cells); one defer_lists=True forward (the fused launch
keeps plain stores whatever the setting) against the two-launch result.  And, beyond the issue's list, the 520 x 512
lattice of tests/test_lists_product_gpu.py (4 160 tiles > LISTS_SMALL_TILES), forward-only and full, strips and cells:
the only way to plan_lists_kernel<4, ...>, the kernel of the headline step; and the same points under 24 x 24 Gaussians
so wide that every group list overflows: the record ranges of that kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import c_oracle
from pigs_amd import synthetic
from test_binned_matrix_gpu import geometry, round32
from test_plan_lists_gpu import env, lattice_of, strips_of, words

pytestmark = pytest.mark.gpu

ORDERS = (0, 1, 2)
TOL = 1e-5              # tests/test_binned_gpu.py
SAMPLED = 2048
FUSED_REL = 2e-6        # another order of a list's entries: tests/test_strips_gpu.py, strips against cells


def lattice_points(nx, ny):
    gx, gy = np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-1, 1, ny), indexing="xy")
    return np.stack((gx, gy), -1).reshape(-1, 2)


def lattice_scene(nx, ny, gx, gy, kappa, seed):
    gs = synthetic.lattice_gaussians(gx, gy, kappa, seed=seed, c=1)
    m, c, v = (round32(gs[k].numpy()) for k in ("means", "conics", "values"))
    return dict(means=m, conics=c, values=v, pts=round32(lattice_points(nx, ny)))


def named_scene(name):
    means, con, pts = geometry(name)
    values = np.random.default_rng(17).uniform(-1, 1, (len(means), 1))
    return dict(means=round32(means), conics=round32(con), values=round32(values), pts=round32(pts))


def offsets(plan, hip_lib):
    info, rec = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 4)()
    assert hip_lib.pigs_plan_layout_info(plan.N, plan.M, plan.c, info) == 0
    assert hip_lib.pigs_plan_records_info(plan.N, plan.M, plan.c, rec) == 0
    tiles, cap, off_hdr, off_tlist, off_g2o, off_glist = (int(x) for x in info)
    N = plan.N
    return {"hdr": (off_hdr, 8 * tiles), "tlist": (off_tlist, tiles * cap), "glist": (off_glist, tiles * 4 * cap),
            "g2o": (off_g2o, N), "rec": (int(rec[0]), 8 * (N + 1)), "pbox": (int(rec[1]), 4 * (-(-N // 16))),
            "sbox": (int(rec[2]), 4 * (-(-N // 256)))}, tiles, cap


def snapshot(plan, hip_lib):
    torch.cuda.synchronize()
    off, tiles, cap = offsets(plan, hip_lib)
    got = {k: words(plan.workspace, o, n).copy() for k, (o, n) in off.items()}
    got["tiles"], got["cap"], got["strips"] = tiles, cap, strips_of(plan, hip_lib)
    return got


def written(snap):
    """the words of a snapshot that its build wrote, by array"""
    tiles, cap = snap["tiles"], snap["cap"]
    hdr = snap["hdr"].reshape(tiles, 8)[:, :5]
    mode, count, ng = hdr[:, 0] >> 30, (hdr[:, 0] & ((1 << 30) - 1)).astype(np.int64), hdr[:, 1:5].astype(np.int64)
    col = np.arange(cap)
    tl_len = np.where(mode == 0, count, np.where(mode == 1, 2 * count, 0))
    assert (tl_len <= cap).all() and (ng <= cap).all()
    listed = ((mode == 0) | (mode == 2))[:, None, None]
    out = {"hdr": hdr, "tlist": np.where(col < tl_len[:, None], snap["tlist"].reshape(tiles, cap), 0),
           "glist": np.where(listed & (col < ng[:, :, None]), snap["glist"].reshape(tiles, 4, cap), 0),
           "rec": snap["rec"], "g2o": snap["g2o"]}
    if snap["strips"]:
        out["pbox"], out["sbox"] = snap["pbox"], snap["sbox"]
    return out


class Runs:
    """one sampler and one set of device tensors for every build of a case"""

    def __init__(self, x, forward_only, strips="1", **kw):
        from diff_gaussian_sampling import GaussianSampler
        dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")
        self.m, self.c, self.v, self.p = dev(x["means"]), dev(x["conics"]), dev(x["values"]), dev(x["pts"])
        self.forward_only, self.strips = forward_only, strips
        if not forward_only:
            for t in (self.m, self.c, self.v):
                t.requires_grad_(True)
        self.s = GaussianSampler(True, backend="binned", fuse="none", q_max=x.get("q_max", 36.0), reuse_samples=True, **kw)

    def preprocess(self):
        if self.forward_only:
            with torch.no_grad():
                self.s.preprocess(self.m, self.v, None, self.c, self.p)
        else:
            self.s.preprocess(self.m, self.v, None, self.c, self.p)
        assert self.s._plan is not None and bool(self.s._plan.forward_only) == self.forward_only

    def build(self, hip_lib, through):
        with env("PIGS_STORE_THROUGH", through), env("PIGS_GAUSS_STRIPS", self.strips):
            self.preprocess()
            snap = snapshot(self.s._plan, hip_lib)
            with torch.no_grad():
                outs = [o.detach().clone() for o in self.s.sample(ORDERS)]
            torch.cuda.synchronize()
        assert snap["strips"] == int(self.strips)
        return snap, outs


ARRAYS = ("hdr", "glist", "tlist", "rec", "pbox", "sbox", "g2o")


def same_words(a, b, label):
    wa, wb = written(a), written(b)
    assert set(wa) == set(wb) == set(ARRAYS), label
    for k in ARRAYS:
        diff = np.flatnonzero(wa[k].ravel() != wb[k].ravel())
        assert diff.size == 0, (label, k, int(diff.size), diff[:8].tolist())


def canonical(snap, forward_only):
    """what does not depend on the rank a build through the cells gave a Gaussian inside its cell"""
    g2o = snap["g2o"].astype(np.int64)
    tiles, cap = snap["tiles"], snap["cap"]
    hdr = snap["hdr"].reshape(tiles, 8)
    mode, count, ng = hdr[:, 0] >> 30, hdr[:, 0] & ((1 << 30) - 1), hdr[:, 1:5]
    assert np.isin(mode, (0, 2)).all()
    glist, tlist = snap["glist"].reshape(tiles, 4, cap), snap["tlist"].reshape(tiles, cap)
    lists = [[np.sort(g2o[glist[t, g, :ng[t, g]]]) for g in range(4)] for t in range(tiles)]
    tl = []
    if not forward_only:
        for t in range(tiles):
            e = tlist[t, :count[t]].astype(np.int64)
            full = g2o[e & ((1 << 24) - 1)] | (e >> 24 << 24)
            tl.append(np.sort(full))
    rec = snap["rec"].reshape(-1, 8)
    order = np.argsort(g2o, kind="stable")
    assert np.array_equal(g2o[order], np.arange(len(g2o)))
    return mode, ng, lists, tl, rec[:-1][order], rec[-1]


def same_canonical(a, b, forward_only, label):
    ca, cb = canonical(a, forward_only), canonical(b, forward_only)
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]), label
    for t in range(len(ca[2])):
        for g in range(4):
            assert np.array_equal(ca[2][t][g], cb[2][t][g]), (label, t, g)
    for t in range(len(ca[3])):
        assert np.array_equal(ca[3][t], cb[3][t]), (label, t)
    assert np.array_equal(ca[4], cb[4]) and np.array_equal(ca[5], cb[5]), (label, "records")


def same_outputs(a, b, label):
    for o, (u, w) in enumerate(zip(a, b)):
        assert torch.equal(u.view(torch.int32), w.view(torch.int32)), (label, "order", o)


def same_outputs_up_to_order(a, b, label):
    """two builds through the cells: the same lists, their entries in the order of the ranks that atomics gave the
    Gaussians of a cell in each build -- the same terms summed in another order (FUSED_REL)"""
    for o, (u, w) in enumerate(zip(a, b)):
        ref = w.cpu().double().numpy()
        err = np.abs(u.cpu().double().numpy() - ref).max() / np.abs(ref).max()
        print(f"{label}: order {o}, one build against the other: {err:.2e}")
        assert err < FUSED_REL, (label, "order", o, err)


def meets_oracle(x, outs, label):
    M = len(x["pts"])
    idx = np.unique(np.random.default_rng(5).integers(0, M, SAMPLED)) if M > SAMPLED else np.arange(M)
    exp = c_oracle.forward(x["means"], x["conics"], x["values"], x["pts"][idx], orders=ORDERS)
    for o, out in zip(ORDERS, outs):
        got = out.cpu().double().numpy()[idx]
        err = np.abs(got - exp[o].reshape(got.shape)).max() / np.abs(exp[o]).max()
        print(f"{label}: order {o} against c_oracle on {len(idx)} points: {err:.2e}")
        assert err < TOL, (label, o, err)


def modes(snap):
    return np.bincount(snap["hdr"].reshape(-1, 8)[:, 0] >> 30, minlength=4)


def both(hip_lib, x, label, forward_only, strips="1", settings=("1", "0")):
    r = Runs(x, forward_only, strips)
    first = None
    for through in settings:
        snap, outs = r.build(hip_lib, through)
        meets_oracle(x, outs, f"{label}, PIGS_STORE_THROUGH={through}")
        if first is None:
            first = (snap, outs)
            continue
        if strips == "1":
            same_words(first[0], snap, f"{label}, {settings[0]} against {through}")
        else:
            same_canonical(first[0], snap, forward_only, f"{label}, {settings[0]} against {through}")
        (same_outputs if strips == "1" else same_outputs_up_to_order)(first[1], outs, f"{label}, {settings[0]} against {through}")
    print(f"{label}: tiles {first[0]['tiles']}, LIST / RANGES / GROUPS / POINTS {modes(first[0]).tolist()}, "
          f"lattice {lattice_of(r.s._plan, hip_lib)}, group-list entries {int(first[0]['hdr'].reshape(-1, 8)[:, 1:5].sum())}")
    return r, first


SMALL = dict(nx=64, ny=64, gx=16, gy=16, kappa=0.5, seed=1)


def test_small_lattice_forward_only(hip_lib):
    """the product path of plan_lists_kernel<1, true, true, THROUGH>"""
    x = lattice_scene(**SMALL)
    r, (snap, _) = both(hip_lib, x, "64 x 64, forward-only", True)
    assert lattice_of(r.s._plan, hip_lib) == (64, 64) and modes(snap)[0] == 64
    assert np.array_equal(snap["g2o"], np.arange(256))
    assert not (snap["hdr"].reshape(-1, 8)[:, 0] & ((1 << 30) - 1)).any()      # a forward-only plan writes no tile list


def test_small_lattice_full_plan(hip_lib):
    """the tile list and its wide masks"""
    x = lattice_scene(**SMALL)
    _, (snap, _) = both(hip_lib, x, "64 x 64, full plan", False)
    count = snap["hdr"].reshape(-1, 8)[:, 0] & ((1 << 30) - 1)
    assert modes(snap)[0] == 64 and count.min() > 0 and (written(snap)["tlist"] >> 24).any()


def test_wide_gaussians_several_flushes(hip_lib):
    x = lattice_scene(**dict(SMALL, kappa=1.3, seed=3))
    _, (snap, _) = both(hip_lib, x, "64 x 64, kappa 1.3", True)
    # a tile's survivors are at least the Gaussians its four group lists name: more than SURV_CAP = 128 of them means
    # more than one flush -- in the tiles of the interior (a tile at the domain's edge meets about half as many)
    w = written(snap)
    named = np.array([len(np.unique(np.concatenate([w["glist"][t, g, :n] for g, n in enumerate(w["hdr"][t, 1:5])])))
                      for t in range(snap["tiles"])])
    print(f"64 x 64, kappa 1.3: Gaussians named by a tile's group lists: median {np.median(named):.0f}, max {named.max()}, "
          f"{int((named > 128).sum())} of {len(named)} tiles above 128")
    assert (named > 128).sum() >= len(named) // 4


def test_72_by_64_points(hip_lib):
    x = lattice_scene(**dict(SMALL, nx=72))
    r, (snap, _) = both(hip_lib, x, "72 x 64", True)
    assert snap["tiles"] == 72


def test_random_points_general_flush(hip_lib):
    x = lattice_scene(**SMALL)
    x["pts"] = round32(np.random.default_rng(6).uniform(-1, 1, (4096, 2)))
    r, _ = both(hip_lib, x, "4 096 random points", True)
    assert lattice_of(r.s._plan, hip_lib) == (0, 0)


def test_ranges_and_groups_rebuild(hip_lib):
    """scenes R and G of tests/test_binned_matrix_gpu.py as full plans of strips: a tile whose lists overflow keeps
    record ranges; one whose tile list overflows while its group lists fit is rebuilt with the wide cut-off"""
    _, (snap, _) = both(hip_lib, named_scene("R"), "scene R", False)
    assert modes(snap)[1] > 0, modes(snap)
    _, (snap, _) = both(hip_lib, named_scene("G"), "scene G", False)
    assert modes(snap)[2] > 0, modes(snap)


def test_build_through_the_cells(hip_lib):
    """PIGS_GAUSS_STRIPS=0: the list launch walks the cells (plan_lists_kernel<1, false, false, THROUGH>)"""
    x = lattice_scene(**SMALL)
    both(hip_lib, x, "64 x 64 through the cells, full plan", False, strips="0")


def test_large_lattice_four_tiles_per_wave(hip_lib):
    """520 x 512 points, 4 160 tiles > LISTS_SMALL_TILES: plan_lists_kernel<4, true, FWD_ONLY>, the headline's kernels"""
    x = lattice_scene(nx=520, ny=512, gx=128, gy=128, kappa=0.5, seed=2)
    for forward_only in (True, False):
        r, (snap, _) = both(hip_lib, x, f"520 x 512, forward_only={forward_only}", forward_only)
        assert snap["tiles"] == 4160 and modes(snap)[0] == 4160 and lattice_of(r.s._plan, hip_lib) == (520, 512)


def test_large_lattice_through_the_cells(hip_lib):
    """plan_lists_kernel<4, false, true, THROUGH>"""
    x = lattice_scene(nx=520, ny=512, gx=128, gy=128, kappa=0.5, seed=2)
    _, (snap, _) = both(hip_lib, x, "520 x 512 through the cells, forward-only", True, strips="0")
    assert snap["tiles"] == 4160 and modes(snap)[0] == 4160


def test_large_lattice_record_ranges(hip_lib):
    """576 Gaussians that all reach every group: no group list fits its 512 entries, every tile keeps record ranges"""
    x = lattice_scene(nx=520, ny=512, gx=24, gy=24, kappa=10.0, seed=4)
    _, (snap, _) = both(hip_lib, x, "520 x 512, wide Gaussians", True)
    assert snap["tiles"] == 4160 and modes(snap)[1] == 4160, modes(snap)


def test_deferred_lists_against_two_launches(hip_lib, monkeypatch):
    """defer_lists=True: the first forward builds the lists in its own launch (plan_lists_forward_kernel, which keeps
    plain stores: its waves read their lists back) -- the same lists up to the order of their entries, the same
    outputs up to the order of the sums"""
    monkeypatch.delenv("PIGS_NO_FUSED_FIRST", raising=False)
    x = lattice_scene(**SMALL)
    two = Runs(x, False)
    want, outs2 = two.build(hip_lib, "1")
    one = Runs(x, False, defer_lists=True)
    with env("PIGS_STORE_THROUGH", "1"), env("PIGS_GAUSS_STRIPS", "1"):
        one.preprocess()
        with torch.no_grad():
            outs1 = [o.detach().clone() for o in one.s.sample(ORDERS)]
        got = snapshot(one.s._plan, hip_lib)
    same_canonical(want, got, False, "deferred lists")
    meets_oracle(x, outs1, "deferred lists")
    for o, (a, b) in enumerate(zip(outs1, outs2)):
        ref = b.cpu().double().numpy()
        err = np.abs(a.cpu().double().numpy() - ref).max() / np.abs(ref).max()
        print(f"deferred lists: order {o} against the two-launch result: {err:.2e}")
        assert err < FUSED_REL, (o, err)
