"""GPU: every instantiation of the binned kernels (pigs_amd/csrc/plan_forward.h and plan_backward.h:
tile_forward_kernel<C, MASK> and tile_backward_kernel<C, MASK>, 23 per direction, and the five plan_lists_forward_kernel<C, MASK> of the fused first
launch) through every tile mode a header word can carry -- LIST, GROUPS, RANGES, POINTS -- against the float64 oracle.

A scene is Gaussians, points and the tile mode they must produce; it is built for c = 1 and c = 2 with the same geometry,
and it asserts from the tile headers of the plan that launched (s._plan3 for orders containing 3, vorticity_terms() and
vorticity_residual(); s._plan otherwise) that the mode is there: a scene that stops producing its mode fails, it does not
test LIST again.  tests/test_binned_matrix.py reads SCENES, RUNS and FUSED_FIRST_CALLS without a GPU and derives that no
(c, mask, mode, direction) cell is left out.

The scenes (N Gaussians x M points; the sizes were tuned on an MI355X from the list build's thresholds, plan.h and
build_block_lists of plan_lists.h; the tile counts are those of that run, the plans of both cut-offs alike unless noted):
  L-lattice  576 x 4 096    synthetic.grid_samples(64): the smallest index-tiled point set; all 64 tiles LIST; streamed stores
  L-sorted   600 x 1 481    random points (sorted into cells: plain stores, the staging records for c = 1) and Gaussians
                            wide enough for group lists of up to 149 entries (five 32-record chunks) and tile lists of up
                            to 221 (four backward steps, a second half of rows); all 24 tiles LIST; M % 64 = 9: the last
                            tile has one populated group of four
  R          700 x 401      close points under Gaussians of widths over a decade, most of which reach every point: the
                            group lists overflow list_cap = 512 and all 7 tiles keep record ranges, three or four each,
                            of lengths such as 4, 9, 686.  The fallback to the single range {0, N} is not reached (the
                            scene asserts that): a plan of 700 Gaussians has fewer ranges than a slab holds pairs.  With
                            one width for all (log-normal, sigma 0.3) every tile's ranges are the one range {0, 700}
                            of the only occupied level, which the sampling kernels cannot tell from the fallback.
  G          3 300 x 1 003  300 domain-wide Gaussians and 3 000 narrow ones in shuffled order: a tile list overflows
                            where its four group lists (up to 507 entries) fit, and the wide ones sit in coarse levels
                            whose 3 x 3 cells are most of the plan (walk_candidates > 4 x the longest list), so the tiles
                            do not go to the per-point walk: 13 of 16 tiles GROUPS (12 under the order-3 cut-off for
                            c = 2), the rest LIST and RANGES
  P          1 100 x 509    narrow Gaussians (G0 = 32, about ten per point), uniform points: every tile spans a hundred
                            finest cells and goes to the per-point walk unlisted, all 8 tiles POINTS; M % 4 = 1: the last
                            quad has three invalid rows
  P-stride   4 100 x 4 417  70 tiles; at this size a list wave builds one tile, whose box spans 46 finest cells (G0 = 64):
                            fewer than the 64 that send a block to the walk unlisted, more than the 16 that send a tile
                            there whose group lists exceed 96 entries, which they do: 69 tiles POINTS, so the 1 024
                            helper waves come round a second time (16 quads a tile).  The trip does not depend on the
                            template: c = 1 orders (0, 1, 2) and c = 2 vorticity_residual() only.  17 M pairs: the two
                            runs take 0.3 s each.

Per (scene, c) one test runs, each call on a fresh preprocess and differentiated: the order sets of
tests/test_dense_matrix_gpu.py (all eight covering masks, requests with holes, a loss that reads only (1, 3)),
residual() with floats (32), with fields without and with advection (64), and for c = 2 the coupled residual (256),
vorticity_terms() (128) and vorticity_residual() with a per-point tau and a previous level (512).  fuse="none": single
orders launch their own instantiations.  One more test per scene (not P-stride) makes each of the five fused first
launches the first call on a plan with deferred lists.

Bars, all the project's own: float32 outputs within TOL = 1e-5 (tests/test_binned_gpu.py) of the largest output -- of
the term scale for the coupled residual, of the column scales for the two vorticity outputs, as their own files have
it; gradients per entry within conftest.grads_within_accumulation_bound's bound (ulps = floor = 1e-6), the magnitudes
summed over an order set's orders; the general residual with advection against its own composition
(tests/test_residual_terms_gpu.py).

The cut-off.  The per-point walk tests every pair against q_max itself, where the lists keep whatever reaches a group's
box: the P scenes truncate exactly at the cut-off, and with about five points per Gaussian nothing hides it.  At the
default q_max = 36 P's gradients were at 2.09 of their bar (order 1, conics); the same inputs through the dense HIP
kernel at 0.19 and through the binned path with q_max = 60 at 0.21: the cut-off, not the kernel, so P and P-stride run
with q_max = 60 (backward 64, order 3 68).  The truncation has its own tests (tests/test_binned_gpu.py, test_fuzz_gpu.py).
The conditioning.  With test_binned_gpu.random_gaussians' correlations (tanh(N(0, 0.7))) the P scenes missed the gradient
bar at either cut-off by up to 3.5 -- and so did the dense kernel on the same inputs: the worst entry belonged to a
Gaussian with rho = -0.989 and three points inside q < 36 (dense 1.29 / 1.67 / 1.25 of the bar for means / conics /
values, binned 1.72 / 1.64 / 1.24).  That is float32 on x^T C x (tests/test_conditioning_gpu.py), not indexing: the P
scenes draw |rho| < 0.9 as the dense matrix does (narrow_gaussians).

Measured on an MI355X, the worst error as a fraction of its bar over the 17 tests (4.8 s together); no case needed
another bar:
                 forward   backward   fused first   backward after it
  list           0.114     0.846      0.040         0.568
  groups         0.194     0.889      0.118         0.345
  ranges         0.168     0.188      0.102         0.331
  points         0.033     0.269      0.017         0.221
  general residual with advection against its own composition: forward 5.9e-8 of the term scale (bar 2e-6), gradients
  4.1e-7 of the largest entry (bar 5e-6)
The matrix catches what it is for -- three value-only edits of plan_forward.h, one run each, never committed:
  (a) forward_points_quad tests q against a quarter of the cut-off: the forward cells of P and P-stride fail (both
      channel counts, every order set and fused output, 33 outputs) and P's fused first launches, and with them the
      gradients of vorticity_residual() there, whose backward reads the record that forward left; nothing else.
  (b) for_each_step's GROUPS branch hands group g's entries to group g ^ 1: the backward cells of G fail (c = 1 and 2,
      and the backward after G's fused first launches); nothing else.
  (c) the record-range queue stores 0 for the second channel's value: the c = 2 forward cells of R fail and those of G
      (one or two of its tiles keep ranges), with the c = 2 fused first launch of both; no c = 1 cell, no backward cell.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import host_program as hp
from test_dense_matrix_gpu import Case, ORDER_SETS, Worst, A0, A1, AL, np64, out_shape

pytestmark = pytest.mark.gpu

# ---- the case list: plain data (tests/test_binned_matrix.py reads it without a GPU)
# name: (intended tile mode, point order, N, M, what the scene claims beyond its mode, q_max)
Q_DEFAULT, Q_POINTS = 36.0, 60.0
SCENES = {
    "L-lattice": ("list", "lattice", 576, 4096, (), Q_DEFAULT),
    "L-sorted": ("list", "sorted", 600, 1481, ("ragged tile",), Q_DEFAULT),
    "R": ("ranges", "sorted", 700, 401, (), Q_DEFAULT),
    "G": ("groups", "sorted", 3300, 1003, (), Q_DEFAULT),
    "P": ("points", "sorted", 1100, 509, ("ragged quad",), Q_POINTS),
    "P-stride": ("points", "sorted", 4100, 4417, ("ragged quad", "second trip"), Q_POINTS),
}
RESIDUAL_KINDS = ("linear residual", "fields", "fields + advection")           # masks 32, 64, 64
C2_KINDS = ("coupled residual", "vorticity_terms", "vorticity_residual")       # masks 256, 128, 512
KIND_MASKS = {"linear residual": 32, "fields": 64, "fields + advection": 64, "coupled residual": 256,
              "vorticity_terms": 128, "vorticity_residual": 512}
# (scene, c, order sets, fused kinds)
RUNS = [(name, c, tuple(ORDER_SETS), RESIDUAL_KINDS + (C2_KINDS if c == 2 else ()))
        for name in ("L-lattice", "L-sorted", "R", "G", "P") for c in (1, 2)]
RUNS += [("P-stride", 1, (((0, 1, 2), None),), ()), ("P-stride", 2, (), ("vorticity_residual",))]
# the first call on a plan with deferred lists: (c, orders of a sample() call, or "linear residual")
FUSED_FIRST_CALLS = [(1, (0,)), (1, (0, 1, 2)), (1, (0, 1, "lap")), (1, "linear residual"), (2, (0, 1, 2))]
FUSED_FIRST_SCENES = ("L-lattice", "L-sorted", "R", "G", "P")

TOL = 1e-5                                    # tests/test_binned_gpu.py
MODE_CODES = {"list": 0, "ranges": 1, "groups": 2, "points": 3}     # plan.h TILE_MODE_*


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def round32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def narrow_gaussians(rng, N, sigma):
    """Means uniform in [-1, 1]^2, standard deviations sigma e^N(0, 0.1) per axis, correlations uniform in (-0.9, 0.9) as
    tests/test_dense_matrix_gpu.py problem() draws them.  (test_binned_gpu.random_gaussians draws tanh(N(0, 0.7)): one
    in a hundred beyond 0.95, where float32 loses digits of x^T C x -- tests/test_conditioning_gpu.py.  Under hundreds
    of points per Gaussian that disappears in the accumulation bound; the P scenes have about five per Gaussian.)"""
    means = rng.uniform(-1, 1, (N, 2))
    sig = sigma * np.exp(rng.normal(0, 0.1, (N, 2)))
    rho = rng.uniform(-0.9, 0.9, N)
    s0, s1 = sig[:, 0], sig[:, 1]
    det = (s0 * s1) ** 2 * (1 - rho ** 2)
    return means, np.stack((s1 ** 2 / det, -rho * s0 * s1 / det, s0 ** 2 / det), -1)


def geometry(name):
    """means [N, 2], flat conics [N, 3], points [M, 2] in float64 (not yet rounded): the same for c = 1 and c = 2."""
    from pigs_amd import synthetic
    from test_binned_gpu import random_gaussians
    _, _, N, M, _, _ = SCENES[name]
    rng = np.random.default_rng(seed_of("geometry", name))
    if name == "L-lattice":
        gs = synthetic.lattice_gaussians(24, 24, 0.8, seed=3)
        means, con, pts = gs["means"].numpy(), gs["conics"].numpy(), synthetic.grid_samples(64).numpy()
    elif name == "L-sorted":          # (random draws: neither the points nor the Gaussians arrive in any order)
        means, con, _ = random_gaussians(rng, N, 1, log_sigma_mean=-2.8, log_sigma_std=0.3)
        pts = rng.uniform(-1, 1, (M, 2))
    elif name == "R":
        means, con, _ = random_gaussians(rng, N, 1, log_sigma_mean=-1.6, log_sigma_std=0.8, lo=-0.5, hi=0.5)
        pts = rng.uniform(-0.5, 0.5, (M, 2))
    elif name == "G":
        wide = random_gaussians(rng, 300, 1, log_sigma_mean=-0.5, log_sigma_std=0.1)
        narrow = random_gaussians(rng, N - 300, 1, log_sigma_mean=-4.8, log_sigma_std=0.1)
        order = rng.permutation(N)
        means, con = np.concatenate((wide[0], narrow[0]))[order], np.concatenate((wide[1], narrow[1]))[order]
        pts = rng.uniform(-1, 1, (M, 2))
    else:
        means, con = narrow_gaussians(rng, N, np.exp(-4.0 if name == "P" else -3.6))
        pts = rng.uniform(-1, 1, (M, 2))
    assert means.shape == (N, 2) and con.shape == (N, 3) and pts.shape == (M, 2)
    return means, con, pts


class Scene(Case):
    """One scene with c channels: the inputs as the kernel sees them (float32-rounded) in float64, the oracle's outputs
    of orders 0..3 (computed once); the device tensors are made per test (``on_device``)."""

    def __init__(self, name, c):
        from oracle import c_oracle
        self.name, self.mode, self.order, self.N, self.M, self.claims, self.q_max = (name,) + SCENES[name]
        self.dtype, self.tdt, self.d, self.c, self.f32 = "float32", torch.float32, 2, c, True
        self.oracle = c_oracle
        means, con, pts = geometry(name)
        values = np.random.default_rng(seed_of("values", name, c)).uniform(-1, 1, (self.N, c))
        self.args = [round32(a) for a in (means, con, values, pts)]               # the oracle's order
        self.exp = c_oracle.forward(*self.args, orders=(0, 1, 2, 3))
        self.exp["lap"] = self.exp[2][:, 0, 0] + self.exp[2][:, 1, 1]

    def on_device(self, key):
        """A copy for one test: fresh leaves, a generator and an error table of its own."""
        import copy
        cs = copy.copy(self)
        cs.rng = np.random.default_rng(seed_of(key))
        cs.w = Worst("float32")
        means, con, values, pts = (cs.dev(a) for a in cs.args)
        cs.t = [means, values, con, pts]
        for x in cs.t[:3]:
            x.requires_grad_(True)
        cs.leaves = (means, con, values)
        return cs

    def sampler(self, **kw):
        from diff_gaussian_sampling import GaussianSampler
        s = GaussianSampler(True, backend="binned", fuse="none", q_max=self.q_max, **kw)
        self.bind(s)
        return s

    def bind(self, s):
        s.preprocess(self.t[0], self.t[1], None, self.t[2], self.t[3])
        assert s._plan is not None, "not the binned path"


@functools.lru_cache(maxsize=None)
def scene(name, c):
    return Scene(name, c)


# ---- what a plan's tile headers say (tools/prof_step.py list_stats reads the same words)
def headers(plan, hip_lib):
    """mode [tiles], count [tiles], group list lengths [tiles, 4], and the tile-list slabs [tiles, list_cap]"""
    import ctypes
    info = (ctypes.c_int64 * 6)()
    assert hip_lib.pigs_plan_layout_info(plan.N, plan.M, plan.c, info) == 0
    ntiles, cap, off_hdr, off_tlist = info[0], info[1], info[2], info[3]
    ws = plan.workspace
    hdr = ws[off_hdr:off_hdr + 32 * ntiles].view(torch.int32).cpu().numpy().astype(np.uint32).reshape(ntiles, 8)
    slabs = ws[off_tlist:off_tlist + 4 * ntiles * cap].view(torch.int32).cpu().numpy().astype(np.uint32).reshape(ntiles, cap)
    return hdr[:, 0] >> 30, hdr[:, 0] & ((1 << 30) - 1), hdr[:, 1:5].astype(np.int64), slabs


def assert_mode(cs, plan, hip_lib, s):
    """The plan that launched holds the scene's mode, with the properties the scene states."""
    from test_lattice_gpu import lattice_of
    mode, count, ng, slabs = headers(plan, hip_lib)
    tiles = -(-cs.M // 64)
    counts = [int((mode == k).sum()) for k in range(4)]
    what = (cs.name, "q_max", plan.q_max, "tiles in LIST / RANGES / GROUPS / POINTS", counts)
    assert len(mode) == tiles, what
    assert lattice_of(s, hip_lib) == ((64, 64) if cs.order == "lattice" else (0, 0)), what
    if cs.name == "L-lattice":
        assert counts[0] == tiles, what
    elif cs.name == "L-sorted":
        assert counts[0] == tiles, what
        assert ng.max() > 64 and count.max() > 128, (what, int(ng.max()), int(count.max()))
        assert ng.max() <= hp.plan_sizes(cs.N)[0] and count.max() <= hp.plan_sizes(cs.N)[0]
        assert 1 <= cs.M % 64 <= 15 and ng[-1, 0] > 0 and not ng[-1, 1:].any(), (what, ng[-1].tolist())
    elif cs.name == "R":
        r = mode == 1
        assert r.any(), what
        lengths = np.concatenate([slabs[t, 1:2 * count[t]:2] for t in np.flatnonzero(r)])
        assert count[r].max() >= 2 and (lengths % 16 != 0).any(), (what, count[r].tolist())
        assert not ((count[r] == 1) & (slabs[r, 1] == cs.N)).any(), "a tile fell back to the single range {0, N}"
    elif cs.name == "G":
        assert counts[2] > 0, what
        assert ng[mode == 2].max() <= hp.plan_sizes(cs.N)[0]
    elif cs.name == "P":
        assert counts[3] == tiles and cs.M % 4 != 0, what
    else:
        assert counts[3] > 64 and cs.M % 4 != 0, what
    return counts


def check_columns(cs, variant, what, got, want, scales):
    """A [M, k] output whose columns have scales of their own (the vorticity outputs)."""
    got = np64(got)
    cs.w.require(np.isfinite(got).all(), (what, "not finite"))
    for k, e in enumerate(np.abs(got - want).max(0) / scales):
        cs.w.note(variant, (what, "column", k), e / TOL)


def oracle_grads(cs, grads):
    return cs.oracle.backward(*cs.args, grads), cs.oracle.backward(*cs.args, grads, absolute=True)


def run_scene(hip_lib, name, c):
    import test_residual_coupled_gpu as RC
    import test_residual_terms_gpu as R
    import test_vorticity_gpu as V
    import test_vorticity_residual_gpu as VR
    from test_vorticity import column_scales, combine, expand
    from test_vorticity_residual import adjoint, compose
    order_sets, kinds = next((o, k) for n, cc, o, k in RUNS if (n, cc) == (name, c))
    cs = scene(name, c).on_device((name, c))
    exp, rng, args, M, d = cs.exp, cs.rng, cs.args, cs.M, 2
    fvar, bvar = cs.mode + " forward", cs.mode + " backward"
    s = cs.sampler()
    seen = {}

    def launched_on(plan):
        assert plan is not None
        seen[plan.q_max] = assert_mode(cs, plan, hip_lib, s)

    # ---- sample(): every covering mask alone, requests with holes, a backward with holes the forward did not have
    r = {o: cs.draw(out_shape(o, M, d, c)) for o in sorted({o for os_, _ in order_sets for o in os_}, key=str)}
    pieces = {o: cs.piece(o, r[o][1]) for o in r}
    for orders, reads in order_sets:
        reads = orders if reads is None else reads
        cs.bind(s)                                                       # forget the outputs of the previous set
        outs = s.sample(orders)
        launched_on(s._plan3 if 3 in orders else s._plan)
        for o, out in zip(orders, outs):
            assert tuple(out.shape) == out_shape(o, M, d, c) and out.dtype == torch.float32
            cs.check_output(fvar, (orders, "output", o), out, exp[o])
        loss = sum((out * r[o][0]).sum() for o, out in zip(orders, outs) if o in reads)
        got = torch.autograd.grad(loss, cs.leaves)
        want = [sum(pieces[o][0][k] for o in reads) for k in range(3)]
        mags = [sum(pieces[o][1][k] for o in reads) for k in range(3)]
        cs.check_grads(bvar, (orders, reads, "gradient"), got, want, mags)

    # ---- residual(): float coefficients (32), per-point fields without and with advection (64)
    if kinds:
        tgt, tgt64 = cs.draw((M, c))
        w, w64 = cs.draw((M, c))
    if "fields" in kinds:
        B64 = np64(cs.dev(rng.uniform(-1, 1, (d, c))))                  # a non-identity advect_by, as the kernel sees it
        B = tuple(tuple(float(x) for x in row) for row in B64)
        consts = (np.full(M, A0), np.tile(np.asarray(A1), (M, 1)), np.full(M, AL), None)
        Fn = tuple(cs.dev(a) for a in R.fields(rng, M, d, advect=False)[:3]) + (None,)
        Fa = tuple(cs.dev(a) for a in R.fields(rng, M, d))
        for what, F, call in (("linear residual", consts, lambda t_: s.residual(a0=A0, a1=A1, lap=AL, target=t_)),
                              ("fields", Fn, lambda t_: R.call(s, Fn, B, t_)),
                              ("fields + advection", Fa, lambda t_: R.call(s, Fa, B, t_))):
            assert what in kinds
            F64 = tuple(None if a is None else np64(a) for a in F)
            cs.bind(s)
            t_ = tgt.clone().requires_grad_(True)
            res = call(t_)
            launched_on(s._plan)
            assert tuple(res.shape) == (M, c) and res.dtype == torch.float32
            cs.check_output(fvar, (what, "output"), res, R.compose(exp, F64, B64, tgt64, d))
            got = torch.autograd.grad((res * w).sum(), cs.leaves + (t_,))
            cs.w.require(torch.equal(got[3], -w), (what, "the target's gradient is not -w"))
            if F[3] is not None:
                # the kernel forms the incoming gradients from its own float32 u and grad u: against torch.autograd
                # through the same expression on the sampler's own outputs
                R.check_against_own_composition(s, (cs.t[0], cs.t[1], cs.t[2]), F, B, tgt, d, w)
                for g in got[:3]:
                    cs.w.require(bool(torch.isfinite(g).all()), (what, "not finite"))
                continue
            want, mags = oracle_grads(cs, R.incoming(w64, exp, F64, B64, d, c))
            cs.check_grads(bvar, (what, "gradient"), got[:3], want, mags)

    # ---- two channels: the coupled residual (256), vorticity_terms() (128), vorticity_residual() (512)
    if "coupled residual" in kinds:
        K = RC.coefficients(rng, M, c)
        Kd = RC.on_device(K)
        K = RC.as_seen(Kd, K)
        cs.bind(s)
        res = RC.call(s, Kd, tgt)
        launched_on(s._plan)
        want_r, scale = RC.expectation(exp, K, tgt64, d, each=False)
        cs.check_output(fvar, ("coupled residual", "output"), res, want_r, scale=scale)
        got = torch.autograd.grad((res * w).sum(), cs.leaves)
        want, mags = oracle_grads(cs, RC.incoming(w64, K, d, c))
        cs.check_grads(bvar, ("coupled residual", "gradient"), got, want, mags)
    if "vorticity_terms" in kinds:
        g7, g7_64 = cs.draw((M, 7))
        cs.bind(s)
        out = s.vorticity_terms()
        launched_on(s._plan3)
        assert tuple(out.shape) == (M, 7)
        check_columns(cs, fvar, "vorticity_terms", out, combine(exp), column_scales(exp))
        got = torch.autograd.grad((out * g7).sum(), cs.leaves)
        want, mags = oracle_grads(cs, expand(g7_64))
        cs.check_grads(bvar, ("vorticity_terms", "gradient"), got, want, mags)
    if "vorticity_residual" in kinds:
        args_prev = [args[0], args[1], round32(VR.other_values(args[2], 5)), args[3]]
        exp_prev = cs.oracle.forward(*args_prev, orders=V.ORDERS)
        tau, tau64 = cs.draw((M,))
        tau, tau64 = (tau + 1) / 2, np64((tau + 1) / 2)                  # in [0, 1], as the kernel sees it
        g2, g2_64 = cs.draw((M, 2))
        now7, prev7 = combine(exp), round32(combine(exp_prev))
        cs.bind(s)
        out = VR.residual_of(s, cs.dev(prev7), tau)
        launched_on(s._plan3)
        assert tuple(out.shape) == (M, 2)
        check_columns(cs, fvar, "vorticity_residual", out, compose(now7, prev7, tau64, VR.NU, VR.DT, VR.TT),
                      VR.bars((exp, exp_prev)))
        got = torch.autograd.grad((out * g2).sum(), cs.leaves)
        want, mags = oracle_grads(cs, expand(adjoint(g2_64, now7, prev7, tau64, VR.NU, VR.DT, VR.TT)))
        cs.check_grads(bvar, ("vorticity_residual", "gradient"), got, want, mags)
    for q, counts in sorted(seen.items()):
        print(f"{name} c={c}: plan with q_max {q:g}: tiles in LIST / RANGES / GROUPS / POINTS {counts}")
    cs.w.report()


@pytest.mark.parametrize("name,c", [(n, c) for n, c, _, _ in RUNS], ids=[f"{n}-c{c}" for n, c, _, _ in RUNS])
def test_matrix(hip_lib, name, c):
    run_scene(hip_lib, name, c)


# ------------------------------------------------------------------------------------------
# the fused first launch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FUSED_FIRST_SCENES)
def test_fused_first(hip_lib, name, monkeypatch):
    """defer_lists=True: each of the five compiled plan_lists_forward_kernel instantiations as the first call on a fresh
    sampler builds the scene's lists and samples through them itself; a later sample((0, 1, 2)) and its backward read the
    lists that launch wrote.  The library takes the fused launch unless an earlier plan of the same (N, M) was seen to
    hold POINTS tiles (plan_expects_points): in scene P call k therefore drops the last k + 1 Gaussians -- sizes no
    plan of this process has had."""
    monkeypatch.delenv("PIGS_NO_FUSED_FIRST", raising=False)
    w = Worst("float32")
    for k, (c, first) in enumerate(FUSED_FIRST_CALLS):
        cs = scene(name, c).on_device((name, c, "fused first", k))
        cs.w = w
        fvar, bvar = cs.mode + " fused first", cs.mode + " backward after fused first"
        if name == "P":
            n = cs.N - 1 - k
            cs.N, cs.args = n, [a[:n] for a in cs.args[:3]] + [cs.args[3]]
            cs.t = [x.detach()[:n].clone().requires_grad_(True) for x in cs.t[:3]] + [cs.t[3]]
            cs.leaves = (cs.t[0], cs.t[2], cs.t[1])
            exp = cs.oracle.forward(*cs.args, orders=(0, 1, 2))
            exp["lap"] = exp[2][:, 0, 0] + exp[2][:, 1, 1]
        else:
            exp = cs.exp
        s = cs.sampler(defer_lists=True)
        if first == "linear residual":
            res = s.residual(a0=A0, a1=A1, lap=AL)
            consts = (np.full(cs.M, A0), np.tile(np.asarray(A1), (cs.M, 1)), np.full(cs.M, AL), None)
            import test_residual_terms_gpu as R
            cs.check_output(fvar, (c, first), res, R.compose(exp, consts, None, None, 2))
        else:
            for o, out in zip(first, s.sample(first)):
                cs.check_output(fvar, (c, first, "output", o), out, exp[o])
        assert_mode(cs, s._plan, hip_lib, s)
        later = s.sample((0, 1, 2))
        r = [cs.draw(out_shape(o, cs.M, 2, c)) for o in range(3)]
        for o, out in enumerate(later):
            cs.check_output(fvar, (c, first, "later output", o), out, exp[o])
        got = torch.autograd.grad(sum((out * r[o][0]).sum() for o, out in enumerate(later)), cs.leaves)
        want, mags = oracle_grads(cs, {o: r[o][1] for o in range(3)})
        cs.check_grads(bvar, (c, first, "later gradient"), got, want, mags)
    w.report()
