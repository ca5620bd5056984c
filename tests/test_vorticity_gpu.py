"""GPU: GaussianSampler.vorticity_terms() -- (u_x, u_y, div, w, w_x, w_y, lap_w) of a two-channel field in one launch
(pair_math.h ORDV, pigs_vorticity_*; the reference's Navier-Stokes outputs, model_pn.py:650-659, 770-781, 848).

Expected values: the float64 oracle's orders 0..3 combined with the reference's own index expressions
(tests/test_vorticity.py combine); expected gradients: the oracle's backward fed with the four full-layout gradient
arrays that a random gout [M, 7] induces (expand, pinned as combine's adjoint on the CPU).

Bars, all taken from the project:
  float32 forward     1e-5 of the column's scale: the largest magnitude among the oracle entries that enter the column
                      (tests/test_residual_terms_gpu.py term_scale; the columns are differences)
  float64             1e-11
  gradients           1e-5 of the tensor's largest entry + conftest.grads_within_accumulation_bound with its defaults
  binned              TOL of tests/test_binned_gpu.py
  own composition     2e-6 / 1e-5 (the residual tests)

Measured on an MI355X, the worst over the cases of this file: dense float32 forward 1.6e-6 of the column scale (rows,
lap_w) and gradients 8.7e-7; float64 4.8e-16 and 2.3e-15; binned forward 7.4e-7; periodic 1.3e-6; own composition 8.5e-7
forward, 2.9e-7 gradients.  No case needed another bar."""
import functools

import numpy as np
import pytest
import torch

from conftest import grads_within_accumulation_bound
from oracle import c_oracle
from pigs_amd import synthetic
from test_binned_gpu import TOL, dev32
from test_periodic_gpu import check_grads as check_periodic_grads
from test_periodic_gpu import periodic_forward
from test_vorticity import column_scales, combine, expand

pytestmark = pytest.mark.gpu
HOSTS = ["native", "ctypes"]
ORDERS = (0, 1, 2, 3)


def np64(x):
    return x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def rel(a, b):
    a, b = np64(a), np64(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def column_errors(got, exp):
    """Per column: the largest error as a fraction of the column's scale."""
    return np.abs(np64(got) - combine(exp)).max(0) / column_scales(exp)


def leaves_of(means, values, con, dtype=torch.float32):
    t = [dev(a, dtype) for a in (means, values, con)]
    for x in t:
        x.requires_grad_(True)
    return t


def oracle_args(t, pts):
    """(means, conics, values, samples) in float64 as the kernels saw them (float32 rounding included)"""
    return [np64(t[0]), np64(t[2]), np64(t[1]), np64(pts)]


def composed_by_torch(s):
    """The seven columns from the sampler's OWN sample((0, 1, 2, 3)): the reference's lines in torch."""
    u, ux, uxx, uxxx = s.sample(ORDERS)
    div = ux[:, 0, 0] + ux[:, 1, 1]
    w = ux[:, 0, 1] - ux[:, 1, 0]
    wx = uxx[..., 0, 1] - uxx[..., 1, 0]
    wxx = uxxx[..., 0, 1] - uxxx[..., 1, 0]
    lap_w = wxx[:, 0, 0] + wxx[:, 1, 1]
    return torch.stack((u[:, 0], u[:, 1], div, w, wx[:, 0], wx[:, 1], lap_w), -1), (u, ux, uxx, uxxx)


def check_f32_grads(got, args, gout64):
    """got = (g_means, g_conics, g_values) against the oracle's backward of expand(gout)."""
    grads = expand(gout64)
    want = c_oracle.backward(*args, grads)
    for name, g, w in zip(("means", "conics", "values"), got, want):
        assert rel(g, w) < 1e-5, (name, rel(g, w))
    bad = grads_within_accumulation_bound(got, args, grads)
    assert not bad, bad


# ------------------------------------------------------------------------------------------
# 1. dense, every launch variant the mask can take
# ------------------------------------------------------------------------------------------
NACC = 7
# the launchers' selection goes by accumulator count: d = 2, c = 7, mask 1 is the instantiation that
# tests/host_program.py can ask about with FwdLayout::N == 7
DENSE_SHAPES = [(33, 81), (161, 81), (100, 19201), (1300, 16400), (1300, 5501)]
DENSE_CASES = [(torch.float32, N, M) for N, M in DENSE_SHAPES] + [(torch.float64, N, M) for N, M in DENSE_SHAPES[:3]]


def variants_of(dtype, N, M):
    import host_program as hp
    ch = hp.dense("float32" if dtype == torch.float32 else "float64", 2, NACC, 1, N, M)
    return ch.forward, ch.backward


def test_the_dense_cases_reach_every_variant():
    """A changed threshold in dense_choice.h shows up here, not as a silent hole."""
    import host_program as hp
    assert hp.dense("float32", 2, NACC, 1, 1, 1).accumulators == NACC
    assert all(N % 64 and M % 64 for N, M in DENSE_SHAPES)
    f32 = [variants_of(torch.float32, N, M) for t, N, M in DENSE_CASES if t == torch.float32]
    f64 = [variants_of(torch.float64, N, M) for t, N, M in DENSE_CASES if t == torch.float64]
    assert {f for f, _ in f32} == {"rows", "w16", "w4"}
    assert {f for f, _ in f64} == {"rows", "w4"}
    assert {b for _, b in f32} == {"staged32", "staged64", "split_atomic"}
    assert [variants_of(t, N, M) for t, N, M in DENSE_CASES] == [
        ("w4", "staged32"), ("rows", "staged32"), ("w16", "split_atomic"), ("w16", "split_atomic"), ("rows", "staged64"),
        ("w4", "staged32"), ("rows", "staged32"), ("w4", "split_atomic")]


def dense_inputs(N, M, seed):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1, 1, (N, 2))
    s0 = np.exp(2 * rng.normal(-3.0, 0.4, (N, 2)))
    tau = np.tanh(rng.normal(0, 0.6, N)) * np.sqrt(s0[:, 0] * s0[:, 1])
    det = s0[:, 0] * s0[:, 1] - tau ** 2
    con = np.stack((s0[:, 1] / det, -tau / det, s0[:, 0] / det), -1)
    return means, rng.uniform(-1, 1, (N, 2)), con, rng.uniform(-1, 1, (M, 2)), rng.uniform(-1, 1, (M, 7))


@functools.lru_cache(maxsize=None)
def dense_expectation(dtype, N, M):
    """The problem in the kernels' dtype, the oracle's outputs and gradients: computed once, shared by both hosts."""
    means, values, con, pts, gout = dense_inputs(N, M, N + M)
    rnd = (lambda a: np64(dev(a, dtype)))
    args = [rnd(means), rnd(con), rnd(values), rnd(pts)]
    gout = rnd(gout)
    exp = c_oracle.forward(*args, orders=ORDERS)
    return args, gout, exp, c_oracle.backward(*args, expand(gout))


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,N,M", DENSE_CASES)
def test_dense_matches_the_oracle(hip_lib, host, dtype, N, M):
    from diff_gaussian_sampling import GaussianSampler
    args, gout, exp, want_g = dense_expectation(dtype, N, M)
    t = leaves_of(args[0], args[2], args[1], dtype)
    pts = dev(args[3], dtype)
    s = GaussianSampler(True, backend="dense", host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    assert s._plan is None
    out = s.vorticity_terms()
    assert tuple(out.shape) == (M, 7) and out.dtype == dtype and out.is_contiguous()
    errs = column_errors(out, exp)
    print(f"{variants_of(dtype, N, M)} forward, per column of its scale: {np.array2string(errs, precision=2)}")
    assert errs.max() < (1e-5 if dtype == torch.float32 else 1e-11), errs
    (out * dev(gout, dtype)).sum().backward()
    got = (t[0].grad, t[2].grad, t[1].grad)
    errs_g = [rel(g, w) for g, w in zip(got, want_g)]
    print("gradients (means, conics, values):", errs_g)
    if dtype == torch.float64:
        assert max(errs_g) < 1e-11, errs_g
    else:
        assert max(errs_g) < 1e-5, errs_g
        bad = grads_within_accumulation_bound(got, args, expand(gout))
        assert not bad, bad


# ------------------------------------------------------------------------------------------
# 2. binned
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def binned_problem(points):
    gs = synthetic.lattice_gaussians(32, 32, 0.8, seed=3, c=2)
    rng = np.random.default_rng(14)
    pts = {"lattice": lambda: synthetic.grid_samples(64).numpy(),            # index-tiled order
           "random": lambda: rng.uniform(-1, 1, (4099, 2)),                   # the sorted path
           "small": lambda: rng.uniform(-1, 1, (300, 2))}[points]()           # the small path
    args = [np64(dev32(a)) for a in (gs["means"].numpy(), gs["conics"].numpy(), gs["values"].numpy(), pts)]
    M = len(pts)
    gout = np.zeros((M, 7))
    gout[::7] = rng.uniform(-1, 1, (len(range(0, M, 7)), 7))                  # a loss supported on every 7th point
    gout = np64(dev32(gout))
    return args, gout, c_oracle.forward(*args, orders=ORDERS)


@pytest.mark.parametrize("points", ["lattice", "random", "small"])
def test_binned_matches_the_oracle(hip_lib, points):
    from diff_gaussian_sampling import GaussianSampler
    args, gout, exp = binned_problem(points)
    assert args[0].shape[0] == 1024
    t = leaves_of(args[0], args[2], args[1])
    s = GaussianSampler(True, backend="binned")
    s.preprocess(t[0], t[1], None, t[2], dev32(args[3]))
    assert s._plan is not None
    out = s.vorticity_terms()
    assert s._plan3 is not None and s._plan3.q_max == pytest.approx(s.q_max_order3)
    errs = column_errors(out, exp)
    print(f"binned {points}: forward, per column of its scale: {np.array2string(errs, precision=2)}")
    assert errs.max() < TOL, errs
    g = torch.autograd.grad((out * dev32(gout)).sum(), t)
    check_f32_grads((g[0], g[2], g[1]), args, gout)


# ------------------------------------------------------------------------------------------
# 3. periodic (-1, 1)
# ------------------------------------------------------------------------------------------
def periodic_problem(box=None):
    """N = 64: 8 means within one sigma of the x seam, 8 of the y seam, 4 at the corners, the rest anywhere in the box;
    sigma = e^-2 .. e^-1.6 (extent at q_cut = 44 below 1.35 < L = 2).  ``box`` = (lo, hi): the same problem moved by
    x -> lo + (x + 1) a, a = (hi - lo) / 2 (means and points mapped, conics / a^2)."""
    rng = np.random.default_rng(7)
    N = 64
    s = np.exp(rng.uniform(-4.0, -3.2, (N, 2)))
    means = rng.uniform(-1, 1, (N, 2))
    means[:8, 0] = rng.choice([-1.0, 1.0], 8) * (1 - rng.uniform(0, 1, 8) * np.sqrt(s[:8, 0]))
    means[8:16, 1] = rng.choice([-1.0, 1.0], 8) * (1 - rng.uniform(0, 1, 8) * np.sqrt(s[8:16, 1]))
    means[16:20] = np.array([[1, 1], [-1, 1], [1, -1], [-1, -1]]) * (1 - 0.5 * np.sqrt(s[16:20]))
    tau = np.tanh(rng.normal(0, 0.5, N)) * np.sqrt(s[:, 0] * s[:, 1])
    det = s[:, 0] * s[:, 1] - tau ** 2
    con = np.stack((s[:, 1] / det, -tau / det, s[:, 0] / det), -1)
    pts = np.concatenate((synthetic.grid_samples(24).numpy(), rng.uniform(-1, 1, (423, 2))))
    values, gout = rng.uniform(-1, 1, (N, 2)), rng.uniform(-1, 1, (len(pts), 7))
    if box is not None:
        from test_aggregate_matrix_gpu import to_box
        means, con = to_box(means, con, box)
        pts = to_box(pts.astype(np.float64), None, box)[0]
    return means, values, con, pts, gout


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_periodic_matches_the_oracle_on_the_images(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    means, values, con, pts, gout = periodic_problem()
    t = leaves_of(means, values, con)
    pts_t, gout_t = dev32(pts), dev32(gout)
    s = GaussianSampler(True, backend=backend, host=host, periodic=(-1.0, 1.0))       # debug mode: runs clean
    s.preprocess(t[0], t[1], None, t[2], pts_t)
    assert (s._plan is not None) == (backend == "binned")
    assert s._inputs[0].shape == (9 * 64, 2)
    out = s.vorticity_terms()
    args = oracle_args(t, pts_t)
    exp = periodic_forward(*args)
    errs = column_errors(out, exp)
    print(f"periodic {backend}: forward, per column of its scale: {np.array2string(errs, precision=2)}")
    assert errs.max() < 1e-5, errs
    g = torch.autograd.grad((out * gout_t).sum(), t)
    assert g[0].shape == (64, 2) and g[1].shape == (64, 2) and g[2].shape == (64, 3)
    check_periodic_grads((g[0], g[2], g[1]), *args, expand(np64(gout_t)), torch.float32)


# ------------------------------------------------------------------------------------------
# 4. against the sampler's own sample((0, 1, 2, 3)) composed in torch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_equals_the_composition_of_the_samplers_own_outputs(hip_lib, host, backend):
    """A sign or a component that the oracle helper might share with the kernel cannot hide here: the composition is
    the reference's lines on the outputs of the existing order 0..3 kernels, the gradients torch.autograd's."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(20, 20, 1.1, seed=5, c=2)
    t = leaves_of(gs["means"].numpy(), gs["values"].numpy(), gs["conics"].numpy())
    rng = np.random.default_rng(2)
    M = 1531
    pts, w = dev32(rng.uniform(-1, 1, (M, 2))), dev32(rng.uniform(-1, 1, (M, 7)))
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    out = s.vorticity_terms()
    g_out = torch.autograd.grad((out * w).sum(), t)
    comp, orders = composed_by_torch(s)
    g_comp = torch.autograd.grad((comp * w).sum(), t)
    sc = [float(o.detach().abs().max()) for o in orders]
    scales = torch.tensor([sc[0], sc[0], sc[1], sc[1], sc[2], sc[2], sc[3]], device="cuda")
    fwd = float(((out - comp).detach().abs().max(0).values / scales).max())
    grads = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_out, g_comp)]
    print(f"own composition ({backend}): forward {fwd:.3g} of the column scale, gradients {grads}")
    assert fwd < 2e-6, fwd
    assert max(grads) < 1e-5, grads


# ------------------------------------------------------------------------------------------
# 5. host parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hosts_agree_bitwise(hip_lib, dtype):
    """Same C ABI, same launches: bit-identical outputs and gradients.  (N = 200, M = 32: the staged backward covers
    the points with ONE slice, so every gradient entry is a single atomic add to zero and has no order to depend on.)"""
    from diff_gaussian_sampling import GaussianSampler
    means, values, con, pts, gout = dense_inputs(200, 32, 5)
    assert variants_of(dtype, 200, 32)[1] == "staged32"
    res = {}
    for host in HOSTS:
        t = leaves_of(means, values, con, dtype)
        s = GaussianSampler(False, backend="dense", host=host)
        s.preprocess(t[0], t[1], None, t[2], dev(pts, dtype))
        out = s.vorticity_terms()
        res[host] = (out.detach(),) + torch.autograd.grad((out * dev(gout, dtype)).sum(), t)
    for a, b in zip(res["native"], res["ctypes"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------
# 6. autograd behaviour
# ------------------------------------------------------------------------------------------
def small_problem(M=700, seed=4, grad=True, n=12):
    gs = synthetic.lattice_gaussians(n, n, 1.0, seed=seed, c=2)
    t = [gs[k].float().cuda() for k in ("means", "values", "conics")]
    if grad:
        for x in t:
            x.requires_grad_(True)
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand((M, 2), generator=gen) * 2 - 1).cuda()
    return t, pts, (torch.rand((M, 7), generator=gen) * 2 - 1).cuda()


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_node_owns_its_inputs_and_plan(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w = small_problem()
    s = GaussianSampler(True, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    out = s.vorticity_terms()
    assert s.vorticity_terms() is out                                  # cached until the next preprocess
    loss = (out * w).sum()
    g1 = torch.autograd.grad(loss, t, retain_graph=True)
    # a later preprocess (other Gaussians, other points) before the second backward of the same graph
    t2, pts2, _ = small_problem(M=333, seed=9)
    s.preprocess(t2[0], t2[1], None, t2[2], pts2)
    out2 = s.vorticity_terms()
    assert out2 is not out and tuple(out2.shape) == (333, 7)
    g2 = torch.autograd.grad(loss, t, retain_graph=True)
    for a, b in zip(g1, g2):
        assert rel(a, b) < 2e-6                                        # the backward's atomics, as between any two runs
    with torch.no_grad():
        t[0].add_(0.0)                                                 # an in-place write, whatever it writes
    with pytest.raises(RuntimeError, match="modified in place"):
        torch.autograd.grad(loss, t)


@pytest.mark.parametrize("host", HOSTS)
def test_differentiable_call_rebuilds_a_forward_only_plan(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w = small_problem(M=3000)
    full = GaussianSampler(True, backend="binned", host=host)
    full.preprocess(t[0], t[1], None, t[2], pts)
    g_full = torch.autograd.grad((full.vorticity_terms() * w).sum(), t)
    assert not full._plan3.forward_only
    lazy = GaussianSampler(True, backend="binned", host=host)
    with torch.no_grad():
        lazy.preprocess(t[0], t[1], None, t[2], pts)
        r0 = lazy.vorticity_terms()                                    # served by forward-only plans
        before, before3 = lazy._plan, lazy._plan3
        assert before.forward_only and before3.forward_only and r0.grad_fn is None
        assert lazy.vorticity_terms() is r0
    r = lazy.vorticity_terms()                                         # differentiable: launched again, both plans rebuilt in full
    assert r is not r0 and r.grad_fn is not None
    assert lazy._plan is not before and lazy._plan3 is not before3
    assert not lazy._plan.forward_only and not lazy._plan3.forward_only
    assert float((r.detach() - r0).abs().max()) <= 1e-6 * float(r0.abs().max())
    # (a preprocess under no_grad binds views of values and conics that do not lead back to the caller's leaves, as for
    # every sample_*() output: the means do)
    g_lazy = torch.autograd.grad((r * w).sum(), t[0])
    assert torch.isfinite(g_lazy[0]).all() and rel(g_lazy[0], g_full[0]) < 1e-5


def test_backward_on_forward_only_workspace_writes_nan(hip_lib):
    """The C ABI: pigs_vorticity_backward on a workspace built with PIGS_BUILD_FORWARD_ONLY writes NaN gradients, as
    pigs_residual_backward does (tests/test_forward_only_gpu.py) -- never a gradient with terms missing; the forward on it
    serves.  The raw helper runs such a plan's backward on a full plan of the same inputs and agrees with one."""
    import ctypes
    from pigs_amd import host_ctypes as S
    t, pts, w = small_problem(M=3000, grad=False, n=32)
    m, v, c = (x.contiguous() for x in t)
    N, M = m.shape[0], pts.shape[0]
    plan = S.Plan(m, v, c, pts, 44.0, q_max_backward=44.0, forward_only=True)
    full = S.Plan(m, v, c, pts, 44.0, q_max_backward=44.0)
    assert plan.forward_only and not full.forward_only
    op = S._VorticityFunction.op
    out = S._fused_call(op, False, m, v, c, pts, None, plan)
    assert torch.isfinite(out).all() and rel(out, S._fused_call(op, False, m, v, c, pts, None, full)) < 1e-6
    gm, gv, gc = (torch.zeros_like(x) for x in (m, v, c))
    p, sws = ctypes.c_void_p, plan.samples.workspace
    rc = hip_lib.pigs_vorticity_backward(0, N, M, p(m.data_ptr()), p(c.data_ptr()), p(v.data_ptr()), p(pts.data_ptr()),
                                         p(w.data_ptr()), p(gm.data_ptr()), p(gc.data_ptr()), p(gv.data_ptr()),
                                         p(plan.workspace.data_ptr()), plan.workspace.numel(), p(sws.data_ptr()), sws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(gm.isnan().all()) and bool(gv.isnan().all()) and bool(gc.isnan().all())
    for x, y in zip(S._fused_call(op, True, m, v, c, pts, None, full, gout=w),
                    S._fused_call(op, True, m, v, c, pts, None, plan, gout=w)):
        assert torch.isfinite(x).all() and rel(y, x) < 1e-5


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_inputs(hip_lib, host, dtype):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, _ = small_problem(M=50)
    t = [x.detach().to(dtype).requires_grad_(True) for x in t]
    s = GaussianSampler(True, host=host)
    # M = 0
    s.preprocess(t[0], t[1], None, t[2], pts[:0].to(dtype))
    out = s.vorticity_terms()
    assert tuple(out.shape) == (0, 7) and out.dtype == dtype
    g = torch.autograd.grad(out.sum(), t)
    assert all(tuple(a.shape) == tuple(x.shape) and not a.any() for a, x in zip(g, t))
    # N = 0
    e = [x.detach()[:0].clone().requires_grad_(True) for x in t]
    s.preprocess(e[0], e[1], None, e[2], pts.to(dtype))
    out = s.vorticity_terms()
    assert tuple(out.shape) == (50, 7) and not out.any()
    g = torch.autograd.grad(out.sum(), e)
    assert [tuple(a.shape) for a in g] == [(0, 2), (0, 2), (0, 3)]


# ------------------------------------------------------------------------------------------
# 7. the overflow guard
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_far_points_of_a_nearly_singular_conic_stay_finite(hip_lib, backend):
    """Conics with |rho| -> 1 and entries of 1e12 and 4e12: at a point 2.5 away g is exactly 0 while |p| reaches 1e13 and
    the cubic factor of lap_w overflows float32 -- 0 * inf would poison the sum of every point.  Such a pair contributes
    exactly nothing: every column is finite and equals the oracle's."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(12, 12, 1.0, seed=4, c=2)
    means, values, con = (gs[k].numpy().copy() for k in ("means", "values", "conics"))
    means[:2] = [[-0.9, -0.9], [-0.8, -0.95]]
    con[0] = [1e12, 1e12 * (1 - 1e-6), 1e12]
    con[1] = [4e12, 4e12 * (1 - 1e-6), 4e12]
    rng = np.random.default_rng(3)
    pts = np.concatenate((rng.uniform(-1, 1, (500, 2)), [[0.9, 0.9], [0.7, 0.99], [0.95, 0.95]]))
    t = leaves_of(means, values, con)
    x = np64(dev32(pts))[-1] - np64(t[0])[1]
    c1 = np64(t[2])[1]
    p = np.array([c1[0] * x[0] + c1[1] * x[1], c1[1] * x[0] + c1[2] * x[1]])
    assert np.abs(p).max() ** 3 > 3.5e38               # past float32 for the second Gaussian, at its edge for the first
    s = GaussianSampler(True, backend=backend)
    s.preprocess(t[0], t[1], None, t[2], dev32(pts))
    out = s.vorticity_terms()
    assert torch.isfinite(out).all()
    exp = c_oracle.forward(*oracle_args(t, dev32(pts)), orders=ORDERS)
    assert np.isfinite(combine(exp)).all()
    assert column_errors(out, exp).max() < 1e-5
    g = torch.autograd.grad(out.sum(), t)
    assert all(torch.isfinite(a).all() for a in g)


# ------------------------------------------------------------------------------------------
# 8. error paths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
def test_unsupported_inputs_raise(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(False, host=host)
    with pytest.raises(RuntimeError, match="preprocess"):
        s.vorticity_terms()
    pts = torch.rand((40, 2)).cuda()
    for c in (1, 3):
        gs = synthetic.lattice_gaussians(6, 6, 1.0, seed=1, c=c)
        s.preprocess(gs["means"].float().cuda(), gs["values"].float().cuda(), None, gs["conics"].float().cuda(), pts)
        with pytest.raises(NotImplementedError, match="two-channel"):
            s.vorticity_terms()
    line = synthetic.line_gaussians_1d(16)
    s.preprocess(line["means"].float().cuda(), line["values"].float().cuda().expand(16, 2).contiguous(), None,
                 line["conics"].float().cuda(), torch.rand((40, 1)).cuda())
    with pytest.raises(NotImplementedError, match="two dimensions"):
        s.vorticity_terms()


# ------------------------------------------------------------------------------------------
# 9. graph capture
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_graphed_step_matches_eager(hip_lib, host, backend):
    """preprocess + vorticity_terms + loss + backward captured once and replayed after an in-place update of the
    values, against the same step issued eagerly."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    t, pts, w = small_problem(M=2000, grad=False)
    sampler = GaussianSampler(False, backend=backend, host=host)

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in t)

    def fn(means, values, conics):
        sampler.preprocess(means, values, None, conics, pts)
        u_x, u_y, div, vort, w_x, w_y, lap_w = sampler.vorticity_terms().unbind(1)
        r = u_x * w_x + u_y * w_y - 0.01 * lap_w
        loss = r.pow(2).mean() + div.pow(2).mean() + 1e-3 * vort.pow(2).mean()
        return (loss,) + torch.autograd.grad(loss, (means, values, conics))

    step = GraphedStep(fn, make_inputs)
    gen = torch.Generator().manual_seed(9)
    for trial in range(2):
        with torch.no_grad():
            step.inputs[1].copy_((torch.rand(t[1].shape, generator=gen) * 2 - 1).cuda())
        got = [x.clone() for x in step()]
        torch.cuda.synchronize()
        m, v, c = (x.detach().clone().requires_grad_(True) for x in step.inputs)
        eager = fn(m, v, c)
        for k, (a, b) in enumerate(zip(got, eager)):
            assert rel(a, b) < 2e-6, (trial, k, rel(a, b))
