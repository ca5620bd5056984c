"""GPU: GaussianSampler.vorticity_residual(data=...) -- (div_b, r, data_weight (w - data)) in one launch each way (pair_math.h
ORDF, pigs_vorticity_fit_*; the data term of main_pn.py:202-212 and the fit of test_initialize.py:131-136) -- and the
end-to-end initialisation fit with pigs_amd.grid_lookup and GaussianAdam.

Expected values: compose3() of the float64 oracle's orders 0..3 of two time levels (tests/test_vorticity_fit.py; the
problems are those of tests/test_vorticity_residual_gpu.py, plus a data array of the vorticity's scale); expected
gradients: the oracle's backward fed with expand(adjoint3(gout, ...)).

Bars, those of tests/test_vorticity_residual_gpu.py, none new.  With S_k = max |o_k| over both levels:
  div, r         as there
  fit            1e-5 |data_weight| S_1 (float32), 1e-11 |data_weight| S_1 (float64): like div, a combination of two
                 first derivatives (the data is exact)
  gradients      1e-5 of the tensor's largest entry + conftest.grads_within_accumulation_bound; float64 1e-11
  binned         TOL of tests/test_binned_gpu.py
  own composition: columns 0-1 against vorticity_residual() on the same plan, bit-equal (both calls take the same launch
                 variant: the table below); column 2 against data_weight * (vorticity_terms()[:, 3] - data) and
                 torch.autograd, 2e-6 / 1e-5

The launch variants of mask 4096 (tests/host_program.py asks dense_choice.h) are those of mask 512: the 16-wave forward
was not withheld -- <float, 2, 2, 4096, 16> compiles to 123 VGPRs without scratch:
  float32  (33, 81) w4 / staged32   (161, 81) rows / staged32   (100, 19 201) w16 / split_atomic
           (1 300, 16 400) w16 / split_atomic   (1 300, 5 501) rows / staged64
  float64  (33, 81) w4 / staged32   (161, 81) rows / staged32   (100, 19 201) w4 / split_atomic

Every case prints its figures before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import host_program as hp
import test_vorticity_residual_gpu as VR
from conftest import grads_within_accumulation_bound
from oracle import c_oracle
from test_binned_gpu import TOL, dev32
from test_periodic_gpu import check_grads as check_periodic_grads
from test_periodic_gpu import periodic_forward
from test_vorticity import combine, expand
from test_vorticity_fit import adjoint3, compose3
from test_vorticity_gpu import (DENSE_CASES, DENSE_SHAPES, HOSTS, ORDERS, binned_problem, dense_inputs, dev, leaves_of, np64,
                                oracle_args, periodic_problem, rel)
from test_vorticity_residual import compose

pytestmark = pytest.mark.gpu
NU, DT, TT = VR.NU, VR.DT, VR.TT
DW = float(np.sqrt(5.0))                  # main_pn.py:209
MASK = 4096


def bars3(exps, dw=DW, **k):
    """The scales of the three columns (module docstring) from the oracle outputs of both levels."""
    S1 = max(np.abs(e[1]).max() for e in exps)
    return np.concatenate((VR.bars(exps, **k), [abs(dw) * S1]))


def fit_of(s, prev, tau, data, dw=DW, nu=NU, dt=DT, tt=TT):
    return s.vorticity_residual(nu, dt, prev, tau, time_term=tt, data=data, data_weight=dw)


def data_like(rng, exps, M):
    """a data array of the vorticity's scale"""
    return rng.uniform(-1, 1, M) * max(np.abs(e[1]).max() for e in exps)


def variants_of(dtype, N, M, mask=MASK):
    ch = hp.dense("float32" if dtype == torch.float32 else "float64", 2, 2, mask, N, M)
    return ch.forward, ch.backward


# ------------------------------------------------------------------------------------------
# 1. dense, every launch variant
# ------------------------------------------------------------------------------------------
def test_the_dense_cases_reach_every_variant():
    """The variant table of the new mask, asked from the launch-choice program: equal to mask 512's (w16 was not withheld)."""
    assert hp.dense("float32", 2, 2, MASK, 1, 1).accumulators == 7
    assert hp.dense("float32", 2, 2, MASK, 1, 1).can_w16 == 1 and hp.dense("float64", 2, 2, MASK, 1, 1).can_w16 == 0
    table = [variants_of(t, N, M) for t, N, M in DENSE_CASES]
    assert table == [
        ("w4", "staged32"), ("rows", "staged32"), ("w16", "split_atomic"), ("w16", "split_atomic"), ("rows", "staged64"),
        ("w4", "staged32"), ("rows", "staged32"), ("w4", "split_atomic")]
    assert table == [variants_of(t, N, M, 512) for t, N, M in DENSE_CASES]
    assert DENSE_SHAPES == [(33, 81), (161, 81), (100, 19201), (1300, 16400), (1300, 5501)]
    assert hp.covering(MASK) == MASK


@functools.lru_cache(maxsize=None)
def dense_expectation(dtype, N, M):
    means, values, con, pts, _ = dense_inputs(N, M, N + M)
    rng = np.random.default_rng(N * 7 + M + 1)
    rnd = (lambda a: np64(dev(a, dtype)))
    args = [rnd(means), rnd(con), rnd(values), rnd(pts)]
    args_prev = [args[0], args[1], rnd(VR.other_values(values, N)), args[3]]
    tau, gout = rnd(rng.uniform(0, 1, M)), rnd(rng.uniform(-1, 1, (M, 3)))
    exp, exp_prev = c_oracle.forward(*args, orders=ORDERS), c_oracle.forward(*args_prev, orders=ORDERS)
    data = rnd(data_like(rng, (exp, exp_prev), M))
    now7, prev7 = combine(exp), rnd(combine(exp_prev))
    want = compose3(now7, prev7, tau, NU, DT, TT, data, DW)
    g7 = adjoint3(gout, now7, prev7, tau, NU, DT, TT, DW)
    return args, prev7, tau, data, gout, want, bars3((exp, exp_prev)), g7, c_oracle.backward(*args, expand(g7))


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,N,M", DENSE_CASES)
def test_dense_matches_the_oracle(hip_lib, host, dtype, N, M):
    from diff_gaussian_sampling import GaussianSampler
    args, prev7, tau, data, gout, want, scales, g7, want_g = dense_expectation(dtype, N, M)
    t = leaves_of(args[0], args[2], args[1], dtype)
    s = GaussianSampler(True, backend="dense", host=host)
    s.preprocess(t[0], t[1], None, t[2], dev(args[3], dtype))
    assert s._plan is None
    out = fit_of(s, dev(prev7, dtype), dev(tau, dtype), dev(data, dtype))
    assert tuple(out.shape) == (M, 3) and out.dtype == dtype and out.is_contiguous()
    errs = VR.column_errors(out, want, scales)
    print(f"{variants_of(dtype, N, M)} forward (div, r, fit) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < (1e-5 if dtype == torch.float32 else 1e-11), errs
    (out * dev(gout, dtype)).sum().backward()
    got = (t[0].grad, t[2].grad, t[1].grad)
    errs_g = [rel(g, w) for g, w in zip(got, want_g)]
    print("gradients (means, conics, values):", errs_g)
    if dtype == torch.float64:
        assert max(errs_g) < 1e-11, errs_g
    else:
        assert max(errs_g) < 1e-5, errs_g
        bad = grads_within_accumulation_bound(got, args, expand(g7))
        assert not bad, bad


# ------------------------------------------------------------------------------------------
# 2. binned: the order-3 plan
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def binned_expectation(points):
    args, _, exp = binned_problem(points)
    M = len(args[3])
    rng = np.random.default_rng(22)
    args_prev = [args[0], args[1], np64(dev32(VR.other_values(args[2], 5))), args[3]]
    exp_prev = c_oracle.forward(*args_prev, orders=ORDERS)
    tau = np64(dev32(rng.uniform(0, 1, M)))
    data = np64(dev32(data_like(rng, (exp, exp_prev), M)))
    gout = np.zeros((M, 3))
    gout[::7] = rng.uniform(-1, 1, (len(range(0, M, 7)), 3))                  # a loss supported on every 7th point
    gout = np64(dev32(gout))
    now7, prev7 = combine(exp), np64(dev32(combine(exp_prev)))
    return (args, prev7, tau, data, gout, compose3(now7, prev7, tau, NU, DT, TT, data, DW), bars3((exp, exp_prev)),
            adjoint3(gout, now7, prev7, tau, NU, DT, TT, DW))


@pytest.mark.parametrize("points", ["lattice", "random", "small"])
def test_binned_matches_the_oracle(hip_lib, points):
    from diff_gaussian_sampling import GaussianSampler
    args, prev7, tau, data, gout, want, scales, g7 = binned_expectation(points)
    assert args[0].shape[0] == 1024
    t = leaves_of(args[0], args[2], args[1])
    s = GaussianSampler(True, backend="binned")
    s.preprocess(t[0], t[1], None, t[2], dev32(args[3]))
    assert s._plan is not None
    out = fit_of(s, dev32(prev7), dev32(tau), dev32(data))
    assert s._plan3 is not None and s._plan3.q_max == pytest.approx(s.q_max_order3)
    errs = VR.column_errors(out, want, scales)
    print(f"binned {points}: forward (div, r, fit) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < TOL, errs
    g = torch.autograd.grad((out * dev32(gout)).sum(), t)
    VR.check_f32_grads((g[0], g[2], g[1]), args, g7)


@pytest.mark.parametrize("name", ["L-lattice", "L-sorted", "R", "G", "P"])
def test_binned_tile_modes(hip_lib, name):
    """tile_forward_kernel<2, 4096> / tile_backward_kernel<2, 4096> through the four tile modes -- tile lists, group lists
    only, record ranges, the per-point walk -- on the c = 2 scenes of tests/test_binned_matrix_gpu.py, each held to its
    mode by assert_mode on the plan that launched (the order-3 plan), with that file's bars."""
    import test_binned_matrix_gpu as BM
    cs = BM.scene(name, 2).on_device((name, 2, "vorticity fit"))
    exp, args, M = cs.exp, cs.args, cs.M
    s = cs.sampler()
    args_prev = [args[0], args[1], BM.round32(VR.other_values(args[2], 5)), args[3]]
    exp_prev = cs.oracle.forward(*args_prev, orders=ORDERS)
    tau, _ = cs.draw((M,))
    tau, tau64 = (tau + 1) / 2, np64((tau + 1) / 2)
    g3, g3_64 = cs.draw((M, 3))
    data64 = BM.round32(data_like(cs.rng, (exp, exp_prev), M))
    now7, prev7 = combine(exp), BM.round32(combine(exp_prev))
    cs.bind(s)
    out = fit_of(s, cs.dev(prev7), tau, cs.dev(data64))
    counts = BM.assert_mode(cs, s._plan3, hip_lib, s)
    print(f"{name}: plan with q_max {s._plan3.q_max:g}: tiles in LIST / RANGES / GROUPS / POINTS {counts}")
    assert tuple(out.shape) == (M, 3)
    BM.check_columns(cs, cs.mode + " forward", "vorticity fit", out, compose3(now7, prev7, tau64, NU, DT, TT, data64, DW),
                     bars3((exp, exp_prev)))
    got = torch.autograd.grad((out * g3).sum(), cs.leaves)
    want, mags = BM.oracle_grads(cs, expand(adjoint3(g3_64, now7, prev7, tau64, NU, DT, TT, DW)))
    cs.check_grads(cs.mode + " backward", ("vorticity fit", "gradient"), got, want, mags)
    cs.w.report()


# ------------------------------------------------------------------------------------------
# 3. periodic (-1, 1)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_periodic_matches_the_oracle_on_the_images(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    means, values, con, pts, _ = periodic_problem()
    rng = np.random.default_rng(32)
    t = leaves_of(means, values, con)
    pts_t = dev32(pts)
    M = len(pts)
    tau_t, gout_t = dev32(rng.uniform(0, 1, M)), dev32(rng.uniform(-1, 1, (M, 3)))
    args = oracle_args(t, pts_t)
    exp = periodic_forward(*args)
    exp_prev = periodic_forward(args[0], args[1], np64(dev32(VR.other_values(values, 9))), args[3])
    prev_t, data_t = dev32(combine(exp_prev)), dev32(data_like(rng, (exp, exp_prev), M))
    s = GaussianSampler(True, backend=backend, host=host, periodic=(-1.0, 1.0))       # debug mode: runs clean
    s.preprocess(t[0], t[1], None, t[2], pts_t)
    assert (s._plan is not None) == (backend == "binned")
    assert s._inputs[0].shape == (9 * 64, 2)
    out = fit_of(s, prev_t, tau_t, data_t)
    now7, prev7, tau, gout, data = combine(exp), np64(prev_t), np64(tau_t), np64(gout_t), np64(data_t)
    errs = VR.column_errors(out, compose3(now7, prev7, tau, NU, DT, TT, data, DW), bars3((exp, exp_prev)))
    print(f"periodic {backend}: forward (div, r, fit) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < 1e-5, errs
    g = torch.autograd.grad((out * gout_t).sum(), t)
    assert g[0].shape == (64, 2) and g[1].shape == (64, 2) and g[2].shape == (64, 3)
    check_periodic_grads((g[0], g[2], g[1]), *args, expand(adjoint3(gout, now7, prev7, tau, NU, DT, TT, DW)), torch.float32)


# ------------------------------------------------------------------------------------------
# 4. against the sampler's own vorticity_residual() and vorticity_terms()
# ------------------------------------------------------------------------------------------
def lattice_problem(**k):
    t, pts, w, tau, pv = VR.lattice_problem(**k)
    gen = torch.Generator().manual_seed(11)
    M = pts.shape[0]
    return t, pts, torch.cat((w, (torch.rand((M, 1), generator=gen) * 2 - 1).cuda()), 1), tau, pv, \
        ((torch.rand(M, generator=gen) * 2 - 1) * 30).cuda()


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_equals_the_samplers_own_composition(hip_lib, host, backend):
    """Columns 0-1 are those of vorticity_residual() without data on the same plan -- the same launch variant, so the same
    bits; column 2 and the gradients are torch's on the outputs of the existing kernels."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, pv, data = lattice_problem()
    assert variants_of(torch.float32, t[0].shape[0], pts.shape[0]) == variants_of(torch.float32, t[0].shape[0], pts.shape[0], 512)
    prev = VR.previous_level(t, pv, pts, backend, host)
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    out = fit_of(s, prev, tau, data)
    g_out = torch.autograd.grad((out * w).sum(), t)
    two = VR.residual_of(s, prev, tau)
    assert torch.equal(out.detach()[:, :2], two.detach())
    now = s.vorticity_terms()
    comp = torch.cat((VR.torch_lines(now, prev, tau), (DW * (now[:, 3] - data)).reshape(-1, 1)), 1)
    g_comp = torch.autograd.grad((comp * w).sum(), t)
    sc = VR.term_scales((now, prev))
    sc = torch.cat((sc, DW * sc[:1]))
    fwd = float(((out - comp).detach().abs().max(0).values / sc).max())
    grads = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_out, g_comp)]
    print(f"own composition ({backend}): forward {fwd:.3g} of the column scale, gradients {grads}")
    assert fwd < 2e-6, fwd
    assert max(grads) < 1e-5, grads


# ------------------------------------------------------------------------------------------
# 5. special values
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_special_values(hip_lib, backend):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, pv, data = lattice_problem(M=700, n=12)
    prev = VR.previous_level(t, pv, pts, backend, "ctypes")
    s = GaussianSampler(False, backend=backend)
    s.preprocess(t[0], t[1], None, t[2], pts)
    # data_weight = 0: exact zeros in column 2, the gradients of the call without data
    out = fit_of(s, prev, tau, data, dw=0.0)
    assert not out[:, 2].any()
    g0 = torch.autograd.grad((out * w).sum(), t)
    g1 = torch.autograd.grad((VR.residual_of(s, prev, tau) * w[:, :2]).sum(), t)
    assert max(rel(a, b) for a, b in zip(g0, g1)) < 2e-6                  # the backward's atomics, as between any two runs
    # nu = dt = time_term = 0: exact zeros in column 1 (the initialisation fit)
    out = fit_of(s, None, 1.0, data, dw=1.0, nu=0.0, dt=0.0, tt=0.0)
    assert not out[:, 1].any()
    now = s.vorticity_terms().detach()
    sc = VR.term_scales((now, torch.zeros_like(now)))
    assert float((out.detach()[:, 0] - now[:, 2]).abs().max() / sc[0]) < 2e-6
    assert float((out.detach()[:, 2] - (now[:, 3] - data)).abs().max() / sc[0]) < 2e-6
    g0 = torch.autograd.grad((out[:, 2] * w[:, 2]).sum(), t)
    g1 = torch.autograd.grad((s.vorticity_terms()[:, 3] * w[:, 2]).sum(), t)
    assert max(rel(a, b) for a, b in zip(g0, g1)) < 1e-5
    # data = the float64 oracle's w: column 2 within its bar of zero
    args = oracle_args(t, pts)
    exp = c_oracle.forward(*args, orders=ORDERS)
    w64 = combine(exp)[:, 3]
    out = fit_of(s, prev, tau, dev32(w64))
    S1 = np.abs(exp[1]).max()
    err = np.abs(np64(out[:, 2]) - DW * (w64 - np64(dev32(w64)))).max() / (DW * S1)
    print(f"data = the oracle's w ({backend}): column 2 at {err:.3g} of its scale")
    assert err < (1e-5 if backend == "dense" else TOL)


# ------------------------------------------------------------------------------------------
# 6. host parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hosts_agree_bitwise(hip_lib, dtype):
    """Same C ABI, same launches: bit-identical outputs and gradients (N = 200, M = 32: staged32, one slice)."""
    from diff_gaussian_sampling import GaussianSampler
    means, values, con, pts, g7 = dense_inputs(200, 32, 5)
    assert hp.dense("float32", 2, 2, MASK, 200, 32).backward == "staged32"
    prev, tau, gout = dev(g7[::-1].copy(), dtype), dev(np.abs(g7[:, 0]), dtype), dev(g7[:, 1:4], dtype)
    data = dev(30 * g7[:, 5], dtype)
    res = {}
    for host in HOSTS:
        t = leaves_of(means, values, con, dtype)
        s = GaussianSampler(False, backend="dense", host=host)
        s.preprocess(t[0], t[1], None, t[2], dev(pts, dtype))
        out = fit_of(s, prev, tau, data)
        res[host] = (out.detach(),) + torch.autograd.grad((out * gout).sum(), t)
    for a, b in zip(res["native"], res["ctypes"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------
# 7. autograd behaviour
# ------------------------------------------------------------------------------------------
def small(M=700, seed=4, grad=True, n=12):
    t, pts, w, tau, prev = VR.small(M=M, seed=seed, grad=grad, n=n)
    gen = torch.Generator().manual_seed(seed + 100)
    return t, pts, torch.cat((w, (torch.rand((M, 1), generator=gen) * 2 - 1).cuda()), 1), tau, prev, \
        ((torch.rand(M, generator=gen) * 2 - 1) * 30).cuda()


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_node_owns_its_inputs_and_plan(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev, data = small()
    s = GaussianSampler(True, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    out = fit_of(s, prev, tau, data)
    assert fit_of(s, prev, tau, data) is not out                       # never cached: the arguments vary
    loss = (out * w).sum()
    g1 = torch.autograd.grad(loss, t, retain_graph=True)
    # a later preprocess (other Gaussians, other points) before the second backward of the same graph
    t2, pts2, _, tau2, prev2, data2 = small(M=333, seed=9)
    s.preprocess(t2[0], t2[1], None, t2[2], pts2)
    assert tuple(fit_of(s, prev2, tau2, data2.reshape(-1, 1)).shape) == (333, 3)
    # an in-place write to the data after the forward is allowed: the backward does not read it
    data.fill_(float("nan"))
    g2 = torch.autograd.grad(loss, t, retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.isfinite(b).all() and rel(a, b) < 2e-6            # the backward's atomics, as between any two runs
    with torch.no_grad():
        t[0].add_(0.0)                                                 # an in-place write, whatever it writes
    with pytest.raises(RuntimeError, match="modified in place"):
        torch.autograd.grad(loss, t)


@pytest.mark.parametrize("host", HOSTS)
def test_differentiable_call_rebuilds_a_forward_only_plan(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev, data = small(M=3000)
    full = GaussianSampler(True, backend="binned", host=host)
    full.preprocess(t[0], t[1], None, t[2], pts)
    g_full = torch.autograd.grad((fit_of(full, prev, tau, data) * w).sum(), t)
    assert not full._plan3.forward_only
    lazy = GaussianSampler(True, backend="binned", host=host)
    with torch.no_grad():
        lazy.preprocess(t[0], t[1], None, t[2], pts)
        r0 = fit_of(lazy, prev, tau, data)                             # served by forward-only plans
        before, before3 = lazy._plan, lazy._plan3
        assert before.forward_only and before3.forward_only and r0.grad_fn is None
    r = fit_of(lazy, prev, tau, data)                                  # differentiable: both plans rebuilt in full
    assert r.grad_fn is not None
    assert lazy._plan is not before and lazy._plan3 is not before3
    assert not lazy._plan.forward_only and not lazy._plan3.forward_only
    assert float((r.detach() - r0).abs().max()) <= 1e-6 * float(r0.abs().max())
    g_lazy = torch.autograd.grad((r * w).sum(), t[0])
    assert torch.isfinite(g_lazy[0]).all() and rel(g_lazy[0], g_full[0]) < 1e-5


def test_no_grad_call_allocates_no_aux(hip_lib):
    from pigs_amd import host_ctypes as S
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev, data = small()
    seen = []
    real = S._fused_call

    def spy(op, backward, *a, **k):
        seen.append((op.forward_name, backward, k.get("aux")))
        return real(op, backward, *a, **k)

    s = GaussianSampler(False, backend="dense", host="ctypes")
    S._fused_call = spy
    try:
        with torch.no_grad():
            s.preprocess(t[0], t[1], None, t[2], pts)
            out = fit_of(s, prev, tau, data)
        assert out.grad_fn is None and seen == [("pigs_vorticity_fit_forward", False, None)]
        s.preprocess(t[0], t[1], None, t[2], pts)
        out = fit_of(s, prev, tau, data)
        assert seen[1][2] is not None and tuple(seen[1][2].shape) == (700, 4) and out.grad_fn is not None
    finally:
        S._fused_call = real


def test_backward_on_forward_only_workspace_writes_nan(hip_lib):
    """The C ABI: pigs_vorticity_fit_backward on a PIGS_BUILD_FORWARD_ONLY workspace writes NaN gradients, as the sibling
    does; the forward on it serves."""
    from pigs_amd import _lib
    from pigs_amd import host_ctypes as S
    t, pts, w, tau, prev, data = small(M=3000, grad=False, n=32)
    m, v, c = (x.contiguous() for x in t)
    N, M = m.shape[0], pts.shape[0]
    plan = S.Plan(m, v, c, pts, 44.0, q_max_backward=44.0, forward_only=True)
    full = S.Plan(m, v, c, pts, 44.0, q_max_backward=44.0)
    assert plan.forward_only and not full.forward_only
    params = S.VorticityFit(NU, DT, TT, tau.reshape(-1, 1).contiguous(), data, DW)
    aux = torch.empty((M, 4), device="cuda")
    op = S._VorticityFitFunction.op
    out = S._fused_call(op, False, m, v, c, pts, params, plan, side=prev, aux=aux)
    ref = S._fused_call(op, False, m, v, c, pts, params, full, side=prev)
    assert tuple(out.shape) == (M, 3)
    assert torch.isfinite(out).all() and torch.isfinite(aux).all() and rel(out, ref) < 1e-6
    gm, gv, gc = (torch.zeros_like(x) for x in (m, v, c))
    p, sws, vz = ctypes.c_void_p, plan.samples.workspace, params.struct()
    rc = hip_lib.pigs_vorticity_fit_backward(0, N, M, p(m.data_ptr()), p(c.data_ptr()), p(v.data_ptr()), p(pts.data_ptr()),
                                             ctypes.byref(vz), p(w.data_ptr()), p(aux.data_ptr()), p(gm.data_ptr()),
                                             p(gc.data_ptr()), p(gv.data_ptr()), p(plan.workspace.data_ptr()),
                                             plan.workspace.numel(), p(sws.data_ptr()), sws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(gm.isnan().all()) and bool(gv.isnan().all()) and bool(gc.isnan().all())
    assert isinstance(vz, _lib.PigsVorticityFit)
    for x, y in zip(S._fused_call(op, True, m, v, c, pts, params, full, gout=w, aux=aux),
                    S._fused_call(op, True, m, v, c, pts, params, plan, gout=w, aux=aux)):
        assert torch.isfinite(x).all() and rel(y, x) < 1e-5


# ------------------------------------------------------------------------------------------
# 8. empty inputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_inputs(hip_lib, host, dtype):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev, data = small(M=50)
    t = [x.detach().to(dtype).requires_grad_(True) for x in t]
    tau, prev, data = tau.to(dtype), prev.to(dtype), data.to(dtype)
    s = GaussianSampler(True, host=host)
    # M = 0
    s.preprocess(t[0], t[1], None, t[2], pts[:0].to(dtype))
    out = fit_of(s, prev[:0], tau[:0], data[:0])
    assert tuple(out.shape) == (0, 3) and out.dtype == dtype
    g = torch.autograd.grad(out.sum(), t)
    assert all(tuple(a.shape) == tuple(x.shape) and not a.any() for a, x in zip(g, t))
    # N = 0: the composition of prev and the data alone
    e = [x.detach()[:0].clone().requires_grad_(True) for x in t]
    s.preprocess(e[0], e[1], None, e[2], pts.to(dtype))
    out = fit_of(s, prev, tau, data)
    want = compose3(np.zeros((50, 7)), np64(prev), np64(tau), NU, DT, TT, np64(data), DW)
    assert tuple(out.shape) == (50, 3)
    assert np.abs(np64(out) - want).max() <= (1e-6 if dtype == torch.float32 else 1e-14) * np.abs(want).max()
    g = torch.autograd.grad(out.sum(), e)
    assert [tuple(a.shape) for a in g] == [(0, 2), (0, 2), (0, 3)]


# ------------------------------------------------------------------------------------------
# 9. error paths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
def test_unsupported_inputs_raise(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd import synthetic
    s = GaussianSampler(False, host=host)
    pts = torch.rand((40, 2)).cuda()
    data = torch.zeros(40).cuda()
    with pytest.raises(RuntimeError, match="preprocess"):
        s.vorticity_residual(NU, DT, data=data)
    for c in (1, 3):
        gs = synthetic.lattice_gaussians(6, 6, 1.0, seed=1, c=c)
        s.preprocess(gs["means"].float().cuda(), gs["values"].float().cuda(), None, gs["conics"].float().cuda(), pts)
        with pytest.raises(NotImplementedError, match="two-channel"):
            s.vorticity_residual(NU, DT, data=data)
    line = synthetic.line_gaussians_1d(16)
    s.preprocess(line["means"].float().cuda(), line["values"].float().cuda().expand(16, 2).contiguous(), None,
                 line["conics"].float().cuda(), torch.rand((40, 1)).cuda())
    with pytest.raises(NotImplementedError, match="two dimensions"):
        s.vorticity_residual(NU, DT, data=data)
    gs = synthetic.lattice_gaussians(6, 6, 1.0, seed=1, c=2)
    s.preprocess(gs["means"].float().cuda(), gs["values"].float().cuda(), None, gs["conics"].float().cuda(), pts)
    with pytest.raises(ValueError, match="data must have shape"):
        s.vorticity_residual(NU, DT, data=torch.zeros(39).cuda())
    with pytest.raises(ValueError, match="data must have shape"):
        s.vorticity_residual(NU, DT, data=torch.zeros((40, 2)).cuda())
    with pytest.raises(RuntimeError, match="device"):
        s.vorticity_residual(NU, DT, data=torch.zeros(40))
    with pytest.raises(ValueError, match="data"):
        s.vorticity_residual(NU, DT, data=data.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="prev must have shape"):
        s.vorticity_residual(NU, DT, torch.zeros((40, 6)).cuda(), data=data)
    assert tuple(s.vorticity_residual(NU, DT, data=data.double().reshape(40, 1)).shape) == (40, 3)
    assert tuple(s.vorticity_residual(NU, DT).shape) == (40, 2)                       # data=None: nothing changes


# ------------------------------------------------------------------------------------------
# 10. graph capture
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_graphed_step_matches_eager(hip_lib, host, backend):
    """preprocess + vorticity_residual(data=) + loss + gradients captured once and replayed with the data (and the values)
    rewritten in place between replays, against the same step issued eagerly: nothing in the call synchronises."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    t, pts, _, tau, prev, data = small(M=2000, grad=False)
    sampler = GaussianSampler(False, backend=backend, host=host)

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in t)

    def fn(means, values, conics):
        sampler.preprocess(means, values, None, conics, pts)
        loss = sampler.vorticity_residual(NU, DT, prev, tau, data=data, data_weight=DW).pow(2).mean(0).sum()
        return (loss,) + torch.autograd.grad(loss, (means, values, conics))

    step = GraphedStep(fn, make_inputs)
    gen = torch.Generator().manual_seed(9)
    losses = []
    for trial in range(2):
        with torch.no_grad():
            step.inputs[1].copy_((torch.rand(t[1].shape, generator=gen) * 2 - 1).cuda())
            data.copy_(((torch.rand(data.shape, generator=gen) * 2 - 1) * 30).cuda())
        got = [x.clone() for x in step()]
        torch.cuda.synchronize()
        m, v, c = (x.detach().clone().requires_grad_(True) for x in step.inputs)
        eager = fn(m, v, c)
        for k, (a, b) in enumerate(zip(got, eager)):
            assert rel(a, b) < 2e-6, (trial, k, rel(a, b))
        losses.append(float(got[0]))
    assert losses[0] != losses[1]


# ------------------------------------------------------------------------------------------
# 11. end to end: five steps of the initialisation fit (test_initialize.py:112-114, 131-136, 172-180, "f" mode)
# ------------------------------------------------------------------------------------------
def test_initialisation_fit_matches_the_references_lines(hip_lib):
    """GaussianAdam(means_map="identity", wrap=(-1, 1)) on a periodic sampler, N = 100, c = 2, M = 1 024 fresh points a
    step: the loss through vorticity_residual(0, 0, None, 1, time_term=0, data=grid_lookup(image, samples)) against the
    same five steps through sample_gaussians_derivative() and the reference's lines.  The losses agree step by step within
    the float32 bar of the loss's scale (1e-5: every term is a mean of squares of first derivatives at their 1e-5), the
    parameters after five steps within 2e-3 of each tensor's scale, the bar tests/test_optim_gpu.py holds a trajectory of
    eager steps against another to (test_capture_of_the_whole_step, test_loss_curve_matches_the_reference_functions)."""
    import pigs_amd
    from diff_gaussian_sampling import GaussianSampler
    res, N, M, steps = 64, 100, 1024, 5
    gen = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, res), torch.linspace(-1, 1, res), indexing="ij")
    img = (torch.sin(3.0 * xx) * torch.cos(2.0 * yy) * 4.0).cuda()
    points = [(torch.rand((M, 2), generator=gen) * 2 - 1).cuda() for _ in range(steps)]
    side = 10
    g = (torch.arange(side, dtype=torch.float32) + 0.5) / side * 2 - 1
    means0 = torch.stack(torch.meshgrid(g, g, indexing="xy"), -1).reshape(N, 2) + 0.01 * (torch.rand((N, 2), generator=gen) - 0.5)
    init = dict(means=means0, values=0.1 * (torch.rand((N, 2), generator=gen) * 2 - 1),
                scaling=torch.full((N, 2), -2.5) + 0.1 * torch.rand((N, 2), generator=gen),
                transform=0.1 * (torch.rand((N, 1), generator=gen) * 2 - 1))

    def run(fused):
        opt = pigs_amd.GaussianAdam(init["means"].cuda(), init["values"].cuda(), init["scaling"].cuda(), init["transform"].cuda(),
                                    lr=1e-2, means_map="identity", wrap=(-1.0, 1.0))
        s = GaussianSampler(False, backend="dense", periodic=(-1.0, 1.0))
        losses = []
        for samples in points:
            g = opt.gaussians()
            s.preprocess(g.means, g.values, g.covariances, g.conics, samples)
            if fused:
                out = s.vorticity_residual(0.0, 0.0, None, 1.0, time_term=0.0, data=pigs_amd.grid_lookup(img, samples))
                loss = out[:, 2].pow(2).mean() + out[:, 0].pow(2).mean()
            else:
                ux = s.sample_gaussians_derivative()
                vorticity = ux[:, 0, 1] - ux[:, 1, 0]                                      # test_initialize.py:112-114
                divergence = ux[:, 0, 0] + ux[:, 1, 1]
                coords = ((samples + 1.0) / 2.0 * res).to(torch.long).clamp(0, res - 1)     # :132-133
                coords = coords[:, 1] * res + coords[:, 0]
                loss = torch.mean((vorticity - torch.take(img, coords)) ** 2) + torch.mean(divergence ** 2)      # :135-136
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return losses, [p.detach().clone() for p in (opt.raw_means, opt.values, opt.raw_scaling, opt.transform)]

    (l_ref, p_ref), (l_got, p_got) = run(False), run(True)
    scale = max(abs(x) for x in l_ref)
    errs = [abs(a - b) / scale for a, b in zip(l_got, l_ref)]
    perr = [rel(a, b) for a, b in zip(p_got, p_ref)]
    print("losses", l_ref, "differences of the scale", errs, "parameters (means, values, scaling, transform)", perr)
    assert l_ref[-1] < l_ref[0]
    assert max(errs) < 1e-5, errs
    assert max(perr) < 2e-3, perr
