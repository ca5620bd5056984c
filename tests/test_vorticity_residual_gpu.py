"""GPU: GaussianSampler.vorticity_residual() -- (div_b, r) of the reference's Navier-Stokes loss in one launch each way
(pair_math.h ORDN, pigs_vorticity_residual_*; model_pn.py:794-818, 629-631, 830, 848-849).

Expected values: compose() of the float64 oracle's orders 0..3 of two time levels (tests/test_vorticity_residual.py; the
previous level: the same means and conics with other values, so both levels have the same scale; tau uniform in [0, 1]
per point); expected gradients: the oracle's backward fed with expand(adjoint(gout, ...)).

Bars, none of them new.  With S_k = max |o_k| over both levels:
  div            1e-5 S_1 (float32), 1e-11 S_1 (float64)
  r              the same fractions of |time_term| S_1 + |dt| (nu S_3 + 4 S_0 S_2): what the seven columns' own 1e-5 bars
                 propagate to through compose (each of the two products has two factors)
  gradients      1e-5 of the tensor's largest entry + conftest.grads_within_accumulation_bound with its defaults;
                 float64 1e-11
  binned         TOL of tests/test_binned_gpu.py
  own composition (vorticity_terms() + the torch lines of INTEGRATION.md 3 + torch.autograd, same plan): 2e-6 / 1e-5

Measured worst values on an MI355X: not recorded yet; every case prints its figures before it asserts."""
import ctypes
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
from test_vorticity import combine, expand
from test_vorticity_gpu import (DENSE_CASES, DENSE_SHAPES, HOSTS, ORDERS, binned_problem, dense_inputs, dev, leaves_of, np64,
                                oracle_args, periodic_problem, rel, small_problem, variants_of)
from test_vorticity_residual import adjoint, compose

pytestmark = pytest.mark.gpu
NU, DT, TT = 0.05, 0.01, 1.0


def bars(exps, nu=NU, dt=DT, tt=TT):
    """The scales of the two columns (module docstring) from the oracle outputs of both levels."""
    S = [max(np.abs(e[k]).max() for e in exps) for k in range(4)]
    return np.array([S[1], abs(tt) * S[1] + abs(dt) * (nu * S[3] + 4 * S[0] * S[2])])


def column_errors(got, want, scales):
    return np.abs(np64(got) - want).max(0) / scales


def other_values(values, seed):
    return np.random.default_rng(seed).uniform(-1, 1, values.shape)


def check_f32_grads(got, args, g7):
    grads = expand(g7)
    want = c_oracle.backward(*args, grads)
    errs = [rel(g, w) for g, w in zip(got, want)]
    print("gradients (means, conics, values):", errs)
    assert max(errs) < 1e-5, errs
    bad = grads_within_accumulation_bound(got, args, grads)
    assert not bad, bad


def residual_of(s, prev, tau, nu=NU, dt=DT, tt=TT):
    return s.vorticity_residual(nu, dt, prev, tau, time_term=tt)


def torch_lines(now, prev, tau, nu=NU, dt=DT, tt=TT):
    """INTEGRATION.md 3, the composition in torch from two [M, 7] rows."""
    tau1 = tau.reshape(-1, 1) if isinstance(tau, torch.Tensor) else tau
    u_x, u_y, div, _, w_x, w_y, lap_w = (tau1 * now + (1 - tau1) * prev).unbind(1)
    r = tt * (now[:, 3] - prev[:, 3]) - dt * (nu * lap_w - (u_x * w_x + u_y * w_y))
    return torch.stack((div, r), -1)


def term_scales(rows, nu=NU, dt=DT, tt=TT):
    """The two columns' scales from [M, 7] rows of the sampler itself (own-composition cases)."""
    a = torch.cat([r.detach().abs() for r in rows]).max(0).values.double().cpu().numpy()
    S0, S1, S2, S3 = max(a[0], a[1]), max(a[2], a[3]), max(a[4], a[5]), a[6]
    return torch.tensor([S1, abs(tt) * S1 + abs(dt) * (nu * S3 + 4 * S0 * S2)], device="cuda")


# ------------------------------------------------------------------------------------------
# 1. dense, every launch variant
# ------------------------------------------------------------------------------------------
def test_the_dense_cases_reach_every_variant():
    """FwdLayout::N is 7 for ORDV and ORDN alike: the launchers pick the variants of tests/test_vorticity_gpu.py."""
    assert [variants_of(t, N, M) for t, N, M in DENSE_CASES] == [
        ("w4", "staged32"), ("rows", "staged32"), ("w16", "split_atomic"), ("w16", "split_atomic"), ("rows", "staged64"),
        ("w4", "staged32"), ("rows", "staged32"), ("w4", "split_atomic")]
    assert DENSE_SHAPES == [(33, 81), (161, 81), (100, 19201), (1300, 16400), (1300, 5501)]


@functools.lru_cache(maxsize=None)
def dense_expectation(dtype, N, M):
    means, values, con, pts, _ = dense_inputs(N, M, N + M)
    rng = np.random.default_rng(N * 7 + M)
    rnd = (lambda a: np64(dev(a, dtype)))
    args = [rnd(means), rnd(con), rnd(values), rnd(pts)]
    args_prev = [args[0], args[1], rnd(other_values(values, N)), args[3]]
    tau, gout = rnd(rng.uniform(0, 1, M)), rnd(rng.uniform(-1, 1, (M, 2)))
    exp, exp_prev = c_oracle.forward(*args, orders=ORDERS), c_oracle.forward(*args_prev, orders=ORDERS)
    now7, prev7 = combine(exp), rnd(combine(exp_prev))
    want = compose(now7, prev7, tau, NU, DT, TT)
    g7 = adjoint(gout, now7, prev7, tau, NU, DT, TT)
    return args, prev7, tau, gout, want, bars((exp, exp_prev)), g7, c_oracle.backward(*args, expand(g7))


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,N,M", DENSE_CASES)
def test_dense_matches_the_oracle(hip_lib, host, dtype, N, M):
    from diff_gaussian_sampling import GaussianSampler
    args, prev7, tau, gout, want, scales, g7, want_g = dense_expectation(dtype, N, M)
    t = leaves_of(args[0], args[2], args[1], dtype)
    s = GaussianSampler(True, backend="dense", host=host)
    s.preprocess(t[0], t[1], None, t[2], dev(args[3], dtype))
    assert s._plan is None
    out = residual_of(s, dev(prev7, dtype), dev(tau, dtype))
    assert tuple(out.shape) == (M, 2) and out.dtype == dtype and out.is_contiguous()
    errs = column_errors(out, want, scales)
    print(f"{variants_of(dtype, N, M)} forward (div, r) of their scales: {np.array2string(errs, precision=2)}")
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
# 2. binned
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def binned_expectation(points):
    args, _, exp = binned_problem(points)
    M = len(args[3])
    rng = np.random.default_rng(21)
    args_prev = [args[0], args[1], np64(dev32(other_values(args[2], 5))), args[3]]
    exp_prev = c_oracle.forward(*args_prev, orders=ORDERS)
    tau = np64(dev32(rng.uniform(0, 1, M)))
    gout = np.zeros((M, 2))
    gout[::7] = rng.uniform(-1, 1, (len(range(0, M, 7)), 2))                  # a loss supported on every 7th point
    gout = np64(dev32(gout))
    now7, prev7 = combine(exp), np64(dev32(combine(exp_prev)))
    return (args, prev7, tau, gout, compose(now7, prev7, tau, NU, DT, TT), bars((exp, exp_prev)),
            adjoint(gout, now7, prev7, tau, NU, DT, TT))


@pytest.mark.parametrize("points", ["lattice", "random", "small"])
def test_binned_matches_the_oracle(hip_lib, points):
    from diff_gaussian_sampling import GaussianSampler
    args, prev7, tau, gout, want, scales, g7 = binned_expectation(points)
    assert args[0].shape[0] == 1024
    t = leaves_of(args[0], args[2], args[1])
    s = GaussianSampler(True, backend="binned")
    s.preprocess(t[0], t[1], None, t[2], dev32(args[3]))
    assert s._plan is not None
    out = residual_of(s, dev32(prev7), dev32(tau))
    assert s._plan3 is not None and s._plan3.q_max == pytest.approx(s.q_max_order3)
    errs = column_errors(out, want, scales)
    print(f"binned {points}: forward (div, r) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < TOL, errs
    g = torch.autograd.grad((out * dev32(gout)).sum(), t)
    check_f32_grads((g[0], g[2], g[1]), args, g7)


# ------------------------------------------------------------------------------------------
# 3. periodic (-1, 1)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_periodic_matches_the_oracle_on_the_images(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    means, values, con, pts, _ = periodic_problem()
    rng = np.random.default_rng(31)
    t = leaves_of(means, values, con)
    pts_t = dev32(pts)
    M = len(pts)
    tau_t, gout_t = dev32(rng.uniform(0, 1, M)), dev32(rng.uniform(-1, 1, (M, 2)))
    args = oracle_args(t, pts_t)
    exp = periodic_forward(*args)
    exp_prev = periodic_forward(args[0], args[1], np64(dev32(other_values(values, 9))), args[3])
    prev_t = dev32(combine(exp_prev))
    s = GaussianSampler(True, backend=backend, host=host, periodic=(-1.0, 1.0))       # debug mode: runs clean
    s.preprocess(t[0], t[1], None, t[2], pts_t)
    assert (s._plan is not None) == (backend == "binned")
    assert s._inputs[0].shape == (9 * 64, 2)
    out = residual_of(s, prev_t, tau_t)
    now7, prev7, tau, gout = combine(exp), np64(prev_t), np64(tau_t), np64(gout_t)
    errs = column_errors(out, compose(now7, prev7, tau, NU, DT, TT), bars((exp, exp_prev)))
    print(f"periodic {backend}: forward (div, r) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < 1e-5, errs
    g = torch.autograd.grad((out * gout_t).sum(), t)
    assert g[0].shape == (64, 2) and g[1].shape == (64, 2) and g[2].shape == (64, 3)
    check_periodic_grads((g[0], g[2], g[1]), *args, expand(adjoint(gout, now7, prev7, tau, NU, DT, TT)), torch.float32)


# ------------------------------------------------------------------------------------------
# 4. against the sampler's own vorticity_terms() composed in torch
# ------------------------------------------------------------------------------------------
def lattice_problem(M=1531, n=20, seed=5):
    gs = synthetic.lattice_gaussians(n, n, 1.1, seed=seed, c=2)
    t = leaves_of(gs["means"].numpy(), gs["values"].numpy(), gs["conics"].numpy())
    rng = np.random.default_rng(2)
    pts, w, tau = dev32(rng.uniform(-1, 1, (M, 2))), dev32(rng.uniform(-1, 1, (M, 2))), dev32(rng.uniform(0, 1, M))
    return t, pts, w, tau, dev32(rng.uniform(-1, 1, gs["values"].shape))


def previous_level(t, prev_values, pts, backend, host):
    from diff_gaussian_sampling import GaussianSampler
    with torch.no_grad():
        s0 = GaussianSampler(False, backend=backend, host=host)
        s0.preprocess(t[0].detach(), prev_values, None, t[2].detach(), pts)
        return s0.vorticity_terms().clone()


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_equals_the_composition_of_the_samplers_own_terms(hip_lib, host, backend):
    """A column or a sign wired wrongly, which a helper shared with the kernel's author might hide, cannot hide here: the
    composition is torch's on the outputs of the existing vorticity_terms() kernels, the gradients torch.autograd's."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, pv = lattice_problem()
    prev = previous_level(t, pv, pts, backend, host)
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    out = residual_of(s, prev, tau)
    g_out = torch.autograd.grad((out * w).sum(), t)
    now = s.vorticity_terms()
    comp = torch_lines(now, prev, tau)
    g_comp = torch.autograd.grad((comp * w).sum(), t)
    fwd = float(((out - comp).detach().abs().max(0).values / term_scales((now, prev))).max())
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
    t, pts, w, tau, pv = lattice_problem(M=700, n=12)
    prev = previous_level(t, pv, pts, backend, "ctypes")
    s = GaussianSampler(False, backend=backend)
    s.preprocess(t[0], t[1], None, t[2], pts)
    now = s.vorticity_terms()
    u_x, u_y, div, vort, w_x, w_y, lap_w = now.detach().unbind(1)
    zero = torch.zeros_like(prev)
    # tau = 1, no prev: the backward rule on a zero previous level
    out = residual_of(s, None, 1.0)
    sc = term_scales((now, zero))
    assert float((out[:, 0] - div).abs().max() / sc[0]) < 2e-6
    assert float((out[:, 1] - (vort - DT * (NU * lap_w - (u_x * w_x + u_y * w_y)))).abs().max() / sc[1]) < 2e-6
    # time_term = 0, dt = -1: the right-hand side of Model.forward
    out = residual_of(s, None, 1.0, nu=0.3, dt=-1.0, tt=0.0)
    sc = term_scales((now, zero), nu=0.3, dt=-1.0, tt=0.0)
    assert float((out[:, 1] - (0.3 * lap_w - (u_x * w_x + u_y * w_y))).abs().max() / sc[1]) < 2e-6
    # tau = 0 as a field (the forward rule): only time_term * w depends on the bound Gaussians
    out = residual_of(s, prev, torch.zeros_like(tau), tt=-2.5)
    g0 = torch.autograd.grad((out * w).sum(), t)
    g1 = torch.autograd.grad((-2.5 * now[:, 3] * w[:, 1]).sum(), t)
    assert max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g0, g1)) < 1e-5
    sc = term_scales((now, prev), tt=-2.5)
    assert float((out.detach() - torch_lines(now.detach(), prev, 0.0, tt=-2.5)).abs().max(0).values.div(sc).max()) < 2e-6
    # a float tau and the equal constant field
    a, b = residual_of(s, prev, 0.3), residual_of(s, prev, torch.full_like(tau, 0.3).reshape(-1, 1))
    assert float(((a - b).detach().abs().max(0).values / term_scales((now, prev))).max()) < 2e-6
    ga, gb = torch.autograd.grad((a * w).sum(), t), torch.autograd.grad((b * w).sum(), t)
    assert max(rel(x, y) for x, y in zip(ga, gb)) < 2e-6


# ------------------------------------------------------------------------------------------
# 6. host parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hosts_agree_bitwise(hip_lib, dtype):
    """Same C ABI, same launches: bit-identical outputs and gradients (N = 200, M = 32: staged32, one slice)."""
    from diff_gaussian_sampling import GaussianSampler
    means, values, con, pts, g7 = dense_inputs(200, 32, 5)
    import host_program as hp
    assert hp.dense("float32", 2, 2, 512, 200, 32).backward == "staged32"
    prev, tau, gout = dev(g7[::-1].copy(), dtype), dev(np.abs(g7[:, 0]), dtype), dev(g7[:, 1:3], dtype)
    res = {}
    for host in HOSTS:
        t = leaves_of(means, values, con, dtype)
        s = GaussianSampler(False, backend="dense", host=host)
        s.preprocess(t[0], t[1], None, t[2], dev(pts, dtype))
        out = residual_of(s, prev, tau)
        res[host] = (out.detach(),) + torch.autograd.grad((out * gout).sum(), t)
    for a, b in zip(res["native"], res["ctypes"]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------
# 7. autograd behaviour
# ------------------------------------------------------------------------------------------
def small(M=700, seed=4, grad=True, n=12):
    t, pts, w7 = small_problem(M=M, seed=seed, grad=grad, n=n)
    return t, pts, w7[:, :2].contiguous(), w7[:, 2].abs().contiguous(), w7.flip(0).contiguous()      # gout, tau, prev


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_node_owns_its_inputs_and_plan(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev = small()
    s = GaussianSampler(True, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    out = residual_of(s, prev, tau)
    assert residual_of(s, prev, tau) is not out                        # never cached: the arguments vary
    loss = (out * w).sum()
    g1 = torch.autograd.grad(loss, t, retain_graph=True)
    # a later preprocess (other Gaussians, other points) before the second backward of the same graph
    t2, pts2, _, tau2, prev2 = small(M=333, seed=9)
    s.preprocess(t2[0], t2[1], None, t2[2], pts2)
    assert tuple(residual_of(s, prev2, tau2).shape) == (333, 2)
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
    t, pts, w, tau, prev = small(M=3000)
    full = GaussianSampler(True, backend="binned", host=host)
    full.preprocess(t[0], t[1], None, t[2], pts)
    g_full = torch.autograd.grad((residual_of(full, prev, tau) * w).sum(), t)
    assert not full._plan3.forward_only
    lazy = GaussianSampler(True, backend="binned", host=host)
    with torch.no_grad():
        lazy.preprocess(t[0], t[1], None, t[2], pts)
        r0 = residual_of(lazy, prev, tau)                              # served by forward-only plans
        before, before3 = lazy._plan, lazy._plan3
        assert before.forward_only and before3.forward_only and r0.grad_fn is None
    r = residual_of(lazy, prev, tau)                                   # differentiable: both plans rebuilt in full
    assert r.grad_fn is not None
    assert lazy._plan is not before and lazy._plan3 is not before3
    assert not lazy._plan.forward_only and not lazy._plan3.forward_only
    assert float((r.detach() - r0).abs().max()) <= 1e-6 * float(r0.abs().max())
    g_lazy = torch.autograd.grad((r * w).sum(), t[0])
    assert torch.isfinite(g_lazy[0]).all() and rel(g_lazy[0], g_full[0]) < 1e-5


def test_no_grad_call_allocates_no_aux(hip_lib):
    from pigs_amd import host_ctypes as S
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev = small()
    seen = []
    real = S._fused_call

    def spy(op, backward, *a, **k):
        seen.append((backward, k.get("aux")))
        return real(op, backward, *a, **k)

    s = GaussianSampler(False, backend="dense", host="ctypes")
    S._fused_call = spy
    try:
        with torch.no_grad():
            s.preprocess(t[0], t[1], None, t[2], pts)
            out = residual_of(s, prev, tau)
        assert out.grad_fn is None and seen == [(False, None)]
        s.preprocess(t[0], t[1], None, t[2], pts)
        out = residual_of(s, prev, tau)
        assert seen[1][1] is not None and tuple(seen[1][1].shape) == (700, 4) and out.grad_fn is not None
    finally:
        S._fused_call = real


def test_backward_on_forward_only_workspace_writes_nan(hip_lib):
    """The C ABI: pigs_vorticity_residual_backward on a PIGS_BUILD_FORWARD_ONLY workspace writes NaN gradients, as every
    backward entry does; the forward on it serves."""
    from pigs_amd import _lib
    from pigs_amd import host_ctypes as S
    t, pts, w, tau, prev = small(M=3000, grad=False, n=32)
    m, v, c = (x.contiguous() for x in t)
    N, M = m.shape[0], pts.shape[0]
    plan = S.Plan(m, v, c, pts, 44.0, q_max_backward=44.0, forward_only=True)
    full = S.Plan(m, v, c, pts, 44.0, q_max_backward=44.0)
    assert plan.forward_only and not full.forward_only
    params = S.VorticityResidual(NU, DT, TT, tau.reshape(-1, 1).contiguous())
    aux = torch.empty((M, 4), device="cuda")
    op = S._VorticityResidualFunction.op
    out = S._fused_call(op, False, m, v, c, pts, params, plan, side=prev, aux=aux)
    ref = S._fused_call(op, False, m, v, c, pts, params, full, side=prev)
    assert torch.isfinite(out).all() and torch.isfinite(aux).all() and rel(out, ref) < 1e-6
    gm, gv, gc = (torch.zeros_like(x) for x in (m, v, c))
    p, sws, vz = ctypes.c_void_p, plan.samples.workspace, params.struct()
    rc = hip_lib.pigs_vorticity_residual_backward(0, N, M, p(m.data_ptr()), p(c.data_ptr()), p(v.data_ptr()), p(pts.data_ptr()),
                                                  ctypes.byref(vz), p(w.data_ptr()), p(aux.data_ptr()), p(gm.data_ptr()),
                                                  p(gc.data_ptr()), p(gv.data_ptr()), p(plan.workspace.data_ptr()),
                                                  plan.workspace.numel(), p(sws.data_ptr()), sws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(gm.isnan().all()) and bool(gv.isnan().all()) and bool(gc.isnan().all())
    assert isinstance(vz, _lib.PigsVorticityResidual)
    for x, y in zip(S._fused_call(op, True, m, v, c, pts, params, full, gout=w, aux=aux),
                    S._fused_call(op, True, m, v, c, pts, params, plan, gout=w, aux=aux)):
        assert torch.isfinite(x).all() and rel(y, x) < 1e-5


@pytest.mark.parametrize("host", HOSTS)
def test_constants_must_not_require_grad(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev = small(M=50)
    s = GaussianSampler(False, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    with pytest.raises(ValueError, match=r"vorticity_terms\(\)"):
        residual_of(s, prev.clone().requires_grad_(True), tau)
    with pytest.raises(ValueError, match="tau"):
        residual_of(s, prev, tau.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------
# 8. empty inputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_inputs(hip_lib, host, dtype):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, w, tau, prev = small(M=50)
    t = [x.detach().to(dtype).requires_grad_(True) for x in t]
    tau, prev = tau.to(dtype), prev.to(dtype)
    s = GaussianSampler(True, host=host)
    # M = 0
    s.preprocess(t[0], t[1], None, t[2], pts[:0].to(dtype))
    out = residual_of(s, prev[:0], tau[:0])
    assert tuple(out.shape) == (0, 2) and out.dtype == dtype
    g = torch.autograd.grad(out.sum(), t)
    assert all(tuple(a.shape) == tuple(x.shape) and not a.any() for a, x in zip(g, t))
    # N = 0: the composition of prev alone
    e = [x.detach()[:0].clone().requires_grad_(True) for x in t]
    s.preprocess(e[0], e[1], None, e[2], pts.to(dtype))
    out = residual_of(s, prev, tau)
    want = compose(np.zeros((50, 7)), np64(prev), np64(tau), NU, DT, TT)
    assert tuple(out.shape) == (50, 2)
    assert np.abs(np64(out) - want).max() <= (1e-6 if dtype == torch.float32 else 1e-14) * np.abs(want).max()
    g = torch.autograd.grad(out.sum(), e)
    assert [tuple(a.shape) for a in g] == [(0, 2), (0, 2), (0, 3)]


# ------------------------------------------------------------------------------------------
# 9. the overflow guard
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_far_points_of_a_nearly_singular_conic_stay_finite(hip_lib, backend):
    """The conics of tests/test_vorticity_gpu.py's test of the same name: g is exactly 0 where the cubic factor of lap_w
    overflows float32.  fwd_accumulate delegates to ORDV, so its `live` guard serves here too."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(12, 12, 1.0, seed=4, c=2)
    means, values, con = (gs[k].numpy().copy() for k in ("means", "values", "conics"))
    means[:2] = [[-0.9, -0.9], [-0.8, -0.95]]
    con[0] = [1e12, 1e12 * (1 - 1e-6), 1e12]
    con[1] = [4e12, 4e12 * (1 - 1e-6), 4e12]
    rng = np.random.default_rng(3)
    pts = np.concatenate((rng.uniform(-1, 1, (500, 2)), [[0.9, 0.9], [0.7, 0.99], [0.95, 0.95]]))
    t = leaves_of(means, values, con)
    pts_t = dev32(pts)
    tau_t = dev32(rng.uniform(0, 1, len(pts)))
    args = oracle_args(t, pts_t)
    exp = c_oracle.forward(*args, orders=ORDERS)
    exp_prev = c_oracle.forward(args[0], args[1], np64(dev32(other_values(values, 2))), args[3], orders=ORDERS)
    prev_t = dev32(combine(exp_prev))
    s = GaussianSampler(True, backend=backend)
    s.preprocess(t[0], t[1], None, t[2], pts_t)
    out = residual_of(s, prev_t, tau_t)
    assert torch.isfinite(out).all()
    want = compose(combine(exp), np64(prev_t), np64(tau_t), NU, DT, TT)
    assert np.isfinite(want).all()
    errs = column_errors(out, want, bars((exp, exp_prev)))
    print(f"overflow guard ({backend}): forward (div, r) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < 1e-5, errs
    g = torch.autograd.grad(out.sum(), t)
    assert all(torch.isfinite(a).all() for a in g)


# ------------------------------------------------------------------------------------------
# 10. error paths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
def test_unsupported_inputs_raise(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(False, host=host)
    with pytest.raises(RuntimeError, match="preprocess"):
        s.vorticity_residual(NU, DT)
    pts = torch.rand((40, 2)).cuda()
    for c in (1, 3):
        gs = synthetic.lattice_gaussians(6, 6, 1.0, seed=1, c=c)
        s.preprocess(gs["means"].float().cuda(), gs["values"].float().cuda(), None, gs["conics"].float().cuda(), pts)
        with pytest.raises(NotImplementedError, match="two-channel"):
            s.vorticity_residual(NU, DT)
    line = synthetic.line_gaussians_1d(16)
    s.preprocess(line["means"].float().cuda(), line["values"].float().cuda().expand(16, 2).contiguous(), None,
                 line["conics"].float().cuda(), torch.rand((40, 1)).cuda())
    with pytest.raises(NotImplementedError, match="two dimensions"):
        s.vorticity_residual(NU, DT)
    gs = synthetic.lattice_gaussians(6, 6, 1.0, seed=1, c=2)
    s.preprocess(gs["means"].float().cuda(), gs["values"].float().cuda(), None, gs["conics"].float().cuda(), pts)
    with pytest.raises(ValueError, match="prev must have shape"):
        s.vorticity_residual(NU, DT, torch.zeros((40, 6)).cuda())
    with pytest.raises(ValueError, match="prev must have shape"):
        s.vorticity_residual(NU, DT, torch.zeros((39, 7)).cuda())
    with pytest.raises(RuntimeError, match="device"):
        s.vorticity_residual(NU, DT, torch.zeros((40, 7)))
    with pytest.raises(ValueError, match="tau must have shape"):
        s.vorticity_residual(NU, DT, None, torch.zeros(39).cuda())
    assert tuple(s.vorticity_residual(NU, DT, torch.zeros((40, 7)).cuda(), torch.zeros((40, 1)).cuda()).shape) == (40, 2)


# ------------------------------------------------------------------------------------------
# 11. graph capture
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_graphed_step_matches_eager(hip_lib, host, backend):
    """preprocess + vorticity_residual + loss + gradients captured once and replayed after an in-place update of the
    values, against the same step issued eagerly: nothing in the call synchronises."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    t, pts, _, tau, prev = small(M=2000, grad=False)
    sampler = GaussianSampler(False, backend=backend, host=host)

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in t)

    def fn(means, values, conics):
        sampler.preprocess(means, values, None, conics, pts)
        loss = sampler.vorticity_residual(NU, DT, prev, tau).pow(2).mean(0).sum()
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
