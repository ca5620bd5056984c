"""GPU: GaussianSampler.residual() in its general form -- per-point coefficient fields and an advection term,

    w_i(m)   = sum_c' B[i][c'] u_c'(x_m)
    r[m][ch] = a0_m u_ch + sum_i a1_{m,i} d_i u_ch + aL_m lap u_ch + adv_m sum_i w_i(m) d_i u_ch - target[m][ch]

(pair_math.h ORDG, pigs_residual_terms_*; the reference's time-blended losses model_pn.py:794-805 and
test_no_mlp.py:122-144, and its Burgers term) -- against the float64 oracle's outputs composed the same way, against
the composition of the sampler's own outputs, dense and binned, both hosts, and inside a training loop."""
import functools

import numpy as np
import pytest
import torch

from conftest import grads_within_accumulation_bound
from oracle import c_oracle, dense_torch
from pigs_amd import synthetic
from test_binned_gpu import random_gaussians, dev32

pytestmark = pytest.mark.gpu
HOSTS = ["native", "ctypes"]
# advect_by per (d, c): never the identity
BY = {(1, 1): ((0.7,),), (2, 1): ((0.8,), (-0.5,)), (2, 2): ((0.9, 0.3), (-0.2, 1.1)),
      (2, 3): ((0.9, 0.3, -0.4), (-0.2, 1.1, 0.5))}


def np64(x):
    return x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def rel(a, b):
    a, b = np64(a), np64(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def fields(rng, M, d, advect=True):
    """a0, a1, aL, adv as float64 arrays [M], [M, d], [M], [M] (adv = None without advection)"""
    return (rng.uniform(0.5, 2.0, M), rng.uniform(-0.2, 0.2, (M, d)), rng.uniform(-0.004, -0.001, M),
            rng.uniform(0.2, 1.0, M) if advect else None)


def compose(exp, F, B, target, d):
    """r from the oracle's outputs of orders 0, 1, 2 (float64)"""
    a0, a1, aL, adv = F
    u, du = exp[0], exp[1]
    lap = sum(exp[2][:, i, i] for i in range(d))
    r = a0[:, None] * u + aL[:, None] * lap - (0 if target is None else target)
    for i in range(d):
        coef = a1[:, i] + (0 if adv is None else adv * (u @ np.asarray(B)[i]))
        r = r + coef[:, None] * du[:, i]
    return r


def incoming(w, exp, F, B, d, c):
    """The gradients that arrive at orders 0, 1, 2 when w [M, c] arrives at r (the issue's backward formulas)."""
    a0, a1, aL, adv = F
    u, du = exp[0], exp[1]
    M = w.shape[0]
    g0 = a0[:, None] * w
    g1 = np.zeros((M, d, c))
    g2 = np.zeros((M, d, d, c))
    for i in range(d):
        coef = a1[:, i]
        if adv is not None:
            coef = coef + adv * (u @ np.asarray(B)[i])
            g0 = g0 + (adv * (w * du[:, i]).sum(-1))[:, None] * np.asarray(B)[i][None, :]
        g1[:, i] = coef[:, None] * w
        g2[:, i, i] = aL[:, None] * w
    return {0: g0, 1: g1, 2: g2}


def term_scale(exp, F, target, d):
    a0, a1, aL, adv = F
    lap = sum(exp[2][:, i, i] for i in range(d))
    terms = [np.abs(a0).max() * np.abs(exp[0]).max(), np.abs(aL).max() * np.abs(lap).max()]
    if target is not None:
        terms.append(np.abs(target).max())
    if adv is not None:
        terms.append(np.abs(adv).max() * np.abs(exp[0]).max() * np.abs(exp[1]).max())
    return max(terms)


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def composed_by_torch(s, F, B, target, d):
    """The same residual from the sampler's OWN u, grad u and trace (three outputs of one launch + torch)."""
    a0, a1, aL, adv = F
    u, du, lap = s.sample((0, 1, "lap"))
    r = a0[:, None] * u + aL[:, None] * lap - (0 if target is None else target)
    Bt = torch.as_tensor(B, dtype=u.dtype, device=u.device)
    for i in range(d):
        coef = a1[:, i] + (0 if adv is None else adv * (u @ Bt[i]))
        r = r + coef[:, None] * du[:, i]
    return r, (u, du, lap)


def call(s, F, B, target):
    a0, a1, aL, adv = F
    return s.residual(a0=a0, a1=a1, lap=aL, target=target, advect=adv, advect_by=None if adv is None else B)


# the bars against the composition of the sampler's own outputs (tests/test_residual_gpu.py,
# test_residual_equals_composed_outputs_at_c3_size): forward 2e-6 of the term scale, gradients 5e-6 of the largest entry.
# Measured worst over every case of this file that uses them (dense f32 c = 1, 3 at three sizes; binned lattice /
# random / per-point-walk / record-range tiles, c = 1, 2; periodic): forward 1.3e-7, gradients 5.5e-7 -- the bars stand.
FWD_OWN, GRAD_OWN = 2e-6, 5e-6


def check_against_own_composition(s, leaves, F, B, target, d, w):
    """Forward and gradients of residual(...) against torch.autograd through the same expression on the same plan."""
    r = call(s, F, B, target)
    g_r = torch.autograd.grad((r * w).sum(), leaves)
    comp, (u, du, lap) = composed_by_torch(s, F, B, target, d)
    g_c = torch.autograd.grad((comp * w).sum(), leaves)
    a0, a1, aL, adv = F
    scale = max(float(a0.abs().max() * u.detach().abs().max()), float(aL.abs().max() * lap.detach().abs().max()),
                0.0 if adv is None else float(adv.abs().max() * u.detach().abs().max() * du.detach().abs().max()))
    fwd = float((r - comp).detach().abs().max()) / scale
    grads = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_r, g_c)]
    print(f"own composition: forward {fwd:.3g} of the term scale, gradients {max(grads):.3g} of the largest entry")
    assert fwd < FWD_OWN, fwd
    assert max(grads) < GRAD_OWN, grads


# ------------------------------------------------------------------------------------------
# 1. dense against the oracle
# ------------------------------------------------------------------------------------------
def dense_problem(d, c, N, M, seed):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1, 1, (N, d))
    if d == 2:
        s0 = np.exp(2 * rng.normal(-3.0, 0.4, (N, 2)))
        tau = np.tanh(rng.normal(0, 0.6, N)) * np.sqrt(s0[:, 0] * s0[:, 1])
        det = s0[:, 0] * s0[:, 1] - tau ** 2
        con = np.stack((s0[:, 1] / det, -tau / det, s0[:, 0] / det), -1)
    else:
        con = 1.0 / np.exp(2 * rng.normal(-3.0, 0.4, (N, 1)))
    return rng, means, rng.uniform(-1, 1, (N, c)), con, rng.uniform(-1, 1, (M, d)), rng.uniform(-1, 1, (M, c))


def run_dense_case(host, dtype, d, c, N, M):
    from diff_gaussian_sampling import GaussianSampler
    rng, means, values, con, pts, target = dense_problem(d, c, N, M, 11 * d + c)
    F64 = fields(rng, M, d)
    B = BY[(d, c)]
    t = [dev(a, dtype) for a in (means, values, con, pts, target)]
    for x in t[:3] + [t[4]]:
        x.requires_grad_(True)
    F = tuple(dev(a, dtype) for a in F64)
    F64 = tuple(np64(a) for a in F)                      # what the kernel saw (float32 rounding included)
    s = GaussianSampler(True, backend="dense", host=host)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert s._plan is None
    r = call(s, F, B, t[4])
    assert tuple(r.shape) == (M, c) and r.dtype == dtype
    args = [np64(x) for x in (t[0], t[2], t[1], t[3])]
    tg = np64(t[4])
    exp = c_oracle.forward(*args, orders=(0, 1, 2))
    want = compose(exp, F64, B, tg, d)
    scale = term_scale(exp, F64, tg, d)
    err = np.abs(np64(r) - want).max() / scale
    print(f"forward: {err:.3g} of the term scale {scale:.3g}")
    w = rng.uniform(-1, 1, (M, c))
    wt = dev(w, dtype)
    if dtype == torch.float64:
        assert err < 1e-11
        (r * wt).sum().backward()
        gm, gc, gv = c_oracle.backward(*args, incoming(np64(wt), exp, F64, B, d, c))
        errs = (rel(t[0].grad, gm), rel(t[2].grad, gc), rel(t[1].grad, gv))
        print("gradients:", errs)
        assert max(errs) < 1e-11, errs
        assert torch.equal(t[4].grad, -wt)
    else:
        assert err < 1e-5
        # the kernel forms the incoming gradients from its own float32 u and grad u: against torch.autograd through
        # the same expression on the sampler's own outputs
        check_against_own_composition(s, t[:3], F, B, t[4].detach(), d, wt)
        (call(s, F, B, t[4]) * wt).sum().backward()
        assert torch.equal(t[4].grad, -wt)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,d,c", [(torch.float64, 2, 2), (torch.float64, 1, 1), (torch.float32, 2, 1), (torch.float32, 2, 3)])
def test_dense_matches_composed_oracle(hip_lib, host, dtype, d, c):
    """N = 403, M = 3001: a ragged tail of Gaussians, the last wave partly filled; all four fields, a non-identity
    advect_by and a target."""
    run_dense_case(host, dtype, d, c, 403, 3001)


@pytest.mark.parametrize("dtype,d,c,N,M", [(torch.float32, 2, 1, 70, 16501), (torch.float32, 2, 3, 70, 16501),
                                           (torch.float64, 2, 2, 40, 16500)])
def test_dense_kernels_of_the_other_sizes(hip_lib, dtype, d, c, N, M):
    """More than 16 384 points: the wave-split forward (16 waves for one channel, 4 for three) and the backward whose
    per-point values are wave-uniform loads, two points per iteration (M odd and even); float64 takes the four-wave
    forward."""
    run_dense_case("ctypes", dtype, d, c, N, M)


# ------------------------------------------------------------------------------------------
# 2. binned, through every store and load site
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def binned_problem_c2(name):
    """(means, conics, values, points) in float64 with two channels, the oracle's outputs and the stats key that must
    be > 0 (or None).  The channels of u, grad u and the trace are independent: the one-channel problem is channel 0."""
    rng = np.random.default_rng(14)
    if name in ("lattice", "random"):
        gs = synthetic.lattice_gaussians(24, 24, 0.8, seed=3, c=2)
        m, con, v = (gs[k].float().double().numpy() for k in ("means", "conics", "values"))
        pts = synthetic.grid_samples(72).float().double().numpy() if name == "lattice" else rng.uniform(-1, 1, (3001, 2))
        key = None
    elif name == "points":       # thin outskirts: every point of a tile walks the grid itself
        m, con, v = random_gaussians(rng, 12000, 2, log_sigma_mean=-4.4, log_sigma_std=0.25)
        pts, key = np.clip(rng.normal(0, 0.15, (60000, 2)), -1, 1), "points_tiles"
    else:                        # very wide Gaussians: record ranges
        m, con, v = random_gaussians(rng, 1500, 2, log_sigma_mean=-1.2, log_sigma_std=0.3, lo=-0.5, hi=0.5)
        pts, key = rng.uniform(-0.5, 0.5, (3000, 2)), "ranges_tiles"
    args = [np64(dev32(a)) for a in (m, con, v, pts)]
    exp = c_oracle.forward(*args, orders=(0, 1, 2))
    return args, exp, key


def binned_problem(name, c):
    args, exp, key = binned_problem_c2(name)
    if c == 2:
        return args, exp, key
    return [args[0], args[1], args[2][:, :1].copy(), args[3]], {k: np.ascontiguousarray(exp[k][..., :1]) for k in (0, 1, 2)}, key


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("name", ["lattice", "random", "points", "ranges"])
def test_binned_through_every_store_and_load_site(hip_lib, name, c):
    """Index-tiled lattice points (streamed stores), sorted random points (plain stores), tiles whose points walk the
    grid themselves, tiles in record ranges: forward against the oracle; gradients against the accumulation bound
    where they are exact functions of the inputs (no advection), and against torch.autograd through the composition of
    the sampler's own outputs with advection."""
    from diff_gaussian_sampling import GaussianSampler
    from tools.prof_step import list_stats
    args, exp, key = binned_problem(name, c)
    M = args[3].shape[0]
    rng = np.random.default_rng(5)
    B = BY[(2, c)]
    t = [dev32(a) for a in (args[0], args[2], args[1], args[3])]
    for x in t[:3]:
        x.requires_grad_(True)
    target = dev32(rng.uniform(-1, 1, (M, c)))
    F = tuple(dev32(a) for a in fields(rng, M, 2))
    F64 = tuple(np64(a) for a in F)
    s = GaussianSampler(True, backend="binned")
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert s._plan is not None
    if key is not None:
        assert list_stats(s._plan)[key] > 0, name
    r = call(s, F, B, target)
    want = compose(exp, F64, B, np64(target), 2)
    scale = term_scale(exp, F64, np64(target), 2)
    err = np.abs(np64(r) - want).max() / scale
    print(f"forward: {err:.3g} of the term scale {scale:.3g}")
    assert err < 1e-5
    w = dev32(rng.uniform(-1, 1, (M, c)))
    check_against_own_composition(s, t[:3], F, B, target, 2, w)
    # fields without advection: the incoming gradients are exact functions of the inputs
    Fn = F[:3] + (None,)
    rn = call(s, Fn, B, target)
    assert np.abs(np64(rn) - compose(exp, F64[:3] + (None,), B, np64(target), 2)).max() / scale < 1e-5
    g = torch.autograd.grad((rn * w).sum(), t[:3])
    # (a Gaussian's gradient depends on no other Gaussian: at 12 000 x 60 000 the oracle's bound is evaluated for every
    # third one -- its floor, a fraction of the largest entry among them, is then no larger than the full set's)
    sel = slice(None, None, 3 if name == "points" else 1)
    bad = grads_within_accumulation_bound((g[0][sel], g[2][sel], g[1][sel]), [a[sel] for a in args[:3]] + [args[3]],
                                          incoming(np64(w), exp, F64[:3] + (None,), B, 2, c))
    assert not bad, bad


# ------------------------------------------------------------------------------------------
# 3. the Burgers blend
# ------------------------------------------------------------------------------------------
def burgers_terms(tau, pu, pux0, plap, dt, nu):
    """The reference's blended Burgers residual (u - pu) / dt - nu (tau plap + (1 - tau) lap u) + (tau pu + (1 - tau) u)
    (tau pux0 + (1 - tau) u_x) as residual() arguments (c = 1, d = 2; advect_by = [[1], [0]]).  All [M]."""
    zero = torch.zeros_like(tau)
    return dict(a0=1 / dt + tau * (1 - tau) * pux0, a1=torch.stack((tau * (1 - tau) * pu, zero), -1), lap=-nu * (1 - tau),
                advect=(1 - tau) ** 2, advect_by=((1.0,), (0.0,)),
                target=(pu / dt + nu * tau * plap - tau ** 2 * pu * pux0)[:, None])


def burgers_by_hand(u, ux0, lap, tau, pu, pux0, plap, dt, nu):
    return (u - pu) / dt - nu * (tau * plap + (1 - tau) * lap) + (tau * pu + (1 - tau) * u) * (tau * pux0 + (1 - tau) * ux0)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_burgers_blend_through_residual(hip_lib, host, backend):
    """Loss and gradients through residual(...) against the loss written with the three sample_*() calls (the bars of
    test_diffusion_loss_through_residual: loss 1e-5, gradients 2e-5 of the largest entry; measured: the same float32
    loss, gradients within 2.1e-7)."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(20, 20, 1.1, seed=5)
    t = {k: v.float().cuda() for k, v in gs.items()}
    for k in ("means", "values", "conics"):
        t[k].requires_grad_(True)
    gen = torch.Generator().manual_seed(1)
    pts = (torch.rand((1024, 2), generator=gen) * 2 - 1).cuda()
    tau = torch.rand((1024,), generator=gen).cuda()
    dt, nu = 0.01, 0.05
    with torch.no_grad():                      # the frozen previous level: other Gaussians, a sampler of its own
        pg = synthetic.lattice_gaussians(20, 20, 1.1, seed=6)
        s2 = GaussianSampler(False, backend=backend, host=host)
        s2.preprocess(pg["means"].float().cuda(), pg["values"].float().cuda(), None, pg["conics"].float().cuda(), pts)
        pu, pdu, plap = s2.sample((0, 1, "lap"))
        pu, pux0, plap = pu[:, 0], pdu[:, 0, 0], plap[:, 0]
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(t["means"], t["values"], t["covariances"], t["conics"], pts)
    assert (s._plan is not None) == (backend == "binned")
    u, du, uxx = s.sample_gaussians(), s.sample_gaussians_derivative(), s.sample_gaussians_laplacian()
    res = burgers_by_hand(u[:, 0], du[:, 0, 0], uxx[:, 0, 0, 0] + uxx[:, 1, 1, 0], tau, pu, pux0, plap, dt, nu)
    loss_ref = res.pow(2).mean()
    leaves = (t["means"], t["values"], t["conics"])
    g_ref = torch.autograd.grad(loss_ref, leaves)
    r = s.residual(**burgers_terms(tau, pu, pux0, plap, dt, nu))
    assert float((r[:, 0] - res).detach().abs().max()) < 1e-5 * float(res.detach().abs().max())
    loss = r.pow(2).mean()
    g = torch.autograd.grad(loss, leaves)
    errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g, g_ref)]
    loss, loss_ref = float(loss.detach()), float(loss_ref.detach())
    print(f"loss {abs(loss - loss_ref) / loss_ref:.3g}, gradients {errs}")
    assert abs(loss - loss_ref) / loss_ref < 1e-5
    assert max(errs) < 2e-5, errs


# ------------------------------------------------------------------------------------------
# 4. equivalence with the linear residual
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_constant_fields_equal_the_float_coefficients(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(20, 20, 1.1, seed=8)
    t = {k: v.float().cuda() for k, v in gs.items()}
    leaves = [t[k].requires_grad_(True) for k in ("means", "values", "conics")]
    gen = torch.Generator().manual_seed(3)
    M = 1500
    pts = (torch.rand((M, 2), generator=gen) * 2 - 1).cuda()
    target = torch.rand((M, 1), generator=gen).cuda()
    w = (torch.rand((M, 1), generator=gen) * 2 - 1).cuda()
    a0, a1, aL = 1.7, (0.3, -0.1), -0.01
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(leaves[0], leaves[1], None, leaves[2], pts)
    r_lin = s.residual(a0=a0, a1=a1, lap=aL, target=target)
    g_lin = torch.autograd.grad((r_lin * w).sum(), leaves)
    r_gen = s.residual(a0=torch.full((M,), a0).cuda(), a1=torch.tensor(a1).expand(M, 2).cuda(),
                       lap=torch.full((M, 1), aL).cuda(), target=target)
    g_gen = torch.autograd.grad((r_gen * w).sum(), leaves)
    u, lap = s.sample((0, "lap"))
    scale = max(a0 * float(u.abs().max()), abs(aL) * float(lap.abs().max()))
    assert float((r_gen - r_lin).detach().abs().max()) / scale < 2e-6
    for a, b in zip(g_gen, g_lin):
        assert float((a - b).abs().max() / b.abs().max()) < 5e-6


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_floats_alone_stay_on_the_linear_kernel(hip_lib, backend):
    """residual() with float coefficients and no advection is the linear residual's own launch, bit for bit:
    pigs_residual_forward through the C ABI on the same inputs (and plan)."""
    import ctypes
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd import host_ctypes as S
    gs = synthetic.lattice_gaussians(20, 20, 1.1, seed=8)
    m, v, con = (gs[k].float().cuda().contiguous() for k in ("means", "values", "conics"))
    pts = (torch.rand((1500, 2), generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    s = GaussianSampler(False, backend=backend, host="ctypes")
    with torch.no_grad():
        s.preprocess(m, v, None, con, pts)
        r = s.residual(a0=1.7, a1=(0.3, -0.1), lap=-0.01)
        raw = S._fused_call(S._ResidualFunction.op, False, m, v, con, pts, S.ResidualCoeffs((1.7, 0.3, -0.1, -0.01)), s._plan)
    assert (s._plan is not None) == (backend == "binned")
    assert torch.equal(r, raw)
    assert r.grad_fn is None
    m.requires_grad_(True)
    s.preprocess(m, v, None, con, pts)
    assert type(s.residual(a0=1.7, lap=-0.01).grad_fn).__name__ == "_ResidualFunctionBackward"
    assert type(s.residual(a0=torch.full((1500,), 1.7).cuda(), lap=-0.01).grad_fn).__name__ == "_ResidualTermsFunctionBackward"


# ------------------------------------------------------------------------------------------
# 5. host behaviour
# ------------------------------------------------------------------------------------------
def small_problem(c=1, M=700, seed=4, grad=True):
    gs = synthetic.lattice_gaussians(12, 12, 1.0, seed=seed, c=c)
    t = [gs[k].float().cuda() for k in ("means", "values", "conics")]
    if grad:
        for x in t:
            x.requires_grad_(True)
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand((M, 2), generator=gen) * 2 - 1).cuda()
    return t, pts, torch.rand((M,), generator=gen).cuda()


@pytest.mark.parametrize("host", HOSTS)
def test_arguments_are_checked(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau = small_problem()
    M = pts.shape[0]
    s = GaussianSampler(False, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    with pytest.raises(ValueError, match="constants"):
        s.residual(a0=tau.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="advect_by"):      # c = 1, d = 2: no default
        s.residual(a0=1.0, advect=0.5)
    with pytest.raises(ValueError, match="advect_by"):
        s.residual(a0=1.0, advect=0.5, advect_by=((1.0, 0.0), (0.0, 1.0)))
    for bad in (dict(a0=tau[:-1]), dict(a1=tau), dict(a1=torch.zeros((M, 3)).cuda()), dict(lap=torch.zeros((M, 2)).cuda()),
                dict(advect=torch.zeros((2, M)).cuda(), advect_by=((1.0,), (0.0,))), dict(a1=(0.1, 0.2, 0.3), a0=tau)):
        with pytest.raises(ValueError):
            s.residual(**bad)
    with pytest.raises(RuntimeError, match="device"):
        s.residual(a0=tau.cpu())
    # [M, 1] is [M]; an integer field is cast
    a = s.residual(a0=tau, lap=-0.01)
    b = s.residual(a0=tau[:, None], lap=-0.01)
    assert torch.equal(a, b)
    ones = s.residual(a0=torch.ones((M,), dtype=torch.int64).cuda())
    assert torch.equal(ones, s.residual(a0=torch.ones((M,)).cuda()))
    # c == d: the default advect_by is the identity
    t2, pts2, tau2 = small_problem(c=2)
    s.preprocess(t2[0], t2[1], None, t2[2], pts2)
    assert torch.equal(s.residual(a0=tau2, advect=0.5), s.residual(a0=tau2, advect=0.5, advect_by=((1.0, 0.0), (0.0, 1.0))))


@pytest.mark.parametrize("host", HOSTS)
def test_no_aux_without_a_backward(hip_lib, host):
    """Under no_grad (and with no input that requires grad) the forward allocates no aux -- M (1 + d) c values -- and
    equals the grad-mode forward."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau = small_problem(M=40000)
    M = pts.shape[0]
    kw = dict(a0=tau, lap=-0.01, advect=1 - tau, advect_by=((1.0,), (0.5,)))
    s = GaussianSampler(False, backend="dense", host=host)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    s.preprocess(t[0], t[1], None, t[2], pts)
    r_grad, with_aux = peak(lambda: s.residual(**kw))
    assert r_grad.grad_fn is not None
    with torch.no_grad():
        r_no, without = peak(lambda: s.residual(**kw))
    assert r_no.grad_fn is None
    assert torch.equal(r_no, r_grad.detach())
    assert with_aux - without >= 3 * 4 * M and without < 3 * 4 * M, (with_aux, without)
    s.preprocess(t[0].detach(), t[1].detach(), None, t[2].detach(), pts)       # grad mode on, nothing requires grad
    r_leafless, leafless = peak(lambda: s.residual(**kw))
    assert r_leafless.grad_fn is None and leafless < 3 * 4 * M
    assert torch.equal(r_leafless, r_no)


@pytest.mark.parametrize("host", HOSTS)
def test_differentiable_call_rebuilds_a_forward_only_plan(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau = small_problem(M=3000)
    kw = dict(a0=tau, lap=-0.01, advect=1 - tau, advect_by=((1.0,), (0.5,)))
    w = torch.rand((3000, 1), generator=torch.Generator().manual_seed(0)).cuda()
    full = GaussianSampler(True, backend="binned", host=host)
    full.preprocess(t[0], t[1], None, t[2], pts)
    assert not full._plan.forward_only
    g_full = torch.autograd.grad((full.residual(**kw) * w).sum(), t)
    lazy = GaussianSampler(True, backend="binned", host=host)
    with torch.no_grad():
        lazy.preprocess(t[0], t[1], None, t[2], pts)
        before = lazy._plan
        assert before.forward_only
        r0 = lazy.residual(**kw)                      # served by the forward-only plan
    assert lazy._plan is before
    r = lazy.residual(**kw)
    assert lazy._plan is not before and not lazy._plan.forward_only
    assert float((r.detach() - r0).abs().max()) <= 1e-6 * float(r0.abs().max())
    g_lazy = torch.autograd.grad((r * w).sum(), t[0])
    assert torch.isfinite(g_lazy[0]).all()
    assert float((g_lazy[0] - g_full[0]).abs().max()) <= 1e-5 * float(g_full[0].abs().max())


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("c", [1, 2])
def test_first_call_on_deferred_lists(hip_lib, host, c):
    """defer_lists=True: the general residual as the plan's first sampling call (the lists in a launch of their own)
    equals the call on a plan with its lists built, and every later call finds them."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau = small_problem(c=c, M=3000)
    kw = dict(a0=tau, lap=-0.01, advect=1 - tau, advect_by=BY[(2, c)])
    w = torch.rand((3000, c), generator=torch.Generator().manual_seed(0)).cuda()
    out = {}
    for defer in (False, True):
        s = GaussianSampler(False, backend="binned", host=host, defer_lists=defer)
        s.preprocess(t[0], t[1], None, t[2], pts)
        r = s.residual(**kw)
        out[defer] = (r.detach(), torch.autograd.grad((r * w).sum(), t), s.sample_gaussians().detach())
    assert float((out[True][0] - out[False][0]).abs().max()) <= 2e-6 * float(out[False][0].abs().max())
    assert float((out[True][2] - out[False][2]).abs().max()) <= 2e-6 * float(out[False][2].abs().max())
    for a, b in zip(out[True][1], out[False][1]):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_graphed_step_sees_the_field_change(hip_lib, host, backend):
    """One step (preprocess, residual, backward) captured and replayed after an in-place change of the tau field:
    no host synchronisation in the path, and the fields are read at replay time."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    t, pts, tau0 = small_problem(M=2000, grad=False)
    sampler = GaussianSampler(False, backend=backend, host=host)

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in t) + (tau0.clone(),)

    def fn(means, values, conics, tau):
        sampler.preprocess(means, values, None, conics, pts)
        r = sampler.residual(a0=10 + tau * (1 - tau), a1=torch.stack((tau, 0 * tau), -1), lap=-0.05 * (1 - tau),
                             advect=(1 - tau) ** 2, advect_by=((1.0,), (0.0,)), target=tau[:, None])
        loss = r.pow(2).mean()
        return (loss,) + torch.autograd.grad(loss, (means, values, conics))

    step = GraphedStep(fn, make_inputs)
    gen = torch.Generator().manual_seed(9)
    for trial in range(2):
        with torch.no_grad():
            step.inputs[3].copy_(torch.rand(tau0.shape, generator=gen).cuda())
        got = step()
        torch.cuda.synchronize()
        m, v, c = (x.detach().clone().requires_grad_(True) for x in step.inputs[:3])
        eager = fn(m, v, c, step.inputs[3].clone())
        for a, b in zip(got, eager):
            assert float((a.detach() - b.detach()).abs().max()) <= 2e-6 * float(b.detach().abs().max()) + 1e-30, trial


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_periodic_sampler(hip_lib, host, backend):
    """An 8 x 8 lattice in [-1, 1)^2 on the torus: the bound images are the Gaussians, so the general residual equals
    the composition of the periodic sampler's own outputs."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(8, 8, 0.3, seed=2, c=2)      # (narrow enough for the torus: extent below the period)
    means = gs["means"].float().cuda().requires_grad_(True)
    values, conics = gs["values"].float().cuda().requires_grad_(True), gs["conics"].float().cuda().requires_grad_(True)
    rng = np.random.default_rng(2)
    M = 2500
    pts = dev32(rng.uniform(-1, 1, (M, 2)))
    F = tuple(dev32(a) for a in fields(rng, M, 2))
    s = GaussianSampler(False, backend=backend, host=host, periodic=(-1.0, 1.0))
    s.preprocess(means, values, None, conics, pts)
    assert (s._plan is not None) == (backend == "binned")
    check_against_own_composition(s, (means, values, conics), F, BY[(2, 2)], dev32(rng.uniform(-1, 1, (M, 2))), 2,
                                  dev32(rng.uniform(-1, 1, (M, 2))))


# ------------------------------------------------------------------------------------------
# 6. training-loop parity
# ------------------------------------------------------------------------------------------
class OracleSampler:
    """The sampler's surface through oracle/dense_torch.py on the CPU (tests/test_training_gpu.py)."""
    backend = "oracle"

    def preprocess(self, means, values, covariances, conics, samples):
        self.args = (means, conics, values, samples)

    def sample(self, orders):
        o = dense_torch.forward(*self.args, orders=(0, 1, 2), chunk=1024)
        return o[0], o[1], o[2][:, 0, 0] + o[2][:, 1, 1]


# 30 steps, as tests/test_training_gpu.py: measured against the CPU oracle loop, the one-launch loop deviates 1.7e-6
# (dense) / 2.2e-6 (binned) and the same GPU loop composed from sample((0, 1, "lap")) 1.4e-6 / 1.3e-6 -- the composed loop
# meets 2e-3 with far more than a factor 2 to spare, so the run is not shortened
LOOP_STEPS = 30


def burgers_loop(sampler, device, mode, steps=LOOP_STEPS, n=16, scale=2.5, dt=0.1, nu=0.1):
    """The loop of tests/test_training_gpu.py::run_loop with the blended Burgers residual as the loss from step 10 on.
    mode "residual": the one-launch residual(); "composed": the same loss from sample((0, 1, "lap")) in torch."""
    g = torch.Generator(device="cpu").manual_seed(7)
    tx = torch.linspace(-1, 1, n) * 0.6
    gx, gy = torch.meshgrid((tx, tx), indexing="ij")
    raw_means = torch.atanh(torch.stack((gx, gy), dim=-1).reshape(n * n, 2)).to(device).requires_grad_(True)
    raw_scaling = torch.full((n * n, 2), -3.0, device=device, requires_grad=True)
    transform = torch.zeros((n * n, 1), device=device, requires_grad=True)
    values = (0.1 * torch.rand((n * n, 1), generator=g)).to(device).requires_grad_(True)
    optim = torch.optim.Adam([raw_means, values, raw_scaling, transform], lr=1e-2)

    def gaussians():
        means = torch.tanh(raw_means) * scale
        cov, con = synthetic.covariances_from_raw(torch.exp(raw_scaling), transform)
        return means, cov, con

    losses, prev = [], None
    for it in range(steps):
        samples = ((torch.rand((1024, 2), generator=g) * 2 - 1) * scale).to(device)
        tau = torch.rand((1024,), generator=g).to(device)
        if it == 10:                      # freeze the fitted state as the previous time level
            with torch.no_grad():
                means, cov, con = gaussians()
                prev = (means.clone(), values.detach().clone(), cov.clone(), con.clone())
        means, cov, con = gaussians()
        sampler.preprocess(means, values, cov, con, samples)
        if it < 10:
            u = sampler.sample((0,))[0] if mode != "oracle" else sampler.sample((0, 1, "lap"))[0]
            desired = torch.exp(-0.5 * (samples ** 2).sum(-1) / (0.1 * scale))
            loss = torch.mean((u[:, 0] - desired) ** 2)
        else:
            with torch.no_grad():
                sampler2 = OracleSampler() if mode == "oracle" else sampler.__class__(False, backend=sampler.backend)
                sampler2.preprocess(*prev, samples)
                pu, pdu, plap = sampler2.sample((0, 1, "lap"))
                pu, pux0, plap = pu[:, 0], pdu[:, 0, 0], plap[:, 0]
            if mode == "residual":
                r = sampler.residual(**burgers_terms(tau, pu, pux0, plap, dt, nu))[:, 0]
            else:
                u, du, lap = sampler.sample((0, 1, "lap"))
                r = burgers_by_hand(u[:, 0], du[:, 0, 0], lap[:, 0], tau, pu, pux0, plap, dt, nu)
            loss = torch.mean(r ** 2)
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


@functools.lru_cache(maxsize=None)
def oracle_curve():
    torch.set_num_threads(8)
    return burgers_loop(OracleSampler(), torch.device("cpu"), "oracle")


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_burgers_training_loop_matches_the_oracle_loop(hip_lib, backend):
    from diff_gaussian_sampling import GaussianSampler
    cpu = oracle_curve()
    s = GaussianSampler(False, backend=backend)
    gpu = burgers_loop(s, torch.device("cuda"), "residual")
    assert (s._plan is not None) == (backend == "binned")
    assert np.isfinite(gpu).all() and gpu[9] < gpu[0] and gpu[-1] < gpu[10]
    dev_r = np.abs(gpu - cpu) / np.maximum(np.abs(cpu), 1e-12)
    print(f"{backend}: residual() loop deviates {dev_r.max():.3g} from the oracle loop over {LOOP_STEPS} steps")
    assert dev_r.max() < 2e-3, (dev_r.max(), gpu, cpu)
