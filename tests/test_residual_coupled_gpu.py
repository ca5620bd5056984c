"""GPU: GaussianSampler.residual() with coupled channels -- two constant c x c matrices mix the channels under a
per-point weight,

    r[m][ch] = a0_m u_ch + aL_m lap u_ch + cw_m sum_c' (couple0[ch][c'] u_c' + couple_lap[ch][c'] lap u_c') - target[m][ch]

(pair_math.h ORDC, pigs_residual_coupled_*; the reference's wave system, test_no_mlp.py:127-139) -- against the float64
oracle's outputs composed the same way, against the composition of the sampler's own outputs, dense and binned, both
hosts, under graph capture and inside a training loop."""
import functools

import numpy as np
import pytest
import torch

from conftest import grads_within_accumulation_bound
from oracle import c_oracle
from pigs_amd import synthetic
from test_binned_gpu import dev32
from test_residual_terms_gpu import (FWD_OWN, GRAD_OWN, OracleSampler, binned_problem_c2, dense_problem, dev, np64, rel,
                                     small_problem)

pytestmark = pytest.mark.gpu
HOSTS = ["native", "ctypes"]


def coefficients(rng, M, c):
    """a0, aL, cw as float64 arrays [M] and the two matrices [c, c] (rounded to float32: every launch type sees the
    same numbers), every off-diagonal entry at least a fifth of the range away from zero and every pair (i, j), (j, i)
    at least two fifths apart: neither matrix is close to symmetric."""
    Q0, QL = rng.uniform(-1, 1, (c, c)), rng.uniform(-0.004, 0.004, (c, c))
    off = ~np.eye(c, dtype=bool)
    for q, least in ((Q0, 0.2), (QL, 0.0008)):
        q[off] = np.where(q[off] < 0, -1.0, 1.0) * np.maximum(np.abs(q[off]), least)
        for i in range(c):
            for j in range(i):
                if abs(q[i, j] - q[j, i]) < 2 * least:
                    q[i, j] = -q[i, j]
    Q0, QL = (np.float32(q).astype(np.float64) for q in (Q0, QL))
    return rng.uniform(0.5, 2.0, M), rng.uniform(-0.004, -0.001, M), rng.uniform(0.2, 1.0, M), Q0, QL


def laplacian(exp, d):
    return sum(exp[2][:, i, i] for i in range(d))


def compose(exp, K, target, d):
    """r from the oracle's outputs of orders 0, 1, 2 (float64): r = ... + cw (u @ couple0.T + lap @ couple_lap.T)"""
    a0, aL, cw, Q0, QL = K
    u, lap = exp[0], laplacian(exp, d)
    return a0[:, None] * u + aL[:, None] * lap + cw[:, None] * (u @ Q0.T + lap @ QL.T) - (0 if target is None else target)


def incoming(w, K, d, c):
    """The gradients that arrive at orders 0 and 2 when w [M, c] arrives at r (the backward formulas of pair_math.h):
    g0[c'] = a0 w_c' + cw sum_ch couple0[ch][c'] w_ch, and the same with aL / couple_lap on the Hessian's diagonal."""
    a0, aL, cw, Q0, QL = K
    M = w.shape[0]
    g2 = np.zeros((M, d, d, c))
    for i in range(d):
        g2[:, i, i] = aL[:, None] * w + cw[:, None] * (w @ QL)
    return {0: a0[:, None] * w + cw[:, None] * (w @ Q0), 1: np.zeros((M, d, c)), 2: g2}


def term_scale(exp, K, target, d):
    a0, aL, cw, Q0, QL = K
    u, lap = np.abs(exp[0]).max(), np.abs(laplacian(exp, d)).max()
    terms = [np.abs(a0).max() * u, np.abs(aL).max() * lap, np.abs(cw).max() * np.abs(Q0).max() * u,
             np.abs(cw).max() * np.abs(QL).max() * lap]
    if target is not None:
        terms.append(np.abs(target).max())
    return max(terms)


def expectation(exp, K, target, d, each=True):
    """(want, scale) -- and the condition on the inputs that makes the comparison worth something: with the matrices
    transposed (a transposition or channel-swap bug) the composition is somewhere else by more than 1e-2 of the scale.
    ``each``: also with either matrix transposed alone (the dense problems; where the Gaussians are so narrow that the
    Laplacian's terms are hundreds of times the field's, couple0 alone cannot move the result that far)."""
    a0, aL, cw, Q0, QL = K
    want, scale = compose(exp, K, target, d), term_scale(exp, K, target, d)
    others = ((a0, aL, cw, Q0.T, QL.T),) + (((a0, aL, cw, Q0.T, QL), (a0, aL, cw, Q0, QL.T)) if each else ())
    for other in others:
        assert np.abs(compose(exp, other, target, d) - want).max() > 1e-2 * scale
    return want, scale


def on_device(K, dtype=torch.float32):
    """the three fields as device tensors, the matrices as nested tuples of floats"""
    a0, aL, cw, Q0, QL = K
    return tuple(dev(a, dtype) for a in (a0, aL, cw)) + (tuple(map(tuple, Q0.tolist())), tuple(map(tuple, QL.tolist())))


def as_seen(Kd, K):
    """the float64 values of what the kernel reads (the fields after their rounding to the launch type)"""
    return tuple(np64(a) for a in Kd[:3]) + (K[3], K[4])


def call(s, Kd, target):
    a0, aL, cw, Q0, QL = Kd
    return s.residual(a0=a0, lap=aL, target=target, couple_weight=cw, couple0=Q0, couple_lap=QL)


def composed_by_torch(s, Kd, target):
    """The same residual from the sampler's OWN u and trace (two outputs of one launch + torch)."""
    a0, aL, cw, Q0, QL = Kd
    u, lap = s.sample((0, "lap"))
    Q0, QL = (torch.as_tensor(q, dtype=u.dtype, device=u.device) for q in (Q0, QL))
    r = a0[:, None] * u + aL[:, None] * lap + cw[:, None] * (u @ Q0.T + lap @ QL.T) - (0 if target is None else target)
    return r, (u, lap)


# The bars against the composition of the sampler's own outputs are FWD_OWN = 2e-6 of the term scale and GRAD_OWN = 5e-6
# of the largest entry (tests/test_residual_terms_gpu.py).  Measured worst over every case of this file that uses them
# (dense f32 c = 2, 3, 4 at every launch variant; binned lattice / random / per-point-walk / record-range tiles;
# periodic): forward 2.3e-7, gradients 6.3e-7; the wave recipe 4.5e-7 / 3.2e-7 -- the bars stand.
def check_against_own_composition(s, leaves, Kd, target, w):
    """Forward and gradients of residual(couple...) against torch.autograd through the same expression on the same plan."""
    r = call(s, Kd, target)
    g_r = torch.autograd.grad((r * w).sum(), leaves)
    comp, (u, lap) = composed_by_torch(s, Kd, target)
    g_c = torch.autograd.grad((comp * w).sum(), leaves)
    a0, aL, cw, Q0, QL = Kd
    um, lm = float(u.detach().abs().max()), float(lap.detach().abs().max())
    scale = max(float(a0.abs().max()) * um, float(aL.abs().max()) * lm, float(cw.abs().max()) * np.abs(Q0).max() * um,
                float(cw.abs().max()) * np.abs(QL).max() * lm, 0.0 if target is None else float(target.detach().abs().max()))
    fwd = float((r - comp).detach().abs().max()) / scale
    grads = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_r, g_c)]
    print(f"own composition: forward {fwd:.3g} of the term scale, gradients {max(grads):.3g} of the largest entry")
    assert fwd < FWD_OWN, fwd
    assert max(grads) < GRAD_OWN, grads


# ------------------------------------------------------------------------------------------
# 1. dense against the oracle
# ------------------------------------------------------------------------------------------
def run_dense_case(host, dtype, d, c, N, M):
    from diff_gaussian_sampling import GaussianSampler
    rng, means, values, con, pts, target = dense_problem(d, c, N, M, 11 * d + c)
    K = coefficients(rng, M, c)
    t = [dev(a, dtype) for a in (means, values, con, pts, target)]
    for x in t[:3] + [t[4]]:
        x.requires_grad_(True)
    Kd = on_device(K, dtype)
    K = as_seen(Kd, K)
    s = GaussianSampler(True, backend="dense", host=host)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert s._plan is None
    r = call(s, Kd, t[4])
    assert tuple(r.shape) == (M, c) and r.dtype == dtype
    args = [np64(x) for x in (t[0], t[2], t[1], t[3])]
    tg = np64(t[4])
    exp = c_oracle.forward(*args, orders=(0, 1, 2))
    want, scale = expectation(exp, K, tg, d)
    err = np.abs(np64(r) - want).max() / scale
    print(f"forward: {err:.3g} of the term scale {scale:.3g}")
    w = rng.uniform(-1, 1, (M, c))
    wt = dev(w, dtype)
    (r * wt).sum().backward()
    assert torch.equal(t[4].grad, -wt)
    if dtype == torch.float64:
        assert err < 1e-11
        gm, gc, gv = c_oracle.backward(*args, incoming(np64(wt), K, d, c))
        errs = (rel(t[0].grad, gm), rel(t[2].grad, gc), rel(t[1].grad, gv))
        print("gradients:", errs)
        assert max(errs) < 1e-11, errs
    else:
        assert err < 1e-5
        # nothing is non-linear in the field: the incoming gradients are exact functions of the inputs
        bad = grads_within_accumulation_bound((t[0].grad, t[2].grad, t[1].grad), args, incoming(np64(wt), K, d, c))
        assert not bad, bad
        for x in t[:3]:
            x.grad = None
        check_against_own_composition(s, t[:3], Kd, t[4].detach(), wt)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,d,c", [(torch.float64, 2, 2), (torch.float64, 1, 2), (torch.float32, 2, 2),
                                       (torch.float32, 2, 3), (torch.float32, 1, 4)])
def test_dense_matches_composed_oracle(hip_lib, host, dtype, d, c):
    """N = 403, M = 3001: a ragged tail of Gaussians and a partly filled last wave.  47 point blocks of 64 and more than
    128 Gaussians: the rows forward (16 points per workgroup); 2 x 47 < 512 workgroups: the staged backward with
    32-point slices.  Three fields, two non-symmetric matrices and a target."""
    run_dense_case(host, dtype, d, c, 403, 3001)


@pytest.mark.parametrize("c", [2, 3])
def test_dense_wave_split_forward_and_split_backward(hip_lib, c):
    """float32, N = 70, M = 16 501.  258 point blocks (> 256: not the rows forward, < 1 024) and 4 / 6 accumulators (the 16-wave
    workgroup's LDS and its 7-accumulator limit hold them): the 16-wave forward.  More than 16 384 points: the backward
    whose per-point values are wave-uniform loads, two points per iteration with an odd one left, the point range split
    65 ways and met by atomics."""
    run_dense_case("ctypes", torch.float32, 2, c, 70, 16501)


def test_dense_four_wave_forward_of_four_channels(hip_lib):
    """float32, c = 4, N = 70, M = 16 501: 8 accumulators exceed the 7 the 16-wave workgroup takes, so the same shape
    lands on the four-wave forward (and the split backward)."""
    run_dense_case("ctypes", torch.float32, 2, 4, 70, 16501)


def test_dense_float64_four_wave_forward(hip_lib):
    """float64, c = 2, N = 40, M = 16 500: 4 accumulators of two words each exceed the 16-wave limit and 40 Gaussians are
    too few for the rows forward (128): the four-wave forward; an even number of points in the split backward."""
    run_dense_case("ctypes", torch.float64, 2, 2, 40, 16500)


def test_dense_staged_backward_with_64_point_slices(hip_lib):
    """float32, c = 2, N = 403, M = 16 384: the largest M of the staged backward, and 2 x 256 = 512 workgroups are no longer
    fewer than 512, so the slices hold 64 points (256 point blocks: still the rows forward)."""
    run_dense_case("ctypes", torch.float32, 2, 2, 403, 16384)


# ------------------------------------------------------------------------------------------
# 2. + 3. binned, through every store and load site; against the own composition
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "random", "points", "ranges"])
def test_binned_through_every_store_and_load_site(hip_lib, name):
    """Index-tiled lattice points (streamed stores), sorted random points (plain stores), tiles whose points walk the
    grid themselves, tiles in record ranges: forward against the oracle, gradients against the accumulation bound (they
    are exact functions of the inputs), and both against torch.autograd through the sampler's own sample((0, "lap"))."""
    from diff_gaussian_sampling import GaussianSampler
    from tools.prof_step import list_stats
    args, exp, key = binned_problem_c2(name)
    M = args[3].shape[0]
    rng = np.random.default_rng(5)
    t = [dev32(a) for a in (args[0], args[2], args[1], args[3])]
    for x in t[:3]:
        x.requires_grad_(True)
    target = dev32(rng.uniform(-1, 1, (M, 2)))
    K = coefficients(rng, M, 2)
    Kd = on_device(K)
    K = as_seen(Kd, K)
    s = GaussianSampler(True, backend="binned")
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert s._plan is not None
    if key is not None:
        assert list_stats(s._plan)[key] > 0, name
    r = call(s, Kd, target)
    want, scale = expectation(exp, K, np64(target), 2, each=False)
    err = np.abs(np64(r) - want).max() / scale
    print(f"forward: {err:.3g} of the term scale {scale:.3g}")
    assert err < 1e-5
    w = dev32(rng.uniform(-1, 1, (M, 2)))
    g = torch.autograd.grad((r * w).sum(), t[:3])
    # (a Gaussian's gradient depends on no other Gaussian: at 12 000 x 60 000 the oracle's bound is evaluated for every
    # third one -- its floor, a fraction of the largest entry among them, is then no larger than the full set's)
    sel = slice(None, None, 3 if name == "points" else 1)
    bad = grads_within_accumulation_bound((g[0][sel], g[2][sel], g[1][sel]), [a[sel] for a in args[:3]] + [args[3]],
                                          incoming(np64(w), K, 2, 2))
    assert not bad, bad
    check_against_own_composition(s, t[:3], Kd, target, w)


# ------------------------------------------------------------------------------------------
# 4. the wave recipe
# ------------------------------------------------------------------------------------------
Q0_WAVE, QL_WAVE = np.array(((0.0, -1.0), (0.0, 0.1))), np.array(((0.0, 0.0), (-10.0, 0.0)))


def wave_residual(cur, prev, tau, dt):
    """The two launches of the recipe: the frozen level's part as the target of the current one's."""
    with torch.no_grad():
        T = prev.residual(a0=1 / dt, couple_weight=tau, couple0=-Q0_WAVE, couple_lap=-QL_WAVE)
    return cur.residual(a0=1 / dt, couple_weight=1 - tau, couple0=Q0_WAVE, couple_lap=QL_WAVE, target=T)


def wave_by_hand(img, uxx, prev_img, prev_uxx, time_samples, dt, d):
    """test_no_mlp.py:127-139 (d = 2) and test_no_mlp_1d.py:144-146 (d = 1), literally; returns (res0, res1) with
    loss = mean(res0^2) + 0.01 mean(res1^2)"""
    ut = (img - prev_img) / dt
    u = time_samples.reshape(-1, 1) * prev_img + (1 - time_samples.reshape(-1, 1)) * img
    uxx = time_samples.reshape(-1, 1, 1, 1) * prev_uxx + (1 - time_samples.reshape(-1, 1, 1, 1)) * uxx
    lap0 = uxx[:, 0, 0, 0] + uxx[:, 1, 1, 0] if d == 2 else uxx[:, 0, 0, 0]
    return ut[:, 0] - u[:, 1], ut[:, 1] - (10 * lap0 - 0.1 * u[:, 1])


def run_wave_recipe(host, backend, d):
    from diff_gaussian_sampling import GaussianSampler
    M, dt = 1024, 0.01
    gen = torch.Generator().manual_seed(1)
    if d == 2:
        cur_g, prev_g = (synthetic.lattice_gaussians(20, 20, 1.1, seed=k, c=2) for k in (5, 6))
        t, p = ({k: v.float().cuda() for k, v in g.items()} for g in (cur_g, prev_g))
    else:
        def line(seed):
            g = torch.Generator().manual_seed(seed)
            return {"means": (torch.rand((300, 1), generator=g) * 2 - 1).cuda(),
                    "values": (torch.rand((300, 2), generator=g) * 2 - 1).cuda(),
                    "conics": (1.0 / (0.02 + 0.05 * torch.rand((300, 1), generator=g)) ** 2).cuda()}
        t, p = line(5), line(6)
    leaves = [t[k].requires_grad_(True) for k in ("means", "values", "conics")]
    pts = (torch.rand((M, d), generator=gen) * 2 - 1).cuda()
    tau = torch.rand((M,), generator=gen).cuda()
    prev = GaussianSampler(False, backend=backend, host=host)
    cur = GaussianSampler(False, backend=backend, host=host)
    with torch.no_grad():
        prev.preprocess(p["means"], p["values"], None, p["conics"], pts)
        prev_img, prev_uxx = prev.sample_gaussians(), prev.sample_gaussians_laplacian()
    cur.preprocess(leaves[0], leaves[1], None, leaves[2], pts)
    assert (cur._plan is not None) == (backend == "binned")
    res0, res1 = wave_by_hand(cur.sample_gaussians(), cur.sample_gaussians_laplacian(), prev_img, prev_uxx, tau, dt, d)
    loss_ref = res0.pow(2).mean() + 0.01 * res1.pow(2).mean()
    g_ref = torch.autograd.grad(loss_ref, leaves)
    r = wave_residual(cur, prev, tau, dt)
    # the terms of either residual: u / dt, the blended u and 10 lap u
    scale = max(float(prev_img.abs().max()), float(cur.sample_gaussians().detach().abs().max())) / dt
    lap_max = float(prev_uxx.abs().max())
    scale = max(scale, 10 * lap_max)
    fwd = max(float((r[:, 0] - res0).detach().abs().max()), float((r[:, 1] - res1).detach().abs().max())) / scale
    loss = r[:, 0].pow(2).mean() + 0.01 * r[:, 1].pow(2).mean()
    g = torch.autograd.grad(loss, leaves)
    errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g, g_ref)]
    loss, loss_ref = float(loss.detach()), float(loss_ref.detach())
    print(f"wave recipe: residuals {fwd:.3g} of the term scale, loss {abs(loss - loss_ref) / loss_ref:.3g}, gradients {errs}")
    assert fwd < FWD_OWN, fwd
    assert abs(loss - loss_ref) / loss_ref < GRAD_OWN
    assert max(errs) < GRAD_OWN, errs


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_wave_recipe(hip_lib, host, backend):
    """Residuals, loss and gradients of the two-launch recipe against the loss written with sample_gaussians() and
    sample_gaussians_laplacian() and the reference's own expressions, within the bars of the own composition."""
    run_wave_recipe(host, backend, 2)


def test_wave_recipe_in_one_dimension(hip_lib):
    run_wave_recipe("ctypes", "dense", 1)


# ------------------------------------------------------------------------------------------
# 5. degenerate and policy cases
# ------------------------------------------------------------------------------------------
def coupled_problem(M=1500, seed=8, grad=True):
    t, pts, tau = small_problem(c=2, M=M, seed=seed, grad=grad)
    gen = torch.Generator().manual_seed(seed + 1)
    target = torch.rand((M, 2), generator=gen).cuda()
    w = (torch.rand((M, 2), generator=gen) * 2 - 1).cuda()
    return t, pts, tau, target, w


QA, QB = ((0.3, -0.8), (0.5, 0.2)), ((0.001, 0.003), (-0.002, 0.0015))


def close(a, b, scale, g_a, g_b):
    assert float((a - b).detach().abs().max()) / scale < FWD_OWN
    for x, y in zip(g_a, g_b):
        assert float((x - y).abs().max() / y.abs().max()) < GRAD_OWN


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_degenerate_couplings(hip_lib, host, backend):
    """A constant couple_weight field is the float; zero matrices are the uncoupled residual(a0, lap, target) of the
    linear kernel; the identity couple0 under a weight cw adds cw to a0."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau, target, w = coupled_problem()
    M = pts.shape[0]
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    assert (s._plan is not None) == (backend == "binned")
    u, lap = (x.detach() for x in s.sample((0, "lap")))
    scale = max(1.7 * float(u.abs().max()), 0.01 * float(lap.abs().max()), 1.0)

    def run(**kw):
        r = s.residual(target=target, **kw)
        return r, torch.autograd.grad((r * w).sum(), t)

    r_f, g_f = run(a0=1.7, lap=-0.01, couple_weight=0.6, couple0=QA, couple_lap=QB)
    r_t, g_t = run(a0=1.7, lap=-0.01, couple_weight=torch.full((M, 1), 0.6).cuda(), couple0=QA, couple_lap=QB)
    assert torch.equal(r_f, r_t)
    assert all(rel(a, b) < 2e-6 for a, b in zip(g_t, g_f))          # the backward's atomics, as between any two runs
    r_lin, g_lin = run(a0=1.7, lap=-0.01)
    assert r_lin.grad_fn.name() in ("_ResidualFunctionBackward", "PigsResidualBackward")      # the linear kernel's node
    r_z, g_z = run(a0=1.7, lap=-0.01, couple0=((0, 0), (0, 0)), couple_weight=tau)
    close(r_z, r_lin, scale, g_z, g_lin)
    r_id, g_id = run(a0=1.0, lap=-0.01, couple0=np.eye(2), couple_weight=0.7)
    close(r_id, r_lin, scale, g_id, g_lin)
    r_idf, g_idf = run(a0=tau, lap=-0.01, couple0=torch.eye(2), couple_weight=1.7 - tau)
    close(r_idf, r_lin, scale, g_idf, g_lin)


@pytest.mark.parametrize("host", HOSTS)
def test_arguments_are_checked(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau, target, w = coupled_problem(M=700)
    M = pts.shape[0]
    s = GaussianSampler(False, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    with pytest.raises(ValueError, match="couple0 / couple_lap"):
        s.residual(a0=1.0, couple_weight=tau)
    for name in ("couple0", "couple_lap"):
        for bad in (((1.0, 0.0),), ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), np.eye(3), 1.0, (1.0, 2.0)):
            with pytest.raises(ValueError, match="c x c"):
                s.residual(a0=1.0, **{name: bad})
        with pytest.raises(ValueError, match="constants"):
            s.residual(a0=1.0, **{name: torch.eye(2).requires_grad_(True)})
    with pytest.raises(ValueError, match="constants"):
        s.residual(a0=1.0, couple0=QA, couple_weight=tau.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="device"):
        s.residual(a0=1.0, couple0=QA, couple_weight=tau.cpu())
    for bad in (tau[:-1], torch.zeros((M, 2)).cuda(), torch.zeros((2, M)).cuda()):
        with pytest.raises(ValueError):
            s.residual(a0=1.0, couple0=QA, couple_weight=bad)
    for kw in (dict(a1=(0.1, 0.0)), dict(a1=torch.zeros((M, 2)).cuda()), dict(advect=0.5), dict(advect_by=((1.0, 0.0), (0.0, 1.0))),
               dict(advect=tau, advect_by=((1.0, 0.0), (0.0, 1.0)))):
        with pytest.raises(NotImplementedError, match=r"sample\("):
            s.residual(a0=1.0, couple0=QA, **kw)
    # a zero a1 is no first-derivative term; [M, 1] is [M]; an integer field is cast; the target is checked as ever
    a = s.residual(a0=1.0, a1=(0.0, 0.0), couple0=QA, couple_weight=tau)
    assert torch.equal(a, s.residual(a0=1.0, couple0=QA, couple_weight=tau[:, None]))
    ones = s.residual(a0=1.0, couple_lap=QB, couple_weight=torch.ones((M,), dtype=torch.int64).cuda())
    assert torch.equal(ones, s.residual(a0=1.0, couple_lap=QB))
    with pytest.raises(ValueError, match="target"):
        s.residual(a0=1.0, couple0=QA, target=target[:-1])
    # one channel: nothing to couple
    t1, pts1, _ = small_problem(c=1)
    s.preprocess(t1[0], t1[1], None, t1[2], pts1)
    with pytest.raises(ValueError, match="a0 / lap"):
        s.residual(a0=1.0, couple0=((1.0,),))
    # three channels on a plan: refused where every binned call is
    t3 = small_problem(c=3)[0]
    with pytest.raises(NotImplementedError):
        b = GaussianSampler(False, backend="binned", host=host)
        b.preprocess(t3[0], t3[1], None, t3[2], pts1)
        b.residual(a0=1.0, couple0=np.eye(3))


@pytest.mark.parametrize("host", HOSTS)
def test_differentiable_call_rebuilds_a_forward_only_plan(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau, target, w = coupled_problem(M=3000)
    kw = dict(a0=tau, lap=-0.01, couple_weight=1 - tau, couple0=QA, couple_lap=QB, target=target)
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
def test_first_call_on_deferred_lists(hip_lib, host):
    """defer_lists=True: the coupled residual as the plan's first sampling call (the lists in a launch of their own)
    equals the call on a plan with its lists built, and every later call finds them."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau, target, w = coupled_problem(M=3000)
    kw = dict(a0=tau, lap=-0.01, couple_weight=1 - tau, couple0=QA, couple_lap=QB, target=target)
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
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_inputs(hip_lib, host, dtype):
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau, target, w = coupled_problem(M=50)
    t = [x.detach().to(dtype).requires_grad_(True) for x in t]
    s = GaussianSampler(True, host=host)
    # M = 0: zero gradients
    s.preprocess(t[0], t[1], None, t[2], pts[:0].to(dtype))
    out = s.residual(a0=1.0, couple0=QA, couple_weight=tau[:0], target=target[:0])
    assert tuple(out.shape) == (0, 2) and out.dtype == dtype
    g = torch.autograd.grad(out.sum(), t)
    assert all(tuple(a.shape) == tuple(x.shape) and not a.any() for a, x in zip(g, t))
    # N = 0: minus the target
    e = [x.detach()[:0].clone().requires_grad_(True) for x in t]
    s.preprocess(e[0], e[1], None, e[2], pts.to(dtype))
    out = s.residual(a0=1.0, couple0=QA, couple_weight=tau, target=target)
    assert torch.equal(out, -target.to(dtype))
    g = torch.autograd.grad(out.sum(), e)
    assert [tuple(a.shape) for a in g] == [(0, 2), (0, 2), (0, 3)]


@pytest.mark.parametrize("host", HOSTS)
def test_debug_mode_and_version_check(hip_lib, host):
    """debug=True synchronises after either launch (an error would surface at the call); an in-place change of a bound
    tensor between the call and its backward is refused."""
    from diff_gaussian_sampling import GaussianSampler
    t, pts, tau, target, w = coupled_problem(M=700)
    for backend in ("dense", "binned"):
        s, q = GaussianSampler(True, backend=backend, host=host), GaussianSampler(False, backend=backend, host=host)
        got = []
        for x in (s, q):
            x.preprocess(t[0], t[1], None, t[2], pts)
            r = x.residual(a0=tau, couple0=QA, couple_lap=QB, target=target)
            got.append((r.detach(), torch.autograd.grad((r * w).sum(), t)))
        # (two plans list a tile's Gaussians in the order their builds' atomics gave: the sums may differ in the last bits)
        assert torch.equal(got[0][0], got[1][0]) if backend == "dense" else rel(got[0][0], got[1][0]) < 2e-6
        assert all(rel(a, b) < 2e-6 for a, b in zip(got[0][1], got[1][1]))      # the backward's atomics
    r = q.residual(a0=tau, couple0=QA)
    with torch.no_grad():
        t[1].add_(0.0)                                                 # an in-place write, whatever it writes
    with pytest.raises(RuntimeError, match="modified in place"):
        r.sum().backward()


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_periodic_sampler(hip_lib, host, backend):
    """An 8 x 8 lattice in [-1, 1)^2 on the torus: the bound images are the Gaussians, so the coupled residual equals the
    composition of the periodic sampler's own outputs."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(8, 8, 0.3, seed=2, c=2)      # (narrow enough for the torus: extent below the period)
    means = gs["means"].float().cuda().requires_grad_(True)
    values, conics = gs["values"].float().cuda().requires_grad_(True), gs["conics"].float().cuda().requires_grad_(True)
    rng = np.random.default_rng(2)
    M = 2500
    pts = dev32(rng.uniform(-1, 1, (M, 2)))
    Kd = on_device(coefficients(rng, M, 2))
    s = GaussianSampler(False, backend=backend, host=host, periodic=(-1.0, 1.0))
    s.preprocess(means, values, None, conics, pts)
    assert (s._plan is not None) == (backend == "binned")
    check_against_own_composition(s, (means, values, conics), Kd, dev32(rng.uniform(-1, 1, (M, 2))),
                                  dev32(rng.uniform(-1, 1, (M, 2))))


# ------------------------------------------------------------------------------------------
# 6. graph capture
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_graphed_step_sees_the_weight_change(hip_lib, host, backend):
    """One step (preprocess, residual, backward) captured and replayed after an in-place change of the couple_weight
    tensor: no host synchronisation in the path, and the field is read at replay time -- the replayed loss follows it."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    t, pts, tau0, target, _ = coupled_problem(M=2000, grad=False)
    sampler = GaussianSampler(False, backend=backend, host=host)

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in t) + (tau0.clone(),)

    def fn(means, values, conics, cw):
        sampler.preprocess(means, values, None, conics, pts)
        r = sampler.residual(a0=10.0, lap=-0.05, couple_weight=cw, couple0=QA, couple_lap=QB, target=target)
        loss = r.pow(2).mean()
        return (loss,) + torch.autograd.grad(loss, (means, values, conics))

    step = GraphedStep(fn, make_inputs)
    gen = torch.Generator().manual_seed(9)
    losses = []
    for trial in range(2):
        with torch.no_grad():
            step.inputs[3].copy_(torch.rand(tau0.shape, generator=gen).cuda() * (1 + 3 * trial))
        got = step()
        torch.cuda.synchronize()
        m, v, c = (x.detach().clone().requires_grad_(True) for x in step.inputs[:3])
        eager = fn(m, v, c, step.inputs[3])
        for a, b in zip(got, eager):
            assert float((a.detach() - b.detach()).abs().max()) <= 2e-6 * float(b.detach().abs().max()) + 1e-30, trial
        losses.append(float(got[0].detach()))
    assert abs(losses[1] - losses[0]) > 1e-3 * losses[0]


# ------------------------------------------------------------------------------------------
# 7. training-loop parity
# ------------------------------------------------------------------------------------------
# 25 steps (10 of fitting, 15 of the wave loss), the tolerance of test_burgers_training_loop_matches_the_oracle_loop
LOOP_STEPS = 25


def wave_loop(sampler, device, mode, steps=LOOP_STEPS, n=10, scale=2.5, dt=0.1):
    """The loop of tests/test_training_gpu.py::run_loop with two channels and the wave loss (test_no_mlp.py:116-139)
    from step 10 on.  mode "residual": the two-launch recipe; "oracle": the same loss from the oracle's outputs."""
    g = torch.Generator(device="cpu").manual_seed(7)
    tx = torch.linspace(-1, 1, n) * 0.6
    gx, gy = torch.meshgrid((tx, tx), indexing="ij")
    raw_means = torch.atanh(torch.stack((gx, gy), dim=-1).reshape(n * n, 2)).to(device).requires_grad_(True)
    raw_scaling = torch.full((n * n, 2), -2.5, device=device, requires_grad=True)
    transform = torch.zeros((n * n, 1), device=device, requires_grad=True)
    values = (0.1 * torch.rand((n * n, 2), generator=g)).to(device).requires_grad_(True)
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
            loss = torch.mean((u[:, 1] - desired) ** 2) + torch.mean(u[:, 0] ** 2)
        else:
            sampler2 = OracleSampler() if mode == "oracle" else sampler.__class__(False, backend=sampler.backend)
            with torch.no_grad():
                sampler2.preprocess(*prev, samples)
            if mode == "residual":
                r = wave_residual(sampler, sampler2, tau, dt)
                res0, res1 = r[:, 0], r[:, 1]
            else:
                with torch.no_grad():
                    pu, _, plap = sampler2.sample((0, 1, "lap"))
                u, _, lap = sampler.sample((0, 1, "lap"))
                ub, lb = tau[:, None] * pu + (1 - tau[:, None]) * u, tau[:, None] * plap + (1 - tau[:, None]) * lap
                ut = (u - pu) / dt
                res0, res1 = ut[:, 0] - ub[:, 1], ut[:, 1] - (10 * lb[:, 0] - 0.1 * ub[:, 1])
            loss = torch.mean(res0 ** 2) + 0.01 * torch.mean(res1 ** 2)
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


@functools.lru_cache(maxsize=None)
def oracle_curve():
    torch.set_num_threads(8)
    return wave_loop(OracleSampler(), torch.device("cpu"), "oracle")


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_wave_training_loop_matches_the_oracle_loop(hip_lib, backend):
    from diff_gaussian_sampling import GaussianSampler
    cpu = oracle_curve()
    s = GaussianSampler(False, backend=backend)
    gpu = wave_loop(s, torch.device("cuda"), "residual")
    assert (s._plan is not None) == (backend == "binned")
    assert np.isfinite(gpu).all() and gpu[9] < gpu[0] and gpu[-1] < gpu[10]
    dev_r = np.abs(gpu - cpu) / np.maximum(np.abs(cpu), 1e-12)
    print(f"{backend}: residual() loop deviates {dev_r.max():.3g} from the oracle loop over {LOOP_STEPS} steps")
    assert dev_r.max() < 2e-3, (dev_r.max(), gpu, cpu)
