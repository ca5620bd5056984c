"""GPU: forward-only plans (PIGS_BUILD_FORWARD_ONLY, ABI 9).  A plan that preprocess() builds while no backward can
follow (grad mode off, or none of means / values / conics requires grad) holds the forward's group lists under one
cut-off and no tile lists.  Its outputs are those of a full plan; a differentiable call on it rebuilds the plan in
full first; a backward on such a workspace through the C ABI writes NaN gradients."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grads_within_accumulation_bound
from oracle import c_oracle
from pigs_amd import synthetic

pytestmark = pytest.mark.gpu
HOSTS = ["native", "ctypes"]


def rel(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else a
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def plan_strips(plan):
    """PlanParams::strips of a completed build (the Gaussians kept the caller's order)."""
    from pigs_amd import _lib
    off = _lib.load().pigs_plan_strips_offset()
    return int(plan.workspace[off:off + 4].view(torch.int32).item())


@pytest.mark.parametrize("host", HOSTS)
def test_lattice_strips_outputs_bit_equal(hip_lib, host):
    """C3's shape (Gaussians on a lattice in row order, a lattice of points, kappa = 0.5): the lists come from strips
    in the caller's order, so a forward-only plan's group lists are a full plan's, entry for entry -- u, grad u and
    the Hessian are bit-for-bit the same."""
    from diff_gaussian_sampling import GaussianSampler
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(128, 128, 0.5, seed=0)
    pts = synthetic.grid_samples(512, 512).float().to(dev)
    t = {k: gs[k].float().to(dev) for k in ("means", "values", "conics")}
    req = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    full = GaussianSampler(False, fuse="all", backend="binned", host=host, reuse_samples=False)
    fwd = GaussianSampler(False, fuse="all", backend="binned", host=host, reuse_samples=False)
    for _ in range(4):          # the library's memory settles on strips after the first completed builds
        full.preprocess(req["means"], req["values"], None, req["conics"], pts)
        a = full.sample((0, 1, 2))
        with torch.no_grad():
            fwd.preprocess(t["means"], t["values"], None, t["conics"], pts)
            b = fwd.sample((0, 1, 2))
        torch.cuda.synchronize()
    assert not full._plan.forward_only and fwd._plan.forward_only
    assert plan_strips(full._plan) == 1 and plan_strips(fwd._plan) == 1
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y)


@pytest.mark.parametrize("host", HOSTS)
def test_shuffled_random_wide_c2_order3_match_oracle(hip_lib, host):
    """Shuffled lattice Gaussians (kappa = 1.3, c = 2) at uniform random points, orders 0..3 (the order-3 plan too)
    from forward-only plans: the fp64 oracle at the binned tests' bar."""
    from diff_gaussian_sampling import GaussianSampler
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(40, 40, 1.3, seed=4, c=2)
    perm = torch.randperm(gs["means"].shape[0], generator=torch.Generator().manual_seed(1))
    t = {k: gs[k][perm].float().contiguous().to(dev) for k in ("means", "values", "conics")}
    gen = torch.Generator().manual_seed(8)
    pts = (torch.rand((6000, 2), generator=gen) * 2 - 1).float().to(dev)
    s = GaussianSampler(False, fuse="none", backend="binned", host=host)
    with torch.no_grad():
        s.preprocess(t["means"], t["values"], None, t["conics"], pts)
        outs = s.sample((0, 1, 2, 3))
        assert s._plan.forward_only and s._plan3.forward_only
    args = [t[k].cpu().double().numpy() for k in ("means", "conics", "values")]
    exp = c_oracle.forward(*args, pts.cpu().double().numpy(), orders=(0, 1, 2, 3))
    for o, out in enumerate(outs):
        assert rel(out, exp[o]) < 1e-5, (o, rel(out, exp[o]))


@pytest.mark.parametrize("host", HOSTS)
def test_differentiable_call_rebuilds_a_forward_only_plan(hip_lib, host):
    """preprocess under no_grad, then sample((0, 1, 2)) with grad on and backward(): the plan is rebuilt in full before
    the launch (a new plan object, not forward-only), and the gradients are a full plan's and within the oracle's
    accumulation bound.  The residual with a target that requires grad follows the same rule."""
    from diff_gaussian_sampling import GaussianSampler
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(48, 48, 0.8, seed=2)
    pts = synthetic.grid_samples(160, 160).float().to(dev)
    rng = np.random.default_rng(3)

    def leaves():
        return [gs[k].float().to(dev).requires_grad_(True) for k in ("means", "values", "conics")]

    def run(s, lazy):
        m, v, c = leaves()
        if lazy:
            with torch.no_grad():
                s.preprocess(m, v, None, c, pts)
            before = s._plan
            assert before.forward_only
        else:
            s.preprocess(m, v, None, c, pts)
            before = s._plan
            assert not before.forward_only
        outs = s.sample((0, 1, 2))
        after = s._plan
        assert not after.forward_only
        assert (after is not before) == lazy
        loss = sum((o * torch.as_tensor(r, device=dev)).sum() for o, r in zip(outs, rs))
        loss.backward()
        return [o.detach() for o in outs], (m.grad, c.grad, v.grad)

    rs = [rng.uniform(-1, 1, sh).astype(np.float32) for sh in ((pts.shape[0], 1), (pts.shape[0], 2, 1), (pts.shape[0], 2, 2, 1))]
    o_full, g_full = run(GaussianSampler(True, fuse="all", backend="binned", host=host), False)
    o_lazy, g_lazy = run(GaussianSampler(True, fuse="all", backend="binned", host=host), True)
    for x, y in zip(o_full, o_lazy):      # (the two builds may differ in kind -- cells or strips -- and so in order)
        assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())
    # (preprocess's own reshape of conics -- and of 1-D values -- under no_grad is a view outside autograd: after a
    # no_grad preprocess the gradient reaches the means alone, as before forward-only plans existed)
    x, y = g_full[0], g_lazy[0]           # the backward sums with atomics: same terms, any order
    assert y is not None and float((x - y).abs().max()) <= 1e-5 * float(x.abs().max())
    args = [gs[k].float().double().numpy() for k in ("means", "conics", "values")]
    bad = grads_within_accumulation_bound((y,) + g_full[1:], args + [pts.cpu().double().numpy()],
                                          {k: r.astype(np.float64) for k, r in enumerate(rs)})
    assert not bad, bad

    # the residual: only the target requires grad -- still a differentiable call, the plan is rebuilt
    s = GaussianSampler(True, fuse="all", backend="binned", host=host)
    with torch.no_grad():
        s.preprocess(*[gs[k].float().to(dev) for k in ("means", "values")], None, gs["conics"].float().to(dev), pts)
    assert s._plan.forward_only
    target = torch.zeros((pts.shape[0], 1), device=dev, requires_grad=True)
    r = s.residual(a0=1.0, lap=-0.1, target=target)
    assert not s._plan.forward_only
    r.pow(2).sum().backward()
    assert torch.isfinite(target.grad).all()


def test_backward_on_forward_only_workspace_writes_nan(hip_lib):
    """The C ABI: pigs_plan_backward / pigs_residual_backward on a workspace built with PIGS_BUILD_FORWARD_ONLY write NaN
    gradients (the plan's own flag, read on the device) -- never a gradient with terms missing.  The raw helper
    backward_raw runs such a plan's backward on a full plan of the same inputs and agrees with one."""
    from pigs_amd import host_ctypes as S
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(32, 32, 0.7, seed=5)
    pts = synthetic.grid_samples(96, 96).float().to(dev)
    m, v, c = (gs[k].float().contiguous().to(dev) for k in ("means", "values", "conics"))
    N, M = m.shape[0], pts.shape[0]
    plan = S.Plan(m, v, c, pts, 36.0, q_max_backward=40.0, forward_only=True)
    assert plan.forward_only
    outs = S.forward_raw(m, v, c, pts, 7, plan)          # the forward serves
    g = [torch.ones((M,) + (2,) * k + (1,), device=dev) for k in range(3)]
    gm, gv, gc = (torch.zeros_like(x) for x in (m, v, c))
    lib = hip_lib
    p = ctypes.c_void_p
    sws = plan.samples.workspace
    rc = lib.pigs_plan_backward(p(plan.workspace.data_ptr()), plan.workspace.numel(), p(sws.data_ptr()), sws.numel(),
                                N, M, 1, ctypes.c_float(36.0), 7, p(g[0].data_ptr()), p(g[1].data_ptr()),
                                p(g[2].data_ptr()), None, p(gm.data_ptr()), p(gc.data_ptr()), p(gv.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs[:3])
    assert bool(gm.isnan().all()) and bool(gv.isnan().all()) and bool(gc.isnan().all())
    gm.zero_(); gv.zero_(); gc.zero_()
    coeffs = (ctypes.c_double * 4)(1.0, 0.0, 0.0, -0.1)
    rc = lib.pigs_residual_backward(0, 2, 1, N, M, p(m.data_ptr()), p(c.data_ptr()), p(v.data_ptr()), p(pts.data_ptr()),
                                    coeffs, p(g[0].data_ptr()), p(gm.data_ptr()), p(gc.data_ptr()), p(gv.data_ptr()),
                                    p(plan.workspace.data_ptr()), plan.workspace.numel(), p(sws.data_ptr()), sws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(gm.isnan().all()) and bool(gv.isnan().all()) and bool(gc.isnan().all())
    full = S.Plan(m, v, c, pts, 36.0, q_max_backward=40.0)
    gf = S.backward_raw(m, v, c, pts, g + [None, None], 7, full)
    gr = S.backward_raw(m, v, c, pts, g + [None, None], 7, plan)
    assert plan.full_for_backward(m, v, c, pts) is plan.full_for_backward(m, v, c, pts)
    torch.cuda.synchronize()
    for x, y in zip(gf, gr):
        assert torch.isfinite(x).all() and float((x - y).abs().max()) <= 1e-5 * float(x.abs().max())


@pytest.mark.parametrize("host", HOSTS)
def test_graphed_step_and_replicated_take_full_plans(hip_lib, host):
    """A captured GraphedStep (grad on, leaves that require grad) records full plans; so do the views of
    distributed.replicated() in an eager training step."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    from pigs_amd import distributed
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(32, 32, 0.7, seed=6)
    pts = synthetic.grid_samples(96, 96).float().to(dev)
    sampler = GaussianSampler(False, backend="binned", fuse="all", host=host)

    def make_inputs():
        return tuple(gs[k].float().to(dev).requires_grad_(True) for k in ("means", "values", "conics"))

    def fn(means, values, conics):
        sampler.preprocess(means, values, None, conics, pts)
        u, du, h = sampler.sample((0, 1, 2))
        loss = ((u[:, 0] - (h[:, 0, 0, 0] + h[:, 1, 1, 0])) ** 2).mean() + (du ** 2).mean()
        return (loss,) + torch.autograd.grad(loss, (means, values, conics))

    step = GraphedStep(fn, make_inputs)
    assert sampler._plan.recorded_only and not sampler._plan.forward_only
    loss, gm, gv, gc = step()
    torch.cuda.synchronize()
    assert torch.isfinite(gm).all() and torch.isfinite(gv).all() and torch.isfinite(gc).all()

    s2 = GaussianSampler(False, backend="binned", fuse="all", host=host)
    m, v, c = make_inputs()
    mr, vr, cr = distributed.replicated(m, v, c)
    s2.preprocess(mr, vr, None, cr, pts)
    assert not s2._plan.forward_only
    s2.sample_gaussians().sum().backward()
    assert torch.isfinite(m.grad).all()


def test_raw_backward_on_forward_only_plans_runs_full_on_both_hosts(hip_lib):
    """The raw helpers -- sampler.backward_raw (ctypes) and the native module's backward_raw -- on the forward-only plan
    a no_grad preprocess built: both run the backward on a full plan of the same inputs (built once, kept with the
    forward-only plan) and give a full plan's gradients, not NaN."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd import host_ctypes as S
    from pigs_amd import _pigs_host
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(40, 40, 0.8, seed=7)
    pts = synthetic.grid_samples(128, 128).float().to(dev)
    m, v, c = (gs[k].float().contiguous().to(dev) for k in ("means", "values", "conics"))
    M = pts.shape[0]
    gen = torch.Generator().manual_seed(4)
    g = [torch.rand((M,) + (2,) * k + (1,), generator=gen).to(dev) for k in range(3)] + [None, None]
    ref = S.backward_raw(m, v, c, pts, g, 7, S.Plan(m, v, c, pts, 36.0, q_max_backward=40.0))
    for host, raw in (("native", _pigs_host.backward_raw), ("ctypes", S.backward_raw)):
        s = GaussianSampler(False, backend="binned", fuse="all", host=host)
        with torch.no_grad():
            s.preprocess(m, v, None, c, pts)
        plan = s._plan
        assert plan.forward_only
        got = raw(m, v, c, pts, g, 7, plan)
        again = raw(m, v, c, pts, g, 7, plan)
        assert plan.full_for_backward(m, v, c, pts) is plan.full_for_backward(m, v, c, pts)
        torch.cuda.synchronize()
        for x, y, z in zip(ref, got, again):
            assert torch.isfinite(y).all(), host
            assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max()), host
            assert float((y - z).abs().max()) <= 1e-5 * float(x.abs().max()), host
