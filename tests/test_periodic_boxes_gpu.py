"""GPU: the periodic sampler on boxes other than (-1, 1) ("Boxes"; the boxes are in
tests/test_periodic_boxes.py).  (-1, 1) is the box on which most box mistakes cancel: lo = -hi, L = 2 hi, L = 2, centre
0, L exact in float32.  Every problem here is one of the (-1, 1) problems of the suite moved by
x -> lo + (x + 1) a, a = (hi - lo) / 2 (to_box) -- means and points mapped, conics / a^2, values unchanged -- plus rows planted
exactly on lo, on hi and one representable number to either side of each (tests/test_periodic_gpu.py: problem,
planted_means).  The expectation is the float64 C oracle on the nine stacked images of the mapped inputs, on the box as
the kernel's dtype holds it: both hosts hand over lo and hi - lo as doubles, the kernels cast them, so in float32 the
torus of box B is the one of float32(2 pi), 1.7e-7 away from 2 pi (box_as_held).

Bars: those of tests/test_periodic_gpu.py -- forward 1e-5 (float32) / 1e-11 (float64) of the largest entry, gradients
through check_grads -- and of the (-1, 1) case of each fused output.  None was widened.

Measured on an MI355X (131 tests, 8 s), worst in units of the bar: forward 0.15 and gradients 0.73 (both box D, float32
dense -- its images reach -9.5, where float32 is twice as coarse as at 3), scale law 1.3e-4, box E in float64 below 1e-11.
The planted rows hold periodic_images_kernel to the closed box: on box B a mean one denormal below lo = 0 has
(mu - lo) / L = -0, and only the period the kernel adds to a negative remainder brings it in.
"""
import numpy as np
import pytest
import torch

import test_periodic_gpu as G
from oracle import c_oracle
from pigs_amd import synthetic
from test_aggregate_matrix_gpu import to_box
from test_binned_gpu import dev32
from test_periodic_boxes import BOXES
from test_periodic_gpu import box_as_held, check_grads, np64, oracle_args, periodic_forward, rel, tol_of

pytestmark = pytest.mark.gpu
HOSTS = ("native", "ctypes")
KINDS = [(torch.float32, "dense"), (torch.float64, "dense"), (torch.float32, "binned")]
# (box, dtype, backend): A-D in every kind, E (far from the origin) in float64 only
CONFIGS = [(b, t, k) for b in "ABCD" for t, k in KINDS] + [("E", torch.float64, "dense")]
FORWARD = [(b, t, k, 1) for b, t, k in CONFIGS] + [("C", t, k, 2) for t, k in KINDS]


def half(box):
    return (box[1] - box[0]) / 2.0


def sampler(box, backend, host, debug=True, **kw):
    from diff_gaussian_sampling import GaussianSampler
    return GaussianSampler(debug, backend=backend, host=host, periodic=box, **kw)


def assert_block0_in_the_closed_box(s, N, box, dtype):
    lo, hi = box_as_held(box, dtype)
    assert s._inputs[0].shape == (9 * N, 2)
    b0 = s._inputs[0][:N].detach().double()
    assert float(b0.min()) >= lo and float(b0.max()) <= hi, (float(b0.min()), float(b0.max()), lo, hi)


def check_forward(s, t, box, dtype, what):
    """Orders 0-3 and "lap" against the image oracle; returns the worst error in units of the bar."""
    u, du, lap = s.sample((0, 1, "lap"))
    hess, third = s.sample((2, 3))
    exp = periodic_forward(*oracle_args(t), box=box_as_held(box, dtype))
    errs = [rel(out, exp[o]) for o, out in enumerate((u, du, hess, third))] + [rel(lap, exp[2][:, 0, 0] + exp[2][:, 1, 1])]
    print(f"{what}: forward (orders 0-3, lap) {np.array2string(np.array(errs) / tol_of(dtype), precision=2)} of the bar")
    for o, out in enumerate((u, du, hess, third)):
        assert out.dtype == dtype
    assert max(errs) < tol_of(dtype), errs
    return max(errs) / tol_of(dtype)


# ------------------------------------------------------------------------------------------
# forward, backward, odd rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name,dtype,backend,c", FORWARD)
def test_forward_matches_the_image_oracle(hip_lib, host, name, dtype, backend, c):
    box = BOXES[name]
    t = G.problem(c=c, seed=c, dtype=dtype, box=box, planted=True)
    s = sampler(box, backend, host)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert (s._plan is not None) == (backend == "binned")
    assert_block0_in_the_closed_box(s, 200, box, dtype)
    lo, hi = box_as_held(box, dtype)
    assert float(t[3].min()) == lo and float(t[3].max()) == hi          # the box's own closed grid
    check_forward(s, t, box, dtype, f"box {name} {dtype} {backend} c={c} {host}")


@pytest.mark.parametrize("name,dtype", [(b, t) for b in "ABCD" for t in (torch.float32, torch.float64)] + [("E", torch.float64)])
def test_hosts_make_the_same_images(hip_lib, name, dtype):
    box = BOXES[name]
    t = G.problem(c=2, seed=51, dtype=dtype, box=box, planted=True)
    imgs = []
    for host in HOSTS:
        s = sampler(box, "dense", host, debug=False)
        s.preprocess(t[0], t[1], None, t[2], t[3])
        imgs.append([x.detach() for x in s._inputs[:3]])
    for a, b in zip(*imgs):
        assert torch.equal(a, b)
    # the nine blocks are block 0 moved by whole periods of the dtype's own period, in the documented order
    lo, hi = box_as_held(box, dtype)
    m = imgs[0][0].double().reshape(9, 200, 2)
    shifts = torch.tensor([(0, 0), (-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)],
                          dtype=torch.float64, device="cuda") * (hi - lo)
    want = (m[0][None] + shifts[:, None, :]).to(dtype).double()
    assert torch.equal(m, want)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name,dtype,backend", CONFIGS)
def test_backward_matches_the_folded_oracle(hip_lib, host, name, dtype, backend):
    box = BOXES[name]
    orders = (0, 1, 2, 3)
    t = G.problem(N=160, c=2, seed=11, dtype=dtype, box=box, planted=True)
    s = sampler(box, backend, host)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    outs = s.sample(orders)
    rng = np.random.default_rng(3)
    ws = {o: rng.uniform(-1, 1, tuple(out.shape)) for o, out in zip(orders, outs)}
    loss = sum((out * torch.as_tensor(ws[o], dtype=dtype, device="cuda")).sum() for o, out in zip(orders, outs))
    g = torch.autograd.grad(loss, (t[0], t[2], t[1]))
    worst = check_grads(g, *oracle_args(t), ws, dtype, box=box_as_held(box, dtype))
    print(f"box {name} {dtype} {backend} {host}: gradients {worst:.3g} of the bar")


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("c,N,offset", [(4, 161, 1), (3, 161, 0)])
def test_wide_odd_and_misaligned_rows_on_box_c(hip_lib, host, dtype, c, N, offset):
    """The scalar instantiations of the images kernel and of the fold (tests/test_periodic_gpu.py:
    test_wide_and_odd_rows_forward_and_backward) on a box with lo != -hi."""
    box = BOXES["C"]
    t = G.problem(N=N, c=c, seed=90 + c, dtype=dtype, box=box, planted=True)
    if offset:
        buf = torch.zeros(N * c + offset, dtype=dtype, device="cuda")
        buf[offset:] = t[1].detach().reshape(-1)
        t[1] = buf[offset:].view(N, c).requires_grad_(True)
        assert t[1].is_contiguous() and t[1].data_ptr() % (4 * t[1].element_size()) != 0
    s = sampler(box, "dense", host)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert_block0_in_the_closed_box(s, N, box, dtype)
    outs = s.sample((0, 1, 2, 3))
    args = oracle_args(t)
    exp = periodic_forward(*args, box=box_as_held(box, dtype))
    for o, out in enumerate(outs):
        assert rel(out, exp[o]) < tol_of(dtype), (o, rel(out, exp[o]))
    rng = np.random.default_rng(c + N)
    ws = {o: rng.uniform(-1, 1, tuple(out.shape)) for o, out in enumerate(outs)}
    loss = sum((out * torch.as_tensor(ws[o], dtype=dtype, device="cuda")).sum() for o, out in enumerate(outs))
    check_grads(torch.autograd.grad(loss, (t[0], t[2], t[1])), *args, ws, dtype, box=box_as_held(box, dtype))


# ------------------------------------------------------------------------------------------
# laws: scale, ends, whole periods, translation
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_scale_law_against_the_unit_box(hip_lib, host, name):
    """Float64 dense: the outputs on the box are those of the (-1, 1) problem times a^-k for order k, to 1e-10 of each
    output's largest entry (kernel against kernel: no oracle, no box handed to any checker)."""
    box = BOXES[name]
    a = half(box)
    outs = []
    for b in ((G.LO, G.HI), box):
        t = G.problem(c=2, seed=17, dtype=torch.float64, box=None if b == (G.LO, G.HI) else b)
        s = sampler(b, "dense", host)
        s.preprocess(t[0], t[1], None, t[2], t[3])
        outs.append([o.detach() for o in s.sample((0, 1, 2, 3))] + [s.sample((0, "lap"))[1].detach()])
    errs = []
    for k, (base, moved) in zip((0, 1, 2, 3, 2), zip(*outs)):
        errs.append(rel(moved, base * a ** -k))
    print(f"box {name} {host}: scale law {np.array2string(np.array(errs) / 1e-10, precision=2)} of the bar")
    assert max(errs) < 1e-10, errs


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name", ["B", "C"])
def test_grid_ends_agree_for_every_order(hip_lib, host, name):
    """On the box's closed 128 x 128 grid the first and last columns carry the same field, so do the first and last rows
    (test_grid_ends_agree_for_every_order of tests/test_periodic_gpu.py, its bar)."""
    box = BOXES[name]
    t = G.problem(N=256, c=1, seed=21, res=128, box=box, planted=True)
    s = sampler(box, "binned", host, debug=False)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert s._plan is not None
    for o, out in enumerate(s.sample((0, 1, 2, 3))):
        f = out.detach().reshape((128, 128) + tuple(out.shape[1:]))      # [row y][column x]
        scale = float(f.abs().max())
        assert float((f[:, 0] - f[:, -1]).abs().max()) / scale < 1e-5, ("columns", o)
        assert float((f[0] - f[-1]).abs().max()) / scale < 1e-5, ("rows", o)


@pytest.mark.parametrize("host", HOSTS)
def test_translation_and_whole_periods_on_box_c(hip_lib, host):
    box = BOXES["C"]
    lo, hi = box
    a = half(box)
    t = G.problem(N=200, c=1, seed=31, unwrapped=False, box=box)
    pts = torch.rand((3000, 2), generator=torch.Generator().manual_seed(2), dtype=torch.float64).mul(hi - lo).add(lo)
    pts = pts.float().cuda()
    s = sampler(box, "dense", host, debug=False)

    def run(means, samples):
        s.preprocess(means, t[1], None, t[2], samples)
        outs = s.sample((0, 1, 2, 3))
        g = torch.autograd.grad(sum(o.sum() for o in outs), (means, t[1], t[2]))
        return [o.detach() for o in outs], g

    base, g0 = run(t[0], pts)
    exp = periodic_forward(np64(t[0]), np64(t[2]), np64(t[1]), np64(pts), box=box)       # the base itself is right
    for o in range(4):
        assert rel(base[o], exp[o]) < 1e-5, (o, rel(base[o], exp[o]))
    shift = torch.tensor([0.37 * a, -0.81 * a], device="cuda")
    moved = (t[0].detach() + shift).requires_grad_(True)
    pts_moved = lo + torch.remainder(pts + shift - lo, hi - lo)       # wrapped back into the box by the test
    for o, (x, y) in enumerate(zip(run(moved, pts_moved)[0], base)):
        assert rel(x, y) < 1e-5, ("translation", o, rel(x, y))
    plus_l = (t[0].detach() + torch.tensor([hi - lo, 0.0], device="cuda")).requires_grad_(True)
    outs, g1 = run(plus_l, pts)
    for o, (x, y) in enumerate(zip(outs, base)):
        assert rel(x, y) < 1e-5, ("mu + L", o, rel(x, y))
    for name, x, y in zip(("means", "values", "conics"), g1, g0):
        assert rel(x, y) < 1e-5, ("mu + L gradient", name, rel(x, y))


# ------------------------------------------------------------------------------------------
# the debug-mode extent check
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("name", ["A", "C"])
def test_debug_mode_extent_check_scales_with_the_box(hip_lib, host, name):
    """sqrt(44 * 0.1) a = 2.10 a > L = 2 a > 1.97 a = sqrt(44 * 0.088) a: a check against hi, against 2 or against
    L without its square gets one side wrong on a box with L != 2."""
    box = BOXES[name]
    a2 = half(box) ** 2
    t = G.problem(N=64, c=1, seed=71, box=box, planted=True)
    s = sampler(box, "dense", host)

    def with_conic(k, con):
        c = t[2].detach().clone()
        c[k] = torch.tensor(con, dtype=c.dtype, device="cuda")
        return c

    def conic(cov):
        return G.conic_of(*(v * a2 for v in cov))

    too_wide = {"x only": (0.1, 0.0, 0.001), "y only": (0.001, 0.0, 0.1), "correlated": (0.1, 0.095, 0.1),
                "isotropic": (0.5, 0.0, 0.5)}
    for case, cov in too_wide.items():
        with pytest.raises(ValueError, match="period"):
            s.preprocess(t[0], t[1], None, with_conic(5, conic(cov)), t[3])
    just_short = {"x only": (0.088, 0.0, 0.001), "y only": (0.001, 0.0, 0.088), "correlated": (0.088, 0.0836, 0.088)}
    for case, cov in just_short.items():
        s.preprocess(t[0], t[1], None, with_conic(5, conic(cov)), t[3])
    with pytest.raises(ValueError, match="positive definite"):
        s.preprocess(t[0], t[1], None, with_conic(7, [1.0, 2.0, 1.0]), t[3])
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert s.sample_gaussians().shape == (t[3].shape[0], 1)
    wide = with_conic(5, conic(too_wide["x only"]))
    sampler(box, "dense", host, debug=False).preprocess(t[0], t[1], None, wide, t[3])       # flag=False: not checked


# ------------------------------------------------------------------------------------------
# one sampler, several boxes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
def test_changing_the_box_on_one_sampler(hip_lib, host):
    """(-1, 1) -> C -> (-1, 1) -> None through the setter, N and M the same throughout: the library remembers point-set
    kinds by (device, sizes) and the host reuses sample plans -- nothing of one box may reach the next."""
    from diff_gaussian_sampling import GaussianSampler
    unit = (G.LO, G.HI)
    s = GaussianSampler(True, backend="binned", host=host, periodic=unit)
    for step, box in enumerate((unit, BOXES["C"], unit, None)):
        s.periodic = box
        t = G.problem(c=1, seed=5, unwrapped=box is not None, box=None if box in (unit, None) else box,
                      planted=box not in (unit, None))
        s.preprocess(t[0], t[1], None, t[2], t[3])
        assert s._plan is not None
        assert s._inputs[0].shape[0] == (200 if box is None else 1800) and t[3].shape[0] == 4096
        outs = s.sample((0, 1, 2))
        args = oracle_args(t)
        exp = c_oracle.forward(*args, orders=(0, 1, 2)) if box is None else \
            periodic_forward(*args, orders=(0, 1, 2), box=box_as_held(box, torch.float32))
        for o, out in enumerate(outs):
            assert rel(out, exp[o]) < 1e-5, (step, box, o, rel(out, exp[o]))
        ws = {o: np.random.default_rng(step).uniform(-1, 1, tuple(out.shape)) for o, out in enumerate(outs)}
        loss = sum((out * dev32(ws[o])).sum() for o, out in enumerate(outs))
        g = torch.autograd.grad(loss, (t[0], t[2], t[1]))
        if box is None:
            from conftest import grads_within_accumulation_bound
            bad = grads_within_accumulation_bound(g, args, ws)
            assert not bad, bad
        else:
            check_grads(g, *args, ws, torch.float32, box=box_as_held(box, torch.float32))


# ------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_captured_step_on_box_c_matches_eager(hip_lib, host, backend):
    """test_captured_periodic_step_matches_eager of tests/test_periodic_gpu.py on box C, its bars; the means drift
    across hi."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    box = BOXES["C"]
    a = half(box)
    t0 = G.problem(N=144, c=1, seed=61, unwrapped=False, box=box)
    init = [x.detach().clone() for x in t0[:3]]
    pts = t0[3]
    M = pts.shape[0]
    gen = torch.Generator().manual_seed(6)
    rs = [(torch.rand(sh, generator=gen) * 2 - 1).cuda() for sh in ((M, 1), (M, 2, 1), (M, 2, 2, 1))]
    graphed = GaussianSampler(False, backend=backend, fuse="all", host=host, periodic=box)
    eager = GaussianSampler(False, backend=backend, fuse="all", host=host, periodic=box)

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in init)

    def step_with(smp, means, values, conics):
        smp.preprocess(means, values, None, conics, pts)
        outs = smp.sample((0, 1, 2))
        loss = sum((o * r).sum() for o, r in zip(outs, rs))
        return (loss,) + tuple(torch.autograd.grad(loss, (means, values, conics)))

    step = GraphedStep(lambda m, v, c: step_with(graphed, m, v, c), make_inputs)
    rng = np.random.default_rng(1)
    for trial in range(4):
        with torch.no_grad():
            step.inputs[0].add_(torch.as_tensor(rng.normal([0.15 * a, 0.05 * a], 0.02 * a, (len(init[0]), 2)),
                                                 dtype=torch.float32, device="cuda"))
        got = [x.clone() for x in step()]
        m, v, c = (x.detach().clone().requires_grad_(True) for x in step.inputs)
        want = step_with(eager, m, v, c)
        for k, (x, y) in enumerate(zip(got, want)):
            bar = 2e-6 if backend == "binned" and k > 0 else 1e-6
            assert rel(x, y) < bar, (trial, k, rel(x, y))
    assert float(step.inputs[0].detach()[:, 0].max()) > box[1]          # the caller's means did cross hi
    # and the last replay is right, not only equal to eager: the outputs of the eager sampler against the oracle
    args = [np64(m), np64(c), np64(v), np64(pts)]
    exp = periodic_forward(*args, orders=(0, 1, 2), box=box)
    for o, out in enumerate(eager.sample((0, 1, 2))):
        assert rel(out, exp[o]) < 1e-5, (o, rel(out, exp[o]))


# ------------------------------------------------------------------------------------------
# fused outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,backend", KINDS)
@pytest.mark.parametrize("name", ["A", "C"])
def test_residual_with_constant_coefficients(hip_lib, host, name, dtype, backend):
    """test_residual_periodic of tests/test_periodic_gpu.py: its coefficients, composition and bars."""
    box = BOXES[name]
    t = G.problem(N=200, c=1, seed=41, dtype=dtype, box=box, planted=True)
    M = t[3].shape[0]
    rng = np.random.default_rng(4)
    target = torch.as_tensor(rng.uniform(-1, 1, (M, 1)), dtype=dtype, device="cuda")
    a0, a1, aL = 1.7, (0.12, -0.07), -0.003
    s = sampler(box, backend, host)
    s.preprocess(t[0], t[1], None, t[2], t[3])
    r = s.residual(a0=a0, a1=a1, lap=aL, target=target)
    args = oracle_args(t)
    held = box_as_held(box, dtype)
    exp = periodic_forward(*args, orders=(0, 1, 2), box=held)
    lap = exp[2][:, 0, 0] + exp[2][:, 1, 1]
    want = a0 * exp[0] + a1[0] * exp[1][:, 0] + a1[1] * exp[1][:, 1] + aL * lap - np64(target)
    scale = max(a0 * np.abs(exp[0]).max(), abs(aL) * np.abs(lap).max(), 1.0)
    err = np.abs(np64(r) - want).max() / scale
    w = rng.uniform(-1, 1, (M, 1))
    g = torch.autograd.grad((r * torch.as_tensor(w, dtype=dtype, device="cuda")).sum(), (t[0], t[2], t[1]))
    g2 = np.zeros((M, 2, 2, 1))
    g2[:, 0, 0] = g2[:, 1, 1] = aL * w
    assert err < tol_of(dtype), err
    worst = check_grads(g, *args, {0: a0 * w, 1: np.stack((a1[0] * w, a1[1] * w), 1), 2: g2}, dtype, box=held)
    print(f"box {name} residual {dtype} {backend} {host}: forward {err / tol_of(dtype):.3g}, gradients {worst:.3g} of the bars")


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
@pytest.mark.parametrize("name", ["B", "C"])
def test_vorticity_terms(hip_lib, host, backend, name):
    """test_periodic_matches_the_oracle_on_the_images of tests/test_vorticity_gpu.py on the box."""
    import test_vorticity_gpu as V
    from test_vorticity import expand
    box = BOXES[name]
    means, values, con, pts, gout = V.periodic_problem(box=box)
    t = V.leaves_of(means, values, con)
    pts_t, gout_t = dev32(pts), dev32(gout)
    s = sampler(box, backend, host)
    s.preprocess(t[0], t[1], None, t[2], pts_t)
    assert (s._plan is not None) == (backend == "binned")
    assert_block0_in_the_closed_box(s, 64, box, torch.float32)
    out = s.vorticity_terms()
    args = V.oracle_args(t, pts_t)
    held = box_as_held(box, torch.float32)
    exp = periodic_forward(*args, box=held)
    errs = V.column_errors(out, exp)
    print(f"box {name} vorticity_terms {backend} {host}: forward, per column of its scale: {np.array2string(errs, precision=2)}")
    assert errs.max() < 1e-5, errs
    g = torch.autograd.grad((out * gout_t).sum(), t)
    assert g[0].shape == (64, 2) and g[1].shape == (64, 2) and g[2].shape == (64, 3)
    check_grads((g[0], g[2], g[1]), *args, expand(np64(gout_t)), torch.float32, box=held)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
@pytest.mark.parametrize("name", ["B", "C"])
def test_vorticity_residual(hip_lib, host, backend, name):
    """test_periodic_matches_the_oracle_on_the_images of tests/test_vorticity_residual_gpu.py on the box."""
    import test_vorticity_gpu as V
    import test_vorticity_residual_gpu as R
    from test_vorticity import combine, expand
    from test_vorticity_residual import adjoint, compose
    box = BOXES[name]
    means, values, con, pts, _ = V.periodic_problem(box=box)
    rng = np.random.default_rng(31)
    t = V.leaves_of(means, values, con)
    pts_t = dev32(pts)
    M = len(pts)
    tau_t, gout_t = dev32(rng.uniform(0, 1, M)), dev32(rng.uniform(-1, 1, (M, 2)))
    args = V.oracle_args(t, pts_t)
    held = box_as_held(box, torch.float32)
    exp = periodic_forward(*args, box=held)
    exp_prev = periodic_forward(args[0], args[1], np64(dev32(R.other_values(values, 9))), args[3], box=held)
    prev_t = dev32(combine(exp_prev))
    s = sampler(box, backend, host)
    s.preprocess(t[0], t[1], None, t[2], pts_t)
    assert (s._plan is not None) == (backend == "binned")
    out = R.residual_of(s, prev_t, tau_t)
    now7, prev7, tau, gout = combine(exp), np64(prev_t), np64(tau_t), np64(gout_t)
    errs = R.column_errors(out, compose(now7, prev7, tau, R.NU, R.DT, R.TT), R.bars((exp, exp_prev)))
    print(f"box {name} vorticity_residual {backend} {host}: forward (div, r) of their scales: {np.array2string(errs, precision=2)}")
    assert errs.max() < 1e-5, errs
    g = torch.autograd.grad((out * gout_t).sum(), t)
    check_grads((g[0], g[2], g[1]), *args, expand(adjoint(gout, now7, prev7, tau, R.NU, R.DT, R.TT)), torch.float32, box=held)


def lattice_on_box_c(M=2500):
    """The 8 x 8 lattice of the periodic cases of tests/test_residual_terms_gpu.py / test_residual_coupled_gpu.py and
    their M random points, moved onto box C."""
    box = BOXES["C"]
    gs = synthetic.lattice_gaussians(8, 8, 0.3, seed=2, c=2)
    means, conics = (x.float().cuda().requires_grad_(True) for x in to_box(gs["means"].double(), gs["conics"].double(), box))
    values = gs["values"].float().cuda().requires_grad_(True)
    rng = np.random.default_rng(2)
    pts = dev32(to_box(rng.uniform(-1, 1, (M, 2)), None, box)[0])
    return box, rng, means, values, conics, pts


def check_own_outputs(s, means, values, conics, pts, box):
    """The composition's ingredients are the periodic field of the box: orders 0-2 against the image oracle."""
    exp = periodic_forward(np64(means), np64(conics), np64(values), np64(pts), orders=(0, 1, 2),
                           box=box_as_held(box, torch.float32))
    for o, out in enumerate(s.sample((0, 1, 2))):
        assert rel(out, exp[o]) < 1e-5, (o, rel(out, exp[o]))


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_residual_with_per_point_coefficients_on_box_c(hip_lib, backend):
    import test_residual_terms_gpu as T
    box, rng, means, values, conics, pts = lattice_on_box_c()
    M = pts.shape[0]
    F = tuple(dev32(x) for x in T.fields(rng, M, 2))
    s = sampler(box, backend, "native", debug=False)
    s.preprocess(means, values, None, conics, pts)
    assert (s._plan is not None) == (backend == "binned")
    check_own_outputs(s, means, values, conics, pts, box)
    T.check_against_own_composition(s, (means, values, conics), F, T.BY[(2, 2)], dev32(rng.uniform(-1, 1, (M, 2))), 2,
                                    dev32(rng.uniform(-1, 1, (M, 2))))


@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_coupled_residual_on_box_c(hip_lib, backend):
    import test_residual_coupled_gpu as Q
    box, rng, means, values, conics, pts = lattice_on_box_c()
    M = pts.shape[0]
    Kd = Q.on_device(Q.coefficients(rng, M, 2))
    s = sampler(box, backend, "ctypes", debug=False)
    s.preprocess(means, values, None, conics, pts)
    assert (s._plan is not None) == (backend == "binned")
    check_own_outputs(s, means, values, conics, pts, box)
    Q.check_against_own_composition(s, (means, values, conics), Kd, dev32(rng.uniform(-1, 1, (M, 2))),
                                    dev32(rng.uniform(-1, 1, (M, 2))))
