"""GPU: the periodic domain (GaussianSampler(..., periodic=(lo, hi)), include/pigs_amd.h ABI 10) against a test-local
periodic oracle: the means wrapped into the box in numpy, the 3 x 3 shifted copies stacked, and the float64 C oracle
run on them; the gradients of the originals are the sums over the nine blocks.  Independent of the HIP images kernel
(its block order included: the oracle stacks its own)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from pigs_amd import synthetic
from test_aggregate_matrix_gpu import to_box

pytestmark = pytest.mark.gpu
HOSTS = ("native", "ctypes")
LO, HI = -1.0, 1.0
SHIFTS = np.array([(kx, ky) for ky in (-1, 0, 1) for kx in (-1, 0, 1)], dtype=np.float64)


def tol_of(dtype):
    return 1e-5 if dtype == torch.float32 else 1e-11


def np64(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def rel(a, b):
    a, b = np64(a), np64(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def images(means, conics, values, lo=LO, hi=HI):
    L = hi - lo
    m = lo + np.mod(np.asarray(means, dtype=np.float64) - lo, L)
    return (np.concatenate([m + s * L for s in SHIFTS]), np.tile(conics, (9, 1)), np.tile(values, (9, 1)))


def fold(g, N):
    return g.reshape((9, N) + g.shape[1:]).sum(0)


def box_as_held(box, dtype):
    """The box as a kernel of ``dtype`` holds it: both hosts hand over lo and hi - lo as doubles and the kernels cast
    them to T, so a float32 run lives on the torus of float32(hi - lo) from float32(lo).  Returned as (lo, hi) in
    float64 with hi - lo that period."""
    lo, period = float(box[0]), float(box[1]) - float(box[0])
    if dtype == torch.float32:
        lo, period = float(np.float32(lo)), float(np.float32(period))
    return lo, lo + period


def periodic_forward(means, conics, values, samples, orders=(0, 1, 2, 3), box=(LO, HI)):
    return c_oracle.forward(*images(means, conics, values, *box), samples, orders=orders)


def periodic_backward(means, conics, values, samples, grads, box=(LO, HI)):
    N = len(means)
    return tuple(fold(g, N) for g in c_oracle.backward(*images(means, conics, values, *box), samples, grads))


def check_grads(got, means, conics, values, samples, grads, dtype, box=(LO, HI)):
    """got = (g_means, g_conics, g_values).  float64: 1e-11 of each tensor's largest entry.  float32: the suite's bars
    (conftest.grads_within_accumulation_bound) restated for the folded gradients -- every entry within 1e-6 of the sum
    of the ABSOLUTE per-pair contributions to it (over all nine images) plus 1e-6 of the folded tensor's largest
    entry -- and the tensor-scale bar, 1e-5 of that largest entry.  Returns the worst figure in units of its bar."""
    N = len(means)
    if dtype == torch.float64:
        want = periodic_backward(means, conics, values, samples, grads, box=box)
        for name, g, w in zip(("means", "conics", "values"), got, want):
            assert rel(g, w) < 1e-11, (name, rel(g, w))
        return max(rel(g, w) for g, w in zip(got, want)) / 1e-11
    img = images(means, conics, values, *box)
    want = [fold(w, N) for w in c_oracle.backward(*img, samples, grads)]
    mag = [fold(m, N) for m in c_oracle.backward(*img, samples, grads, absolute=True)]
    worst = 0.0
    for name, g, w, m in zip(("means", "conics", "values"), got, want, mag):
        g = np64(g).reshape(w.shape)
        ratio = np.abs(g - w) / (1e-6 * m + 1e-6 * np.abs(w).max())
        assert (ratio <= 1.0).all(), (name, float(ratio.max()))
        assert rel(g, w) < 1e-5, (name, rel(g, w))
        worst = max(worst, float(ratio.max()), rel(g, w) / 1e-5)
    return worst


def planted_means(box, dtype):
    """Means exactly on lo, on hi and one representable number to either side of each, in ``dtype`` (12 rows: six on
    each axis, the other coordinate inside the box; then (lo, hi) and (hi, lo), the corners)."""
    npt = np.float32 if dtype == torch.float32 else np.float64
    lo, hi = (npt(v) for v in box_as_held(box, dtype))
    edge = [lo, hi, np.nextafter(lo, npt(-np.inf)), np.nextafter(lo, npt(np.inf)), np.nextafter(hi, npt(-np.inf)),
            np.nextafter(hi, npt(np.inf))]
    mid = [float(lo) + f * (float(hi) - float(lo)) for f in (0.13, 0.29, 0.41, 0.58, 0.77, 0.92)]
    rows = [(float(e), m) for e, m in zip(edge, mid)] + [(m, float(e)) for e, m in zip(edge, mid)]
    return np.array(rows + [(float(lo), float(hi)), (float(hi), float(lo))], dtype=np.float64)


def problem(N=200, c=1, seed=0, dtype=torch.float32, unwrapped=True, res=64, box=None, planted=False):
    """Random Gaussians in the box, an eighth of them within one extent of each seam and a few at the corners, a quarter
    handed over unwrapped (mu +- L, mu +- 2L); variances e^-4.5 .. e^-3 (extent at q_cut = 44 below 1.48 < L = 2).
    Samples: the linspace(-1, 1) grid, both ends included.  ``box`` = (lo, hi): the same problem moved by
    to_box (means and points mapped, conics / a^2; the samples are the box's own closed grid); ``planted``: 14 of the rows are then put exactly on the seams and next to them (planted_means)."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(LO, HI, (N, 2))
    k = N // 8
    means[:k, 0] = rng.choice([-0.97, 0.97], k) + rng.uniform(-0.05, 0.05, k)
    means[k:2 * k, 1] = rng.choice([-0.97, 0.97], k) + rng.uniform(-0.05, 0.05, k)
    means[2 * k:2 * k + 4] = [[0.98, 0.98], [-0.98, 0.98], [0.98, -0.98], [-0.98, -0.98]]
    if unwrapped:
        sel = rng.permutation(N)[:N // 4]
        means[sel] += rng.choice([-2, -1, 1, 2], (len(sel), 2)) * (HI - LO)
    s = np.exp(rng.uniform(-4.5, -3.0, (N, 2)))
    tau = np.tanh(rng.normal(0, 0.5, N)) * np.sqrt(s[:, 0] * s[:, 1])
    det = s[:, 0] * s[:, 1] - tau ** 2
    con = np.stack((s[:, 1] / det, -tau / det, s[:, 0] / det), -1)
    values = rng.uniform(-1, 1, (N, c))
    pts = synthetic.grid_samples(res).numpy()
    if box is not None:
        means, con = to_box(means, con, box)
        pts = to_box(pts.astype(np.float64), None, box)[0]
        if planted:
            means[2 * k + 4:2 * k + 18] = planted_means(box, dtype)
    t = [torch.as_tensor(a, dtype=dtype, device="cuda") for a in (means, values, con, pts)]
    for x in t[:3]:
        x.requires_grad_(True)
    return t


def oracle_args(t):
    """(means, conics, values, samples) in float64 from the tensors the sampler saw (float32 rounding included)."""
    return [np64(t[0]), np64(t[2]), np64(t[1]), np64(t[3])]


CONFIGS = [(torch.float32, "dense", 1), (torch.float32, "dense", 2), (torch.float64, "dense", 1),
           (torch.float64, "dense", 2), (torch.float32, "binned", 1), (torch.float32, "binned", 2)]


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,backend,c", CONFIGS)
def test_forward_matches_periodic_oracle(hip_lib, host, dtype, backend, c):
    from diff_gaussian_sampling import GaussianSampler
    t = problem(c=c, seed=c, dtype=dtype)
    s = GaussianSampler(True, backend=backend, host=host, periodic=(LO, HI))
    s.preprocess(t[0], t[1], None, t[2], t[3])
    assert (s._plan is not None) == (backend == "binned")
    assert s._inputs[0].shape == (9 * t[0].shape[0], 2)
    u, du, lap = s.sample((0, 1, "lap"))
    hess, third = s.sample((2, 3))
    args = oracle_args(t)
    exp = periodic_forward(*args)
    for o, out in enumerate((u, du, hess, third)):
        assert out.dtype == dtype
        assert rel(out, exp[o]) < tol_of(dtype), (o, rel(out, exp[o]))
    assert rel(lap, exp[2][:, 0, 0] + exp[2][:, 1, 1]) < tol_of(dtype)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("orders", [(0,), (1,), (2,), (3,), (0, 1, 2, 3)])
@pytest.mark.parametrize("dtype,backend", [(torch.float32, "dense"), (torch.float64, "dense"), (torch.float32, "binned")])
def test_backward_matches_folded_oracle(hip_lib, host, orders, dtype, backend):
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=160, c=2, seed=11, dtype=dtype)
    s = GaussianSampler(True, backend=backend, host=host, periodic=(LO, HI))
    s.preprocess(t[0], t[1], None, t[2], t[3])
    outs = s.sample(orders)
    rng = np.random.default_rng(3)
    ws = {o: rng.uniform(-1, 1, tuple(out.shape)) for o, out in zip(orders, outs)}
    loss = sum((out * torch.as_tensor(ws[o], dtype=dtype, device="cuda")).sum() for o, out in zip(orders, outs))
    g = torch.autograd.grad(loss, (t[0], t[2], t[1]))
    check_grads(g, *oracle_args(t), ws, dtype)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("c,N,offset", [(4, 161, 1), (4, 160, 0), (3, 161, 0)])
def test_wide_and_odd_rows_forward_and_backward(hip_lib, host, dtype, c, N, offset):
    """The launchers move rows of width 2 / 4 as vectors only where every pointer allows: c = 4 values handed over at
    an odd element offset take the images kernel's scalar instantiation, and with N odd the values block of the flat
    gradient buffers ([means | values | conics], at 2N and 18N elements) is misaligned, so the fold takes its scalar
    one too; c = 4 with N even runs both vector instantiations, c = 3 rows are never vectors."""
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=N, c=c, seed=90 + c, dtype=dtype)
    if offset:
        buf = torch.zeros(N * c + offset, dtype=dtype, device="cuda")
        buf[offset:] = t[1].detach().reshape(-1)
        t[1] = buf[offset:].view(N, c).requires_grad_(True)
        assert t[1].is_contiguous() and t[1].data_ptr() % (4 * t[1].element_size()) != 0
    s = GaussianSampler(True, backend="dense", host=host, periodic=(LO, HI))
    s.preprocess(t[0], t[1], None, t[2], t[3])
    outs = s.sample((0, 1, 2, 3))
    args = oracle_args(t)
    exp = periodic_forward(*args)
    for o, out in enumerate(outs):
        assert rel(out, exp[o]) < tol_of(dtype), (o, rel(out, exp[o]))
    rng = np.random.default_rng(c + N)
    ws = {o: rng.uniform(-1, 1, tuple(out.shape)) for o, out in enumerate(outs)}
    loss = sum((out * torch.as_tensor(ws[o], dtype=dtype, device="cuda")).sum() for o, out in enumerate(outs))
    check_grads(torch.autograd.grad(loss, (t[0], t[2], t[1])), *args, ws, dtype)


@pytest.mark.parametrize("host", HOSTS)
def test_auto_backend_counts_image_pairs(hip_lib, host):
    """backend="auto" switches to the plan at 2^26 pairs; a periodic sampler evaluates 9N * M of them.  N = 2 048,
    M = 4 096: N * M = 2^23 stays dense without periodic, 9 N M > 2^26 goes binned with it."""
    from diff_gaussian_sampling import GaussianSampler
    N, M = 2048, 4096
    assert N * M < GaussianSampler.BINNED_AUTO_MIN_PAIRS <= 9 * N * M
    gs = synthetic.lattice_gaussians(32, 64, 1.0, seed=4)
    t = [gs[k].float().cuda() for k in ("means", "values", "conics")] + [synthetic.grid_samples(64).float().cuda()]
    plain = GaussianSampler(False, host=host)
    plain.preprocess(t[0], t[1], None, t[2], t[3])
    assert plain._plan is None
    auto = GaussianSampler(False, host=host, periodic=(LO, HI))
    auto.preprocess(t[0], t[1], None, t[2], t[3])
    assert auto._plan is not None
    dense = GaussianSampler(False, backend="dense", host=host, periodic=(LO, HI))
    dense.preprocess(t[0], t[1], None, t[2], t[3])
    assert rel(auto.sample_gaussians(), dense.sample_gaussians()) < 1e-5


@pytest.mark.parametrize("host", HOSTS)
def test_gradcheck_f64_across_a_corner(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    rng = np.random.default_rng(5)
    means = np.array([[0.93, 0.95], [-0.96, 0.9], [0.9, -0.94], [-0.92, -0.97], [1.02, 0.97], [-0.99, 1.04]])
    s0 = np.exp(rng.uniform(-3.5, -3.0, (6, 2)))
    tau = 0.3 * np.sqrt(s0[:, 0] * s0[:, 1]) * rng.uniform(-1, 1, 6)
    det = s0[:, 0] * s0[:, 1] - tau ** 2
    con = np.stack((s0[:, 1] / det, -tau / det, s0[:, 0] / det), -1)
    values = rng.uniform(-1, 1, (6, 1))
    pts = np.array([[x, y] for x in (-0.99, 0.0, 0.99) for y in (-0.98, 0.05, 0.97)])
    m, v, cn = (torch.as_tensor(a, dtype=torch.float64, device="cuda").requires_grad_(True) for a in (means, values, con))
    p = torch.as_tensor(pts, dtype=torch.float64, device="cuda")
    s = GaussianSampler(False, backend="dense", fuse="all", host=host, periodic=(LO, HI))

    def f(m_, v_, c_):
        s.preprocess(m_, v_, None, c_, p)
        return s.sample((0, 1, 2, 3))

    assert torch.autograd.gradcheck(f, (m, v, cn), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("host", HOSTS)
def test_grid_ends_agree_for_every_order(hip_lib, host):
    """On linspace(-1, 1)^2 (both ends present) the first and last columns carry the same field, so do the first and
    last rows."""
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=256, c=1, seed=21, res=128)
    s = GaussianSampler(False, backend="binned", host=host, periodic=(LO, HI))
    s.preprocess(t[0], t[1], None, t[2], t[3])
    for o, out in enumerate(s.sample((0, 1, 2, 3))):
        f = out.detach().reshape((128, 128) + tuple(out.shape[1:]))      # [row y][column x]
        scale = float(f.abs().max())
        assert float((f[:, 0] - f[:, -1]).abs().max()) / scale < 1e-5, ("columns", o)
        assert float((f[0] - f[-1]).abs().max()) / scale < 1e-5, ("rows", o)


@pytest.mark.parametrize("host", HOSTS)
def test_translation_and_whole_periods_change_nothing(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=200, c=1, seed=31, unwrapped=False)
    pts = torch.rand((3000, 2), generator=torch.Generator().manual_seed(2), dtype=torch.float64).mul(2).sub(1)
    pts = pts.float().cuda()
    s = GaussianSampler(False, backend="dense", host=host, periodic=(LO, HI))

    def run(means, samples):
        s.preprocess(means, t[1], None, t[2], samples)
        outs = s.sample((0, 1, 2, 3))
        g = torch.autograd.grad(sum(o.sum() for o in outs), (means, t[1], t[2]))
        return [o.detach() for o in outs], g

    base, g0 = run(t[0], pts)
    # shift Gaussians and samples by the same vector; the samples are wrapped back into the box by the test
    shift = torch.tensor([0.37, -0.81], device="cuda")
    moved = (t[0].detach() + shift).requires_grad_(True)
    pts_moved = LO + torch.remainder(pts + shift - LO, HI - LO)
    for o, (a, b) in enumerate(zip(run(moved, pts_moved)[0], base)):
        assert rel(a, b) < 1e-5, ("translation", o, rel(a, b))
    # mu and mu + L: same outputs, same gradients (the wrap is float arithmetic: not bitwise)
    plus_l = (t[0].detach() + torch.tensor([HI - LO, 0.0], device="cuda")).requires_grad_(True)
    outs, g1 = run(plus_l, pts)
    for o, (a, b) in enumerate(zip(outs, base)):
        assert rel(a, b) < 1e-5, ("mu + L", o, rel(a, b))
    for name, a, b in zip(("means", "values", "conics"), g1, g0):
        assert rel(a, b) < 1e-5, ("mu + L gradient", name, rel(a, b))


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,backend", [(torch.float64, "dense"), (torch.float32, "binned")])
def test_torus_recipe_wraps_across_the_seam(hip_lib, host, dtype, backend):
    """tests/golden/ref_test_torus.npz (test_torus.py: a column of Gaussians at x = -0.95) through a periodic sampler."""
    import os
    from diff_gaussian_sampling import GaussianSampler
    from conftest import GOLDEN
    fx = np.load(os.path.join(GOLDEN, "ref_test_torus.npz"))
    t = [torch.as_tensor(fx[k], dtype=dtype, device="cuda") for k in ("means", "values", "conics", "samples")]
    s = GaussianSampler(True, backend=backend, host=host, periodic=(LO, HI))
    s.preprocess(t[0], t[1], t[0].new_tensor(fx["covariances"]), t[2], t[3])
    outs = s.sample((0, 1, 2, 3))
    exp = periodic_forward(*oracle_args(t))
    for o in range(4):
        assert rel(outs[o], exp[o]) < tol_of(dtype), (o, rel(outs[o], exp[o]))
    # the mass really appears across the seam: near x = +1 the non-periodic field is nil, the periodic one is not
    near = fx["samples"][:, 0] > 0.9
    flat = fx["out0_f64"][near]
    assert np.abs(flat).max() < 1e-6
    assert np.abs(np64(outs[0])[near] - flat).max() > 0.1


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,backend", [(torch.float32, "dense"), (torch.float64, "dense"), (torch.float32, "binned")])
def test_residual_periodic(hip_lib, host, dtype, backend):
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=200, c=1, seed=41, dtype=dtype)
    M = t[3].shape[0]
    rng = np.random.default_rng(4)
    target = torch.as_tensor(rng.uniform(-1, 1, (M, 1)), dtype=dtype, device="cuda")
    a0, a1, aL = 1.7, (0.12, -0.07), -0.003
    s = GaussianSampler(True, backend=backend, host=host, periodic=(LO, HI))
    s.preprocess(t[0], t[1], None, t[2], t[3])
    r = s.residual(a0=a0, a1=a1, lap=aL, target=target)
    args = oracle_args(t)
    exp = periodic_forward(*args, orders=(0, 1, 2))
    lap = exp[2][:, 0, 0] + exp[2][:, 1, 1]
    want = a0 * exp[0] + a1[0] * exp[1][:, 0] + a1[1] * exp[1][:, 1] + aL * lap - np64(target)
    scale = max(a0 * np.abs(exp[0]).max(), abs(aL) * np.abs(lap).max(), 1.0)
    assert np.abs(np64(r) - want).max() / scale < tol_of(dtype)
    w = rng.uniform(-1, 1, (M, 1))
    g = torch.autograd.grad((r * torch.as_tensor(w, dtype=dtype, device="cuda")).sum(), (t[0], t[2], t[1]))
    g2 = np.zeros((M, 2, 2, 1))
    g2[:, 0, 0] = g2[:, 1, 1] = aL * w
    check_grads(g, *args, {0: a0 * w, 1: np.stack((a1[0] * w, a1[1] * w), 1), 2: g2}, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hosts_agree_bitwise(hip_lib, dtype):
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=200, c=2, seed=51, dtype=dtype)
    res = {}
    for host in HOSTS:
        s = GaussianSampler(False, backend="dense", host=host, periodic=(LO, HI))
        s.preprocess(t[0], t[1], None, t[2], t[3])
        outs = s.sample((0, 1, 2, 3))
        g = torch.autograd.grad(sum(o.sum() for o in outs), (t[0], t[1], t[2]))
        res[host] = ([o.detach() for o in outs], g, [x.detach() for x in s._inputs[:3]])
    for a, b in zip(res["native"][2], res["ctypes"][2]):          # the images
        assert torch.equal(a, b)
    for a, b in zip(res["native"][0], res["ctypes"][0]):          # same kernels, same geometry: bit-identical
        assert torch.equal(a, b)
    for a, b in zip(res["native"][1], res["ctypes"][1]):          # the dense backward's cross-workgroup atomics
        assert rel(a, b) < 2e-6


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_captured_periodic_step_matches_eager(hip_lib, host, backend):
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    t0 = problem(N=144, c=1, seed=61, unwrapped=False)
    init = [x.detach().clone() for x in t0[:3]]
    pts = t0[3]
    M = pts.shape[0]
    gen = torch.Generator().manual_seed(6)
    rs = [(torch.rand(sh, generator=gen) * 2 - 1).cuda() for sh in ((M, 1), (M, 2, 1), (M, 2, 2, 1))]
    graphed = GaussianSampler(False, backend=backend, fuse="all", host=host, periodic=(LO, HI))
    eager = GaussianSampler(False, backend=backend, fuse="all", host=host, periodic=(LO, HI))

    def make_inputs():
        return tuple(x.clone().requires_grad_(True) for x in init)

    def step_with(sampler, means, values, conics):
        sampler.preprocess(means, values, None, conics, pts)
        outs = sampler.sample((0, 1, 2))
        loss = sum((o * r).sum() for o, r in zip(outs, rs))
        return (loss,) + tuple(torch.autograd.grad(loss, (means, values, conics)))

    step = GraphedStep(lambda m, v, c: step_with(graphed, m, v, c), make_inputs)
    rng = np.random.default_rng(1)
    for trial in range(4):
        with torch.no_grad():     # drift along x: a share of the Gaussians crosses the seam (the sampler wraps them)
            step.inputs[0].add_(torch.as_tensor(rng.normal([0.15, 0.05], 0.02, (len(init[0]), 2)), dtype=torch.float32,
                                                 device="cuda"))
        got = [x.clone() for x in step()]
        m, v, c = (x.detach().clone().requires_grad_(True) for x in step.inputs)
        want = step_with(eager, m, v, c)
        for k, (a, b) in enumerate(zip(got, want)):
            # binned gradients: the order of a tile list's entries and of the backward's sums comes from atomics, as
            # between any two binned runs (tests/test_host_gpu.py: 2e-6)
            bar = 2e-6 if backend == "binned" and k > 0 else 1e-6
            assert rel(a, b) < bar, (trial, k, rel(a, b))
    assert float(step.inputs[0].detach()[:, 0].max()) > HI          # the caller's means did cross


@pytest.mark.parametrize("host", HOSTS)
def test_short_trajectory_across_the_seam(hip_lib, host):
    """20 Adam steps (binned) whose means drift across x = 1 and are wrapped by the caller the way model_pn.py:689-693
    does it; outputs and gradients against the oracle every 5th step."""
    from diff_gaussian_sampling import GaussianSampler
    gs = synthetic.lattice_gaussians(8, 8, 1.0, seed=7)
    means0 = gs["means"].clone()
    means0[:, 0] = 0.55 + 0.4 * (means0[:, 0] + 1) / 2          # x in [0.55, 0.95]
    pts = synthetic.grid_samples(64).float().cuda()
    rng = np.random.default_rng(8)
    var = np.exp(rng.uniform(-4.5, -3.5, (64, 2)))
    tau = 0.4 * np.sqrt(var[:, 0] * var[:, 1]) * rng.uniform(-1, 1, 64)
    det = var[:, 0] * var[:, 1] - tau ** 2
    con = torch.as_tensor(np.stack((var[:, 1] / det, -tau / det, var[:, 0] / det), -1))
    means = means0.float().cuda().requires_grad_(True)
    values = gs["values"].float().cuda().requires_grad_(True)
    conics = con.float().cuda().requires_grad_(True)
    s = GaussianSampler(False, backend="binned", host=host, periodic=(LO, HI))
    with torch.no_grad():         # the target: the same field moved by +0.4 along x
        s.preprocess(means + torch.tensor([0.4, 0.0], device="cuda"), values, None, conics, pts)
        target = s.sample_gaussians().clone()
    opt = torch.optim.Adam([means, values, conics], lr=0.02)
    crossed = False
    for step in range(20):
        s.preprocess(means, values, None, conics, pts)
        u = s.sample_gaussians()
        keep = []
        u.register_hook(lambda g: keep.append(g.detach().cpu().double().numpy()))
        loss = ((u - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        if step % 5 == 4:
            args = [np64(x) for x in (means, conics, values, pts)]
            assert rel(u, periodic_forward(*args, orders=(0,))[0]) < 1e-5, step
            check_grads((means.grad, conics.grad, values.grad), *args, {0: keep[0]}, torch.float32)
        opt.step()
        with torch.no_grad():     # model_pn.py:689-693
            crossed = crossed or bool((means > 1.0).any())
            means[means > 1.0] -= 2.0
            means[means < -1.0] += 2.0
    assert crossed


def conic_of(sxx, sxy, syy):
    det = sxx * syy - sxy * sxy
    return [syy / det, -sxy / det, sxx / det]


@pytest.mark.parametrize("host", HOSTS)
def test_debug_mode_rejects_gaussians_wider_than_a_period(hip_lib, host):
    """The extent is sqrt(q_cut Sigma_ii) on each axis, Sigma the COVARIANCE (not the conic's diagonal): Gaussians long
    along one axis only, and long along the diagonal, are told apart from ones just short of a period."""
    from diff_gaussian_sampling import GaussianSampler
    t = problem(N=64, c=1, seed=71)
    s = GaussianSampler(True, host=host, periodic=(LO, HI))

    def with_conic(k, con):
        c = t[2].detach().clone()
        c[k] = torch.tensor(con, dtype=c.dtype, device="cuda")
        return c

    too_wide = {      # covariance (xx, xy, yy): sqrt(44 * 0.1) = 2.10 > L = 2 on the axis named
        "x only": (0.1, 0.0, 0.001), "y only": (0.001, 0.0, 0.1), "correlated": (0.1, 0.095, 0.1),
        "isotropic": (0.5, 0.0, 0.5)}
    for name, cov in too_wide.items():
        with pytest.raises(ValueError, match="period"):
            s.preprocess(t[0], t[1], None, with_conic(5, conic_of(*cov)), t[3])
    just_short = {    # sqrt(44 * 0.088) = 1.97 < 2: the images suffice
        "x only": (0.088, 0.0, 0.001), "y only": (0.001, 0.0, 0.088), "correlated": (0.088, 0.0836, 0.088)}
    for name, cov in just_short.items():
        s.preprocess(t[0], t[1], None, with_conic(5, conic_of(*cov)), t[3])
    with pytest.raises(ValueError, match="positive definite"):
        s.preprocess(t[0], t[1], None, with_conic(7, [1.0, 2.0, 1.0]), t[3])
    s.preprocess(t[0], t[1], None, t[2], t[3])                      # the well-posed problem passes
    assert s.sample_gaussians().shape == (t[3].shape[0], 1)
    wide = with_conic(5, conic_of(*too_wide["x only"]))
    GaussianSampler(False, host=host, periodic=(LO, HI)).preprocess(t[0], t[1], None, wide, t[3])   # not checked


@pytest.mark.parametrize("host", HOSTS)
def test_d1_is_not_implemented_and_aggregation_uses_the_originals(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(False, host=host, periodic=(LO, HI), unpinned_aggregate=True)
    x = torch.zeros(8, 1, device="cuda")
    with pytest.raises(NotImplementedError):
        s.preprocess(x, torch.ones(8, 1, device="cuda"), None, torch.ones(8, 1, device="cuda"), torch.zeros(16, 1, device="cuda"))
    t = problem(N=100, c=1, seed=81, unwrapped=False)
    feats = torch.randn(100, 4, device="cuda", dtype=torch.float32)
    args = (feats, torch.eye(4, device="cuda"), torch.randn(100, 3, device="cuda"), torch.randn(100, 3, device="cuda"),
            torch.ones(2, device="cuda"), torch.randn(4, 2 * 9, device="cuda"))
    outs = []
    for periodic in ((LO, HI), None):
        a = GaussianSampler(False, host=host, periodic=periodic, unpinned_aggregate=True)
        a.preprocess(t[0], t[1], None, t[2], t[3])
        a.preprocess_aggregate()
        outs.append(a.aggregate_neighbors(*args).detach())
    assert outs[0].shape == (100, 4) and torch.equal(outs[0], outs[1])
