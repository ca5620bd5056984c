"""GPU: ``GaussianSampler(periodic=(lo, hi), periodic_aggregate=True)`` -- preprocess_aggregate / aggregate_neighbors
on the neighbour lists of the torus (pigs_amd/csrc/aggregate.hip, the PER instantiations).

The definition is the repository's own aggregation definition (oracle/aggregate_torch.py) applied to the 9N images of
pigs_periodic_images, rows of block 0, so the dense checker needs no change: it runs in float64 on the CPU on the
wrapped 9N image arrays with features, queries and keys repeated 9 times, and autograd through the repeat folds the
gradients.  Checked: (1) the kernels against that checker, output and all six gradients, float64 and float32, on a
lattice that fills the box and on a wide case in which a Gaussian is met through two images and a row is longer than
N; (2) invariance under a translation of all means round the torus (which the non-periodic lists do not have);
(3) agreement with the non-periodic path when no ellipse reaches the seam; (4) the grid build (N = 2 500) against the
existing non-periodic kernels on the 9N image arrays; (5) both hosts, gradcheck, overflow and argument errors.
"""
import math

import pytest
import torch

from oracle import aggregate_torch

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
PERIOD = HI - LO
# (kx, ky) of image block k, the block order of pigs_periodic_images (include/pigs_amd.h)
SHIFTS = ((0, 0), (-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
NAMES = ("features", "transform", "queries", "keys", "frequencies", "distance_transform")
HOSTS = ("native", "ctypes")


def lattice(n_side, seed=0, sigma=(0.06, 0.10), scale=1.0, box=None):
    """A jittered n_side x n_side lattice that fills [-1, 1)^2, float64 on the CPU: means [N, 2], conics [N, 3].
    ``sigma`` is the range of the standard deviations at n_side = 8 (it shrinks with the cell); ``scale`` < 1 pulls
    all means towards the middle of the box.  ``box`` = (lo, hi): the same lattice moved by x -> lo + (x + 1) a,
    a = (hi - lo) / 2 (conics / a^2)."""
    g = torch.Generator().manual_seed(seed)
    N = n_side * n_side
    cell = PERIOD / n_side
    t = LO + (torch.arange(n_side, dtype=torch.float64) + 0.5) * cell
    gx, gy = torch.meshgrid((t, t), indexing="ij")
    means = torch.stack((gx, gy), dim=-1).reshape(N, 2) + (torch.rand((N, 2), generator=g, dtype=torch.float64) - 0.5) * 0.7 * cell
    sd = (sigma[0] + (sigma[1] - sigma[0]) * torch.rand((N, 2), generator=g, dtype=torch.float64)) * (8.0 / n_side)
    rho = torch.tanh(torch.randn(N, generator=g, dtype=torch.float64) * 0.5) * 0.5
    sxx, syy, sxy = sd[:, 0] ** 2, sd[:, 1] ** 2, rho * sd[:, 0] * sd[:, 1]
    det = sxx * syy - sxy * sxy
    conics = torch.stack((syy / det, -sxy / det, sxx / det), dim=-1)
    if box is not None:
        from test_aggregate_matrix_gpu import to_box
        return to_box(means * scale, conics, box)
    return means * scale, conics


def arguments(N, L, K, F, dtype, seed=1, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    E = 4 * F + 1
    shapes = [(N, L), (L, L), (N, K), (N, K), (F,), (L, 2 * E)]
    args = [torch.rand(s, generator=g, dtype=torch.float64) for s in shapes]
    args[4] = torch.randn(F, generator=g, dtype=torch.float64) * 10
    return [a.to(dtype).to(device).requires_grad_(True) for a in args]


def image_indices(nb):
    """The image index k of every valid row entry (entries are j | k << 28)."""
    cap = nb.row_lists.shape[1]
    valid = torch.arange(cap)[None, :] < nb.row_counts.cpu()[:, None]
    return ((nb.row_lists.cpu().to(torch.int64) & 0xFFFFFFFF) >> 28)[valid]


def sampler_for(means, conics, q_max=36.0, periodic_aggregate=True, periodic=(LO, HI), **kw):
    from diff_gaussian_sampling import GaussianSampler
    kw.setdefault("backend", "dense")
    s = GaussianSampler(True, unpinned_aggregate=True, q_max=q_max, periodic=periodic,
                        periodic_aggregate=periodic_aggregate, **kw)
    values = torch.ones((means.shape[0], 1), dtype=means.dtype, device=means.device)
    s.preprocess(means, values, None, conics, means[:16].detach())
    s.preprocess_aggregate()
    return s


def run(s, args, r):
    out = s.aggregate_neighbors(*args)
    return [out.detach()] + [g.detach() for g in torch.autograd.grad((out * r).sum(), args)]


def images64(means, conics, lo=LO, period=PERIOD):
    """The wrapped 9N image system in float64 on the CPU, from the (rounded) inputs."""
    m = means.detach().double().cpu()
    m = lo + torch.remainder(m - lo, period)
    sh = torch.tensor(SHIFTS, dtype=torch.float64) * period
    return (m[None] + sh[:, None, :]).reshape(-1, 2), conics.detach().double().cpu().repeat(9, 1)


def checker(means, conics, args, r, q_max, lo=LO, period=PERIOD):
    """The dense checker on the 9N images, rows of block 0: [out, six gradients], the mask [N, 9N] and q - q_max of
    every (row of block 0, image) pair."""
    N = means.shape[0]
    m9, c9 = images64(means, conics, lo, period)
    a64 = [a.detach().double().cpu().requires_grad_(True) for a in args]
    f, tr, q, k, fr, dist = a64
    mask, delta, g = aggregate_torch.neighbor_structure(m9, c9, q_max)
    exp = aggregate_torch.aggregate(mask, delta, g, f.repeat(9, 1), tr, q.repeat(9, 1), k.repeat(9, 1), fr, dist)[:N]
    grads = torch.autograd.grad((exp * r.double().cpu()).sum(), a64)
    margin = (-2.0 * torch.log(g[:N]) - q_max).abs().min()
    return [exp.detach()] + [x.detach() for x in grads], mask[:N], float(margin)


def rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def errors(got, want):
    return {name: rel(a, b) for name, a, b in zip(("out",) + NAMES, got, want)}


def assert_within(err, tol):
    """The bars of tests/test_aggregate_gpu.py against the checker: ``tol``, frequencies x 10."""
    for name, e in err.items():
        assert e < tol * (10 if name == "frequencies" else 1), (name, e, err)


def assert_all_below(err, tol):
    """Every figure, the frequencies gradient included, against the same bar."""
    for name, e in err.items():
        assert e < tol, (name, e, err)


@pytest.mark.parametrize("case,dtype,tol", [("lattice", torch.float64, 1e-11), ("lattice", torch.float32, 2e-5),
                                            ("wide", torch.float64, 1e-11), ("wide", torch.float32, 2e-5)])
def test_kernels_match_dense_checker_on_the_images(hip_lib, case, dtype, tol):
    """The bars are those of tests/test_aggregate_gpu.py for such shapes."""
    n_side, L, K, F = 8, 4, 4, 3
    N = n_side * n_side
    m64, c64 = lattice(n_side, seed=3)
    q_max = 36.0
    if case == "wide":            # half extents between L/2 and L at q = 44: largest sqrt(44) * 0.25 = 1.66 < 2
        c64 = c64 / 2.5 ** 2
        q_max = 44.0
    means, conics = m64.to(dtype).cuda(), c64.to(dtype).cuda()
    args = arguments(N, L, K, F, dtype)
    r = torch.randn((N, L), dtype=dtype, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    want, mask, margin = checker(means, conics, args, r, q_max)
    # the checker's relation really is periodic: rows that meet a neighbour through an image ...
    per_image = mask.reshape(N, 9, N)
    assert int(per_image[:, 1:].any(dim=(1, 2)).sum()) > N // 4
    if case == "wide":            # ... a Gaussian met through two images, and a row longer than N
        assert int((per_image.sum(1) >= 2).any(1).sum()) > 0
        assert int(mask.sum(1).max()) > N
    # no pair close enough to the cut-off to flip in the kernels' arithmetic (float32: q ~ 40 from offsets and a
    # wrap rounded to 1e-7 relative is good to ~1e-4)
    assert margin > (1e-6 if dtype == torch.float64 else 2e-3), margin
    s = sampler_for(means, conics, q_max=q_max)
    nb = s._neighbors
    assert int(nb.overflow.item()) == 0
    assert int(nb.row_counts.sum()) == int(mask.sum()) == int(nb.col_counts.sum())
    assert torch.equal(nb.row_counts.cpu().long(), mask.sum(1))
    err = errors(run(s, args, r), want)
    print(f"periodic aggregate {case} {dtype}: cap {nb.cap}, pairs {int(mask.sum())}, margin {margin:.3g}, errors {err}")
    if dtype == torch.float32:    # the non-periodic path's error on the same inputs, for comparison
        mask0, delta0, g0 = aggregate_torch.neighbor_structure(means.double().cpu(), conics.double().cpu(), q_max)
        a64 = [a.detach().double().cpu().requires_grad_(True) for a in args]
        exp0 = aggregate_torch.aggregate(mask0, delta0, g0, *a64)
        want0 = [exp0.detach()] + list(torch.autograd.grad((exp0 * r.double().cpu()).sum(), a64))
        err0 = errors(run(sampler_for(means, conics, q_max=q_max, periodic_aggregate=False), args, r), want0)
        print(f"non-periodic lists, same inputs: errors {err0}")
    assert_within(err, tol)


def wrapped(means):
    return LO + torch.remainder(means - LO, PERIOD)


def test_translation_round_the_torus_changes_nothing(hip_lib):
    """The translated configuration goes to the periodic lists as it is (the sampler wraps it); the non-periodic lists
    get it wrapped into the box, as the reference's model holds its means (model_pn.py:689-693) -- an unwrapped
    translation would leave them unchanged trivially."""
    n_side, L, K, F = 8, 4, 4, 3
    N = n_side * n_side
    m64, c64 = lattice(n_side, seed=3)
    conics = c64.cuda()
    args = arguments(N, L, K, F, torch.float64)
    r = torch.randn((N, L), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    base = run(sampler_for(m64.cuda(), conics), args, r)
    base_plain = run(sampler_for(m64.cuda(), conics, periodic_aggregate=False), args, r)
    scale = float(base[0].abs().max())
    moved_plain = 0.0
    for shift in ((0.37, -0.81), (1.0, 1.0), (0.123, 0.0)):
        means = (m64 + torch.tensor(shift, dtype=torch.float64)).cuda()
        _, _, margin = checker(means, conics, args, r, 36.0)
        assert margin > 1e-6, (shift, margin)          # no neighbour can flip
        got = run(sampler_for(means, conics), args, r)
        err = errors(got, base)
        print(f"shift {shift}: periodic lists move by {err}")
        assert_all_below(err, 1e-10)
        plain = run(sampler_for(wrapped(means), conics, periodic_aggregate=False), args, r)
        moved_plain = max(moved_plain, float((plain[0] - base_plain[0]).abs().max()) / scale)
    # the non-periodic lists on the same periodic sampler are not invariant
    assert moved_plain > 1e-2, moved_plain


def test_interior_configuration_equals_the_non_periodic_lists(hip_lib):
    n_side, L, K, F = 8, 4, 4, 3
    N = n_side * n_side
    m64, c64 = lattice(n_side, seed=3, scale=0.2)      # means within 0.2 of the middle, half extents <= 0.6: nothing reaches the seam
    means, conics = m64.cuda(), c64.cuda()
    _, mask, _ = checker(means, conics, arguments(N, L, K, F, torch.float64),
                         torch.zeros((N, L), dtype=torch.float64), 36.0)
    assert not mask.reshape(N, 9, N)[:, 1:].any()
    args = arguments(N, L, K, F, torch.float64)
    r = torch.randn((N, L), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    a = run(sampler_for(means, conics), args, r)
    b = run(sampler_for(means, conics, periodic_aggregate=False), args, r)
    assert_all_below(errors(a, b), 1e-10)


def test_grid_build_matches_the_plain_kernels_on_the_images(hip_lib):
    """N = 2 500 > 2 048: the lists come from the walk of the grid of the wrapped centres, once per shift.  The dense
    checker is out of reach; the comparison runs through the existing non-periodic kernels on the 9N image arrays
    (22 500 Gaussians, also sparse), arguments repeated, rows of block 0."""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.host_ctypes import periodic_images_raw
    n_side, L, K, F = 50, 4, 4, 3
    N = n_side * n_side
    m64, c64 = lattice(n_side, seed=7)
    means, conics = (m64 + 0.31).cuda(), c64.cuda()    # part of the means start outside the box
    args = arguments(N, L, K, F, torch.float64)
    r = torch.randn((N, L), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    s = sampler_for(means, conics)
    got = run(s, args, r)
    nb = s._neighbors
    assert int(nb.overflow.item()) == 0
    pairs = int(nb.row_counts.sum())
    assert pairs == int(nb.col_counts.sum())

    values = torch.ones((N, 1), dtype=torch.float64, device="cuda")
    img_m, img_v, img_c = periodic_images_raw(means, values, conics, LO, PERIOD, 44.0)
    plain = GaussianSampler(True, unpinned_aggregate=True, backend="dense")
    plain.preprocess(img_m, img_v, None, img_c, img_m[:16])
    plain.preprocess_aggregate()
    f, tr, q, k, fr, dist = args
    out = plain.aggregate_neighbors(f.repeat(9, 1), tr, q.repeat(9, 1), k.repeat(9, 1), fr, dist)[:N]
    want = [out.detach()] + list(torch.autograd.grad((out * r).sum(), args))
    assert int(plain._neighbors.row_counts[:N].sum()) == pairs
    k_used = image_indices(nb)
    assert int(k_used.max()) <= 8 and int((k_used != 0).sum()) > 0
    err = errors(got, want)
    print(f"grid build N={N}: cap {nb.cap}, pairs {pairs}, errors {err}")
    assert_all_below(err, 1e-10)


def test_hosts_agree(hip_lib):
    n_side, L, K, F = 12, 8, 4, 3
    N = n_side * n_side
    m64, c64 = lattice(n_side, seed=11)
    means, conics = m64.float().cuda(), c64.float().cuda()
    args = arguments(N, L, K, F, torch.float32)
    r = torch.randn((N, L), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    res, pairs = {}, {}
    for host in HOSTS:
        s = sampler_for(means, conics, host=host)
        res[host] = run(s, args, r)
        nb = s._neighbors
        assert int(nb.overflow.item()) == 0 and int(nb.row_counts.max()) <= nb.cap
        pairs[host] = int(nb.row_counts.sum())
        assert int(nb.col_counts.sum()) == pairs[host]
    assert pairs["native"] == pairs["ctypes"]
    for a, b in zip(res["native"], res["ctypes"]):
        assert rel(a, b) < 2e-5


@pytest.mark.parametrize("host", HOSTS)
def test_gradcheck_all_six_arguments_float64(hip_lib, host):
    m64, c64 = lattice(5, seed=2)
    s = sampler_for(m64.cuda(), c64.cuda(), host=host)
    nb = s._neighbors
    assert int(nb.row_counts.sum()) == int(nb.col_counts.sum())
    assert int((image_indices(nb) != 0).sum()) > 0        # the lists are periodic ones
    args = arguments(25, 2, 4, 2, torch.float64)
    assert torch.autograd.gradcheck(lambda *a: s.aggregate_neighbors(*a), args)


@pytest.mark.parametrize("host", HOSTS)
def test_too_small_cap_raises_in_debug_mode(hip_lib, host):
    m64, c64 = lattice(8, seed=3)
    from pigs_amd._lib import PigsError          # both hosts raise it (the native one through its translator)
    with pytest.raises(PigsError, match="truncated"):
        sampler_for(m64.cuda(), c64.cuda(), host=host, aggregate_cap=4)


@pytest.mark.parametrize("host", HOSTS)
def test_periodic_aggregate_needs_periodic(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    with pytest.raises(ValueError, match="periodic"):
        GaussianSampler(True, unpinned_aggregate=True, host=host, periodic_aggregate=True)
    s = GaussianSampler(True, unpinned_aggregate=True, host=host, periodic=(LO, HI), periodic_aggregate=True)
    assert s.periodic_aggregate is True
    with pytest.raises(ValueError, match="periodic"):
        s.periodic = None
