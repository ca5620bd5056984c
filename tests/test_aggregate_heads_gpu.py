"""GPU: GaussianSampler.aggregate_neighbors_heads -- all H attention heads of a layer in one launch
(pigs_amd/csrc/aggregate.hip, the aggregate_heads_* kernels) -- against the checkers of aggregate_neighbors run once per
head and stacked: out[:, h] = aggregate_neighbors(features, transforms[h], queries[:, h], keys[:, h], frequencies,
distance_transforms[h]).  Autograd through the stack gives the checker's gradients in the arguments' shapes, d features
and d frequencies summed over the heads.

Bars (relative to the largest entry, the frequency gradient x 10), those of tests/test_aggregate_gpu.py: float64 1e-11
(1e-10 at the model's shape at N = 1 600), float32 2e-5 (5e-5 at the model's shape L = K = 16, F = 6).  The float64
checkers run on the CPU, as they do there.

(1) the reference test's shape (N = 25, L = 2, K = 4, F = 5) with H = 2, 3, 4 against the dense checker;
(2) the model's shape (L = K = 16, F = 6, H = 2) at N = 144 and 1 600 against the sparse checker on the pair list read
    back from the built lists;
(3) (1) with head 1's queries x 30 and, float64, x 1000 (beyond the range of exp: the case that catches a shared
    running maximum): a softmax state per head;
(4) the crowded scene of tests/test_aggregate_matrix_gpu.py at N = 2 049 / 4 097 / 8 193: four, two and one waves per
    Gaussian, second rounds and idle waves, the split sums over N;
(5) the lists of the torus against the dense checker on the 9N images;
(6) gradcheck; (7) H = 1 is aggregate_neighbors; (8) both hosts; (9) errors.
"""
import functools
import math

import pytest
import torch

from oracle import aggregate_sparse as sparse
from oracle import aggregate_torch as dense

pytestmark = pytest.mark.gpu

NAMES = ("features", "transforms", "queries", "keys", "frequencies", "distance_transforms")
HOSTS = ("native", "ctypes")
DTYPES = {"float32": torch.float32, "float64": torch.float64}


def head_arguments(N, H, L, K, F, seed=1):
    """The six arguments in float64 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    E = 4 * F + 1
    args = [torch.rand(s, generator=g, dtype=torch.float64) for s in [(N, L), (H, L, L), (N, H, K), (N, H, K), (F,), (H, L, 2 * E)]]
    args[4] = torch.randn(F, generator=g, dtype=torch.float64) * 10
    return args


def on_gpu(a64, dtype):
    return [a.to(dtype).cuda().requires_grad_(True) for a in a64]


def weights(N, H, L, dtype):
    return torch.randn((N, H, L), generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(dtype)


def per_head(single, a64):
    """The checker ``single(features, transform, queries, keys, frequencies, distance_transform)`` per head, stacked."""
    f, tr, q, k, fr, dist = a64
    return torch.stack([single(f, tr[h], q[:, h], k[:, h], fr, dist[h]) for h in range(q.shape[1])], dim=1)


def run(call, args, r):
    out = call(*args)
    return [out.detach()] + [g.detach() for g in torch.autograd.grad((out * r.to(out.device)).sum(), args)]


def expected(single, args, r):
    """[out, six gradients] of the stacked checker in float64 on the CPU, on the (rounded) inputs of the kernels."""
    a64 = [a.detach().double().cpu().requires_grad_(True) for a in args]
    want = per_head(single, a64)
    return [want.detach()] + [g.detach() for g in torch.autograd.grad((want * r.double().cpu()).sum(), a64)]


def rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def assert_within(got, want, tol, what):
    err = {}
    for name, a, b in zip(("out",) + NAMES, got, want):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err[name] = rel(a, b)
    print(f"{what}: bar {tol:g}, errors " + ", ".join(f"{n} {e:.2g}" for n, e in err.items()))
    for name, e in err.items():
        assert e < tol * (10 if name == "frequencies" else 1), (what, name, e, err)


def sampler_on(means, conics, **kw):
    from diff_gaussian_sampling import GaussianSampler
    kw.setdefault("backend", "dense")
    s = GaussianSampler(True, unpinned_aggregate=True, **kw)
    s.preprocess(means, torch.ones((means.shape[0], 1), dtype=means.dtype, device=means.device), None, conics, means[:16].detach())
    s.preprocess_aggregate()
    return s


# ---- (1), (3): the reference test's shape against the dense checker
@functools.lru_cache(maxsize=None)
def small_scene(dtype):
    from test_aggregate_gpu import gaussians
    means, _, conics = gaussians(5, DTYPES[dtype], spread=2.0)
    mask, delta, g = dense.neighbor_structure(means.double().cpu(), conics.double().cpu(), 36.0)
    assert mask.sum(1).max() > 1 and not mask.all()
    return means, conics, (mask, delta, g)


def check_small(dtype, H, tol, scale_head_1=1.0):
    means, conics, nb = small_scene(dtype)
    N, L, K, F = 25, 2, 4, 5
    a64 = head_arguments(N, H, L, K, F)
    a64[2][:, 1] *= scale_head_1
    args = on_gpu(a64, DTYPES[dtype])
    r = weights(N, H, L, DTYPES[dtype])
    s = sampler_on(means, conics)
    got = run(s.aggregate_neighbors_heads, args, r)
    assert got[0].shape == (N, H, L) and got[0].dtype == DTYPES[dtype]
    want = expected(lambda *a: dense.aggregate(*nb, *a), args, r)
    assert_within(got, want, tol, f"heads N={N} H={H} {dtype} queries[:, 1] x {scale_head_1:g}")
    return args


@pytest.mark.parametrize("H", [2, 3, 4])
@pytest.mark.parametrize("dtype,tol", [("float64", 1e-11), ("float32", 2e-5)])
def test_reference_shape_many_heads(hip_lib, dtype, tol, H):
    check_small(dtype, H, tol)


@pytest.mark.parametrize("dtype,tol,scale", [("float64", 1e-11, 30.0), ("float32", 2e-5, 30.0), ("float64", 1e-11, 1000.0)])
def test_softmax_state_is_per_head(hip_lib, dtype, tol, scale):
    """Head 1's scores are ``scale`` times head 0's.  With a running maximum shared between the heads, head 0's weights
    would be exp(s - m) with m from head 1.  At x 30 (scores up to ~60) that is ~e^-58, representable in float32 and in
    float64, and the normalised result is still right to the bar: those two cases check the arithmetic at widely
    different scales but cannot catch a shared maximum.  The float64 x 1000 case does (exp(s - m) is below the smallest
    double: 0 / 0).  A float32 scale large enough to underflow would put the float32 rounding of head 1's own scores
    (~|s| 2^-23) beyond the 2e-5 bar, so the float32 instantiation is covered only in as much as it is the same
    template, per-head arrays included."""
    args = check_small(dtype, 2, tol, scale_head_1=scale)
    q, k = args[2].detach().double(), args[3].detach().double()
    top = [float((q[:, h] @ k[:, h].t()).max()) / 2.0 for h in range(2)]        # / sqrt(K), an upper bound of the row maxima
    assert top[1] > 10 * top[0]


# ---- (2): the model's shape against the sparse checker on the built lists' pairs
def pairs_of(nb, N):
    from test_aggregate_matrix_gpu import list_keys
    rows = list_keys(nb.row_counts, nb.row_lists, N, N, False, False).sort().values
    cols = list_keys(nb.col_counts, nb.col_lists, N, N, False, True).sort().values
    assert torch.equal(rows, cols) and int(nb.overflow.item()) == 0
    return rows // N, rows % N


def check_on_lists(nb, means, conics, dtype, H, L, K, F, tol, what):
    from pigs_amd import aggregate as A
    N = means.shape[0]
    I, J = pairs_of(nb, N)
    args = on_gpu(head_arguments(N, H, L, K, F), DTYPES[dtype])
    r = weights(N, H, L, DTYPES[dtype])
    got = run(lambda *a: A.aggregate_heads(nb, *a), args, r)
    m64, c64 = means.double().cpu(), conics.double().cpu()
    want = expected(lambda *a: sparse.aggregate(N, I, J, m64, c64, *a), args, r)
    assert_within(got, want, tol, f"{what} N={N} H={H} L={L} K={K} F={F} {dtype}, {I.numel()} pairs")


@pytest.mark.parametrize("n_side,dtype,tol", [(12, "float64", 1e-11), (12, "float32", 5e-5), (40, "float64", 1e-10),
                                              (40, "float32", 5e-5)])
def test_model_shape(hip_lib, n_side, dtype, tol):
    from pigs_amd.aggregate import NeighborLists
    from test_aggregate_gpu import gaussians
    means, _, conics = gaussians(n_side, DTYPES[dtype], spread=2.0)
    nb = NeighborLists(means, conics, 36.0)
    check_on_lists(nb, means, conics, dtype, 2, 16, 16, 6, tol, "model shape")


# ---- (4): second rounds and idle waves, one / two / four waves per Gaussian, split sums
@pytest.mark.parametrize("dtype,N,tol", [("float32", 2049, 2e-5), ("float32", 4097, 2e-5), ("float32", 8193, 2e-5),
                                         ("float64", 2049, 1e-11)])
def test_crowded_scene_launch_variants(hip_lib, dtype, N, tol):
    import test_aggregate_matrix_gpu as G
    means, conics = G.inputs(dtype, "spread", N)
    nb = G.build_lists(dtype, "spread", N)
    wpg = 4 if N <= 4096 else 2 if N <= 8192 else 1
    for counts in (nb.row_counts.cpu(), nb.col_counts.cpu()):
        assert int(counts.max()) > 64 * (2 * wpg - 1) and int(counts.min()) < 64, (int(counts.min()), int(counts.max()))
    check_on_lists(nb, means, conics, dtype, 2, 16, 16, 2, tol, "crowded scene")


# ---- (5): the torus
@pytest.mark.parametrize("dtype,tol", [("float64", 1e-11), ("float32", 2e-5)])
def test_torus_lists(hip_lib, dtype, tol):
    from test_periodic_aggregate_gpu import LO, HI, images64, lattice
    n_side, H, L, K, F = 8, 2, 4, 4, 3
    N = n_side * n_side
    m64, c64 = lattice(n_side, seed=3)
    means, conics = m64.to(DTYPES[dtype]).cuda(), c64.to(DTYPES[dtype]).cuda()
    m9, c9 = images64(means, conics)
    mask, delta, g = dense.neighbor_structure(m9, c9, 36.0)
    assert int(mask[:N].reshape(N, 9, N)[:, 1:].any(dim=(1, 2)).sum()) > N // 4          # rows that reach through an image
    assert float((-2.0 * torch.log(g[:N]) - 36.0).abs().min()) > (1e-6 if dtype == "float64" else 2e-3)

    def single(f, tr, q, k, fr, dist):
        return dense.aggregate(mask, delta, g, f.repeat(9, 1), tr, q.repeat(9, 1), k.repeat(9, 1), fr, dist)[:N]
    args = on_gpu(head_arguments(N, H, L, K, F), DTYPES[dtype])
    r = weights(N, H, L, DTYPES[dtype])
    s = sampler_on(means, conics, periodic=(LO, HI), periodic_aggregate=True)
    got = run(s.aggregate_neighbors_heads, args, r)
    assert_within(got, expected(single, args, r), tol, f"torus N={N} H={H} {dtype}")


# ---- (6), (7)
def test_gradcheck_all_six_arguments_float64(hip_lib):
    means, conics, _ = small_scene("float64")
    s = sampler_on(means, conics)
    args = on_gpu(head_arguments(25, 2, 2, 4, 5), torch.float64)
    assert torch.autograd.gradcheck(lambda *a: s.aggregate_neighbors_heads(*a), args)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_head_is_aggregate_neighbors(hip_lib, dtype, host):
    means, conics, _ = small_scene(dtype)
    s = sampler_on(means, conics, host=host)
    args = on_gpu(head_arguments(25, 1, 2, 4, 5), DTYPES[dtype])
    r = weights(25, 1, 2, DTYPES[dtype])
    got = run(s.aggregate_neighbors_heads, args, r)
    f, tr, q, k, fr, dist = args
    want = run(lambda *a: s.aggregate_neighbors(f, tr[0], q[:, 0], k[:, 0], fr, dist[0])[:, None], args, r)
    assert got[0].shape == (25, 1, 2)
    for name, a, b in zip(("out",) + NAMES, got, want):
        assert a.shape == b.shape and torch.equal(a, b), name


# ---- (8): both hosts
def cloud(N, dtype, seed=3):
    """N centres over [-1, 1)^2 with standard deviations around 1.15 * 2 / sqrt(N) (rows of ~ 100 entries)."""
    g = torch.Generator().manual_seed(seed)
    means = torch.rand((N, 2), generator=g, dtype=torch.float64) * 2 - 1
    sd = 1.15 * 2 / math.sqrt(N) * torch.exp(torch.randn((N, 2), generator=g, dtype=torch.float64) * 0.3)
    rho = torch.tanh(torch.randn(N, generator=g, dtype=torch.float64) * 0.5) * 0.5
    sxx, syy, sxy = sd[:, 0] ** 2, sd[:, 1] ** 2, rho * sd[:, 0] * sd[:, 1]
    det = sxx * syy - sxy * sxy
    return means.to(dtype).cuda(), torch.stack((syy / det, -sxy / det, sxx / det), dim=-1).to(dtype).cuda()


@pytest.mark.parametrize("N", [144, 3000])
def test_hosts_agree(hip_lib, N):
    """The model's shape in float32 (bar 5e-5); N = 3 000 builds the lists through the grid, whose order -- and with it
    the last bits -- may differ between two builds."""
    H, L, K, F = 2, 16, 16, 6
    means, conics = cloud(N, torch.float32)
    args = on_gpu(head_arguments(N, H, L, K, F), torch.float32)
    r = weights(N, H, L, torch.float32)
    res = {host: run(sampler_on(means, conics, host=host).aggregate_neighbors_heads, args, r) for host in HOSTS}
    assert_within(res["native"], res["ctypes"], 5e-5, f"hosts N={N}")
    assert float(res["ctypes"][0].abs().max()) > 0


# ---- (9): errors
@pytest.mark.parametrize("host", HOSTS)
def test_errors(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    means, conics, _ = small_scene("float64")
    N, H, L, K, F = 25, 2, 2, 4, 5
    a64 = head_arguments(N, H, L, K, F)
    args = on_gpu(a64, torch.float64)
    fresh = GaussianSampler(True, unpinned_aggregate=True, host=host, backend="dense")
    fresh.preprocess(means, torch.ones((N, 1), dtype=means.dtype, device="cuda"), None, conics, means[:16])
    with pytest.raises(RuntimeError, match="preprocess_aggregate"):
        fresh.aggregate_neighbors_heads(*args)
    s = sampler_on(means, conics, host=host)
    f, tr, q, k, fr, dist = args
    for bad in ((f[:-1], tr, q, k, fr, dist), (f, tr[0], q, k, fr, dist), (f, tr, q[:, 0], k[:, 0], fr, dist),
                (f, tr, q, k[:, :1], fr, dist), (f, tr, q, k, fr, dist[:, :, :-1]), (f, tr[:1], q, k, fr, dist),
                (f, tr, q, k, fr[None], dist)):
        with pytest.raises(ValueError):
            s.aggregate_neighbors_heads(*bad)
    for x in range(6):
        moved = [a.detach().cpu() if y == x else a for y, a in enumerate(args)]
        with pytest.raises(RuntimeError, match="GPU only"):
            s.aggregate_neighbors_heads(*moved)
    # refused shapes: the message names the limit and what remains available (that the C entries refuse them before any
    # HIP call is tests/test_aggregate_heads.py's business)
    for Hb, Lb, Kb, Fb, limit in ((4, 16, 16, 6, "163840"), (3, 16, 16, 6, "163840"), (4, 20, 16, 2, "128"), (5, 2, 4, 5, "<= 4")):
        wide = on_gpu(head_arguments(N, Hb, Lb, Kb, Fb), torch.float64)
        with pytest.raises(NotImplementedError, match=limit) as e:
            s.aggregate_neighbors_heads(*wide)
        assert "separate aggregate_neighbors calls remain available" in str(e.value)
    # float32 inputs on float64 lists are cast, the result and the gradients come back in the arguments' dtypes
    a32 = on_gpu(a64, torch.float32)
    out = s.aggregate_neighbors_heads(*a32)
    assert out.dtype == torch.float32
    grads = torch.autograd.grad(out.sum(), a32)
    assert all(g.dtype == torch.float32 and g.shape == a.shape for g, a in zip(grads, a32))
    # a saved tensor modified in place before the backward
    out = s.aggregate_neighbors_heads(*args)
    with torch.no_grad():
        args[2].mul_(2.0)
    with pytest.raises(RuntimeError, match="modified"):
        out.sum().backward()
