"""GPU: the neighbour lists of the torus and the sampling kernels on them (``periodic_aggregate=True``) on boxes other
than (-1, 1): DESIGN.md section 11, "Boxes".  Every problem is one of tests/test_aggregate_matrix_gpu.py or
tests/test_periodic_aggregate_gpu.py moved by x -> lo + (x + 1) a, a = (hi - lo) / 2 (means mapped, conics / a^2,
frequencies / a); the expectation is the float64 checker run on the mapped inputs with the box as the kernel's dtype
holds it (float32: float32(lo), float32(hi - lo)).  tests/test_periodic_boxes.py shows without a device that the
checkers do not see the map and that no list case leaves pairs to rounding.

(1) lists against the brute-force relation (check_lists: no sure pair missed, no sure-out pair stored, rows = columns
    transposed, no overflow, the cap rule), grid build and all-pairs build, with the level-mask assertions;
(2) numerics through the sampler on both hosts: (a) the 8 x 8 lattice and its wide variant against the dense checker on
    the images, as they are and with ten centres planted on the seams, (b) N = 2 500 against the sparse checker, four
    centres planted, (c) aggregate_neighbors_heads;
(3) translation round the torus; (4) gradcheck round a corner.
Bars: those of the (-1, 1) tests, unchanged.

Measured on an MI355X (79 tests, 34 s): no band pair in any list case, no pair missed or too many, centres on hi included; worst error in units of
its bar 0.089 (box C, wide lattice with planted centres, float32), float64 below 1e-3 of its bars.  With ``blo = -bhi`` in aggregate_lists_kernel
(a scratch build) the six list cases of box D fail on missed pairs and every (-1, 1) test passes.
"""
import pytest
import torch

import test_aggregate_matrix_gpu as G
import test_periodic_aggregate_gpu as P
from oracle import aggregate_sparse as sparse
from oracle import aggregate_torch
from test_periodic_boxes import BOXES, LIST_CASES

pytestmark = pytest.mark.gpu
HOSTS = ("native", "ctypes")
DTYPES = G.DTYPES



def half(box):
    return (box[1] - box[0]) / 2.0


def plant_on_the_seams(m64, n_side, box, dtype):
    """Ten centres of the n_side x n_side lattice moved onto the seams, in ``dtype``: x exactly lo, one representable
    number above and below it (first lattice column), x exactly hi and its two neighbours (last column), and y = lo,
    y = hi, nextafter(lo, -inf), nextafter(hi, +inf) in the first and last rows.  pigs_periodic_images puts a mean
    just below lo onto hi, so block 0 -- the centres the lists are built from -- holds centres ON hi as well as on lo."""
    lo, period = G.lo_period_as_held(box, "float32" if dtype == torch.float32 else "float64")
    lo, hi = torch.tensor(lo, dtype=dtype), torch.tensor(lo + period, dtype=dtype)
    up, down = torch.tensor(float("inf"), dtype=dtype), torch.tensor(float("-inf"), dtype=dtype)
    m = m64.clone()
    last = n_side - 1
    for iy, v in enumerate((lo, torch.nextafter(lo, up), torch.nextafter(lo, down))):
        m[0 * n_side + iy + 1, 0] = v.double()
    for iy, v in enumerate((hi, torch.nextafter(hi, down), torch.nextafter(hi, up))):
        m[last * n_side + iy + 1, 0] = v.double()
    for ix, v in zip((2, 3), (lo, torch.nextafter(lo, down))):
        m[ix * n_side + 0, 1] = v.double()
    for ix, v in zip((4, 5), (hi, torch.nextafter(hi, up))):
        m[ix * n_side + last, 1] = v.double()
    return m


# ---- (1)
@pytest.mark.parametrize("name,dtype,gen,N", LIST_CASES)
def test_lists_match_the_brute_force_on_the_box(hip_lib, name, dtype, gen, N):
    box = BOXES[name]
    rel = G.relation(dtype, gen, N, box)
    assert rel.band_fraction <= G.BAND_CAP[dtype], (rel.band.numel(), rel.sure.numel())
    assert rel.images_used
    if gen == "torus_small" and name in ("A", "D"):          # sure pairs through images across both seams
        assert rel.images_seen & {4, 5} and rel.images_seen & {2, 7}, rel.images_seen
    nb = G.build_lists(dtype, gen, N, box=box)
    rows = G.check_lists(nb, rel, dtype)
    used = set(((rows % rel.M) // N).unique().tolist())
    assert used >= rel.images_seen and used != {0}              # every image of the relation is in the lists
    if N > 2048:
        mask, levels = G.occupied_levels(hip_lib, nb, dtype, N)
        assert 0 < mask < 1 << levels
        if gen == "torus_small":
            assert mask == 1                                    # the finest level alone: the reach cull is active
        if gen == "torus_wide":
            assert mask >> (levels - 1) == 1                    # the top level occupied: the reach unbounded
        if gen == "torus":
            assert mask >> (levels - 1) == 0
    longest = int(max(nb.row_counts.max(), nb.col_counts.max()))
    assert nb.cap == max(64, (longest + 63) // 64 * 64)
    print(f"box {name} lists {gen} N={N} {dtype}: pairs {rel.sure.numel()}, band {rel.band.numel()}, cap {nb.cap}, "
          f"images {sorted(used)}")


# ---- (2a)
@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("case,dtype,tol", [("lattice", torch.float64, 1e-11), ("lattice", torch.float32, 2e-5),
                                            ("wide", torch.float64, 1e-11), ("wide", torch.float32, 2e-5)])
@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("name", ["B", "C"])
def test_kernels_match_the_dense_checker_on_the_box(hip_lib, name, planted, case, dtype, tol, host):
    box = BOXES[name]
    a = half(box)
    n_side, L, K, F = 8, 4, 4, 3
    N = n_side * n_side
    m64, c64 = P.lattice(n_side, seed=3, box=box)
    if planted:
        m64 = plant_on_the_seams(m64, n_side, box, dtype)
    q_max = 36.0
    if case == "wide":            # half extents between L/2 and L at q = 44, as on (-1, 1)
        c64 = c64 / 2.5 ** 2
        q_max = 44.0
    means, conics = m64.to(dtype).cuda(), c64.to(dtype).cuda()
    args = P.arguments(N, L, K, F, dtype)
    with torch.no_grad():
        args[4].div_(a)                                         # frequencies / a: the phases are those of (-1, 1)
    r = torch.randn((N, L), dtype=dtype, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    lo, period = G.lo_period_as_held(box, "float32" if dtype == torch.float32 else "float64")
    want, mask, margin = P.checker(means, conics, args, r, q_max, lo, period)
    per_image = mask.reshape(N, 9, N)
    assert int(per_image[:, 1:].any(dim=(1, 2)).sum()) > N // 4
    if case == "wide":
        assert int((per_image.sum(1) >= 2).any(1).sum()) > 0 and int(mask.sum(1).max()) > N
    assert margin > (1e-6 if dtype == torch.float64 else 2e-3), margin
    s = P.sampler_for(means, conics, q_max=q_max, periodic=box, host=host)
    nb = s._neighbors
    if planted:          # the lists are built from centres on both ends of the closed box
        b0 = s._inputs[0][:N].detach().double().cpu()
        assert float(b0.min()) == lo and float(b0.max()) == lo + period
    assert int(nb.overflow.item()) == 0
    assert int(nb.row_counts.sum()) == int(mask.sum()) == int(nb.col_counts.sum())
    assert torch.equal(nb.row_counts.cpu().long(), mask.sum(1))
    err = P.errors(P.run(s, args, r), want)
    print(f"box {name} periodic aggregate {case}{' planted' if planted else ''} {dtype} {host}: worst {max(err.values()) / tol:.3g} of the bar, errors {err}")
    P.assert_within(err, tol)


# ---- (2b), (2c): N = 2 500 (the grid build) on box C, through the sampler, against the sparse checker on the lists' pairs
def sampler_on_lists(dtype, host):
    """The sampler with its lists, the brute-force relation of the centres it bound (block 0 of its images: the wrap
    lo + ((mu - lo) mod L) may move a float32 centre by an ulp, and the lists are those of the moved ones) and the
    lists' pairs after check_lists.  The relation takes those centres as they are (wrap=False): one on hi meets its
    neighbours across the seam through other images k than one on lo, and the lists name k."""
    import types
    box = BOXES["C"]
    N = 2500
    means, conics = (x.clone() for x in G.inputs(dtype, "torus", N, box))
    lo, period = G.lo_period_as_held(box, dtype)
    # four centres on the seams: exactly lo, and one representable number below it, which the images kernel puts ON
    # hi -- the grid build (aggregate_lists_kernel, its culls against the box) gets centres on both ends of the closed box
    below = torch.nextafter(torch.tensor(lo, dtype=means.dtype), torch.tensor(float("-inf"), dtype=means.dtype))
    means[0, 0], means[1, 0], means[2, 1], means[3, 1] = below, lo, below, lo
    means, conics = means.cuda(), conics.cuda()
    s = P.sampler_for(means, conics, periodic=box, host=host)
    bound = s._inputs[0][:N].detach().cpu()
    moved = (bound - means.cpu()).abs()
    assert float(torch.minimum(moved, (moved - period).abs()).max()) <= 2 * torch.finfo(DTYPES[dtype]).eps * box[1]
    assert bool((bound >= lo).all() and (bound <= lo + period).all())
    assert float(bound[0, 0]) == float(bound[2, 1]) == lo + period and float(bound[1, 0]) == float(bound[3, 1]) == lo
    i, j, k, q, S = sparse.brute_pairs_periodic(bound, conics, G.Q_MAX, lo, period, wrap=False)
    sure, band = sparse.classify(q, S, G.Q_MAX, DTYPES[dtype])
    key = i * 9 * N + k * N + j
    rel = types.SimpleNamespace(N=N, M=9 * N, periodic=True, sure=key[sure].sort().values, band=key[band].sort().values,
                                bound=bound.double())
    rel.band_fraction = rel.band.numel() / max(1, rel.sure.numel())
    assert bool((k[sure] != 0).any())
    return s, rel, G.check_lists(s._neighbors, rel, dtype)


def sparse_single(dtype, rel, rows):
    """The checker of one head on the pairs of the lists: f(features, transform, queries, keys, frequencies, dist)."""
    N = rel.N
    conics = G.inputs(dtype, "torus", N, BOXES["C"])[1].double()
    m9, c9 = sparse.periodic_images(rel.bound, conics, *G.lo_period_as_held(BOXES["C"], dtype), wrap=False)
    I, col = rows // rel.M, rows % rel.M
    return lambda f, tr, q, k, fr, dist: sparse.aggregate(N, I, col, m9, c9, f.repeat(9, 1), tr, q, k.repeat(9, 1), fr, dist)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_grid_built_lists_through_the_sampling_kernels_on_box_c(hip_lib, dtype, host):
    N, L, K, F = 2500, 4, 1, 3
    s, rel, rows = sampler_on_lists(dtype, host)
    dt = DTYPES[dtype]
    a64 = [x.to(dt).double() for x in G.arguments(N, L, K, F)]
    a64[4] = (a64[4] / half(BOXES["C"])).to(dt).double()
    args = [x.to(dt).cuda().requires_grad_(True) for x in a64]
    r64 = G.randn(torch.Generator().manual_seed(5), N, L).to(dt).double()
    out = s.aggregate_neighbors(*args)
    grads = torch.autograd.grad((out * r64.to(dt).cuda()).sum(), args)
    for x in a64:
        x.requires_grad_(True)
    want = sparse_single(dtype, rel, rows)(*a64)
    wgrads = torch.autograd.grad((want * r64).sum(), a64)
    err = {"out": G.rel_err(out, want)}
    for n, got, w in zip(G.NAMES, grads, wgrads):
        assert got.shape == w.shape and got.dtype == dt
        err[n] = G.rel_err(got, w)
    print(f"box C aggregate torus N={N} {dtype} {host}: pairs {rows.numel()}, worst "
          f"{max(e / (10 if n == 'frequencies' else 1) for n, e in err.items()) / G.TOL[dtype]:.3g} of the bar, errors {err}")
    for n, e in err.items():
        assert e < G.TOL[dtype] * (10 if n == "frequencies" else 1), (n, e, err)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("dtype,tol", [("float64", 1e-11), ("float32", 2e-5)])
def test_heads_on_box_c(hip_lib, dtype, tol, H, host):
    """aggregate_neighbors_heads against H separate aggregate_neighbors calls (same lists, same kernels' arithmetic per
    head: the bar of tests/test_aggregate_heads_gpu.py against the checker serves for both) and against the dense
    checker on the images."""
    import test_aggregate_heads_gpu as A
    box = BOXES["C"]
    n_side, L, K, F = 8, 4, 4, 3
    N = n_side * n_side
    m64, c64 = P.lattice(n_side, seed=3, box=box)
    means, conics = m64.to(DTYPES[dtype]).cuda(), c64.to(DTYPES[dtype]).cuda()
    lo, period = G.lo_period_as_held(box, dtype)
    m9, c9 = P.images64(means, conics, lo, period)
    mask, delta, g = aggregate_torch.neighbor_structure(m9, c9, 36.0)
    assert int(mask[:N].reshape(N, 9, N)[:, 1:].any(dim=(1, 2)).sum()) > N // 4
    assert float((-2.0 * torch.log(g[:N]) - 36.0).abs().min()) > (1e-6 if dtype == "float64" else 2e-3)

    def single(f, tr, q, k, fr, dist):
        return aggregate_torch.aggregate(mask, delta, g, f.repeat(9, 1), tr, q.repeat(9, 1), k.repeat(9, 1), fr, dist)[:N]
    a64 = A.head_arguments(N, H, L, K, F)
    a64[4] = a64[4] / half(box)
    args = A.on_gpu(a64, DTYPES[dtype])
    r = A.weights(N, H, L, DTYPES[dtype])
    s = A.sampler_on(means, conics, periodic=box, periodic_aggregate=True, host=host)
    got = A.run(s.aggregate_neighbors_heads, args, r)
    assert got[0].shape == (N, H, L)
    A.assert_within(got, A.expected(single, args, r), tol, f"box C torus heads N={N} H={H} {dtype} {host} against the checker")
    f, tr, q, k, fr, dist = args
    apart = A.run(lambda *x: torch.stack([s.aggregate_neighbors(x[0], x[1][h], x[2][:, h], x[3][:, h], x[4], x[5][h])
                                          for h in range(H)], dim=1), args, r)
    A.assert_within(got, apart, tol, f"box C torus heads N={N} H={H} {dtype} {host} against {H} separate calls")


# ---- (3)
def test_translation_round_the_torus_on_box_d(hip_lib):
    box = BOXES["D"]
    a = half(box)
    n_side, L, K, F = 8, 4, 4, 3
    N = n_side * n_side
    m64, c64 = P.lattice(n_side, seed=3, box=box)
    conics = c64.cuda()
    args = P.arguments(N, L, K, F, torch.float64)
    with torch.no_grad():
        args[4].div_(a)
    r = torch.randn((N, L), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    base = P.run(P.sampler_for(m64.cuda(), conics, periodic=box), args, r)
    # the base is itself right (and through images): otherwise two equal wrong answers would pass
    want, mask, margin = P.checker(m64, c64, args, r, 36.0, box[0], box[1] - box[0])
    assert margin > 1e-6 and bool(mask.reshape(N, 9, N)[:, 1:].any())
    P.assert_within(P.errors(base, want), 1e-11)
    means = (m64 + torch.tensor((0.37 * a, -0.81 * a), dtype=torch.float64)).cuda()
    _, _, margin = P.checker(means, conics, args, r, 36.0, box[0], box[1] - box[0])
    assert margin > 1e-6, margin                                # no neighbour can flip
    assert bool((means.cpu() < box[0]).any() or (means.cpu() >= box[1]).any())      # some means left the box
    err = P.errors(P.run(P.sampler_for(means, conics, periodic=box), args, r), base)
    print(f"box D, shift (0.37, -0.81) a: periodic lists move by {err}")
    P.assert_all_below(err, 1e-10)


# ---- (4)
@pytest.mark.parametrize("host", HOSTS)
def test_gradcheck_round_a_corner_of_box_c(hip_lib, host):
    box = BOXES["C"]
    a = half(box)
    lo, hi = box
    off = torch.tensor([[-0.07, -0.05], [0.06, -0.08], [-0.04, 0.07], [0.05, 0.04], [0.02, -0.03], [-0.09, 0.09]],
                       dtype=torch.float64) * a
    means = (torch.tensor([hi, hi], dtype=torch.float64) + off).cuda()      # round the corner (hi, hi) = (lo, lo)
    g = torch.Generator().manual_seed(2)
    sd = (0.06 + 0.04 * torch.rand((6, 2), generator=g, dtype=torch.float64)) * a
    conics = G.conics_of(sd[:, 0], sd[:, 1], torch.rand(6, generator=g, dtype=torch.float64) - 0.5).cuda()
    s = P.sampler_for(means, conics, periodic=box, host=host)
    nb = s._neighbors
    assert int(nb.row_counts.sum()) == int(nb.col_counts.sum()) > 6
    k_used = P.image_indices(nb)
    assert {1, 3, 6, 8} & set(k_used.tolist())                  # a diagonal image: the corner itself
    args = P.arguments(6, 2, 4, 2, torch.float64)
    with torch.no_grad():
        args[4].div_(a)
    assert torch.autograd.gradcheck(lambda *x: s.aggregate_neighbors(*x), args, eps=1e-6 * a)
