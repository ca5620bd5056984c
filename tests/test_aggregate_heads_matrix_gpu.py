"""GPU: the four aggregate_heads_* kernels of pigs_amd/csrc/aggregate.hip at every launch variant against the float64
sparse checker (oracle/aggregate_sparse.py) run once per head and stacked.

tests/test_aggregate_heads_gpu.py leaves open the second component per lane of all three sampling kernels (its widths
stay within 64), two of the three outcomes of ``heads_waves_per_gaussian`` at N <= 2 048, H = 3 and 4 beyond N = 25, the
LDS requests above 64 KB in float32, F = 0 and the scalar rows of ``for_row``.  tests/test_aggregate_heads_matrix.py
asks the launchers' own choice functions and asserts, without a GPU, that the case lists below reach all of it.

Every case compares the output [N, H, L] and all six gradients.  The checker runs on the pair list read back from the
lists the library built (so the cut-off band plays no part; the lists are tests/test_aggregate_matrix_gpu.py's
business), on inputs rounded to the kernel's dtype, under random incoming gradients.  Every case asserts its scene
itself: an admitted shape, no list overflow, rows and columns from under 64 entries to more than 64 (2 wpg - 1) for the
largest wpg a kernel of the case runs with (more than 256 where that is 4 and N < 449): a second round of 64 in every
wave wherever N allows one.

(a) all-pairs lists, N = 301 / 601 / 603, scene "shapes" of tests/test_aggregate_matrix_gpu.py with six of its
    Gaussians moved out of the crowd (``scene_inputs``: that scene has no list under 64 entries);
(b) grid-built lists, the crowded scene "spread" at N = 2 049 / 4 097 / 8 193 with H = 4, 3, 4 (float64: 4, 3, 3);
(c) the <T, true> instantiations on the torus's lists, all-pairs and grid-built, H = 3, against the checker on the 9N
    images; one float32 case with a second component;
(d) three cases of (a), (b) through GaussianSampler on both hosts, each against the checker (the native host sizes
    scratch and LDS through pigs_aggregate_heads_lds_bytes and has a launch body of its own);
(e) a float32 case that catches a running maximum shared between the heads.

Bars: those of tests/test_aggregate_matrix_gpu.py -- float32 5e-5, float64 1e-10, the frequency gradient x 10, relative
to the largest entry of the tensor; (e) at the 2e-5 of the test it complements.  No case needed another.

Waves per Gaussian (forward / rows / columns) as the launchers choose them -- ``WAVES`` below, which the CPU file's
coverage test holds against the launchers' rule -- with (H, L, K, F) @ N:
    float32  (2, 40, 24, 5) @ 301: 4/4/2, @ 601: 2/2/1   (3, 20, 22, 4) @ 301: 4/4/2   (3, 21, 21, 4) @ 603: 4/2/1
             (4, 8, 24, 2) @ 301: 4/2/2, @ 601: 4/1/1    (2, 62, 2, 8) @ 301: 2/4/2, @ 601: 1/4/1
             (2, 1, 63, 2) @ 301: 4/2/2                  (4, 1, 29, 12) @ 301: 4/2/2
    float64  (2, 30, 8, 5) @ 301: 2/4/2, @ 601: 1/4/1    (2, 37, 2, 7) @ 301: 2/4/2    (2, 4, 33, 2) @ 601: 4/1/1
             (3, 2, 22, 1) @ 301: 4/2/2                  (4, 2, 16, 3) @ 301: 4/2/2    (4, 1, 14, 14) @ 301: 2/2/2
    both     (4, 1, 1, 0), (4, 2, 3, 1), (3, 7, 5, 2) @ 301: 4/4/4;  (2, 16, 16, 6) @ 301: 4/4/4 in float32, 2/2/2 in float64
    grid     N = 2 049: 4/4/4, 4 097: 2/2/2, 8 193: 1/1/1;  torus (3, 4, 1, 3) @ 400, 2 500: 4/4/4, (3, 21, 21, 4) @ 400: 4/4/2

Measured on an MI355X (all 43 tests, 19 s; the longest 3.1 s: float32 H = 4 at N = 8 193, 1 250 963 pairs, then 1.7 s
for float64 H = 3 there; every case of (a) under 0.8 s).  Worst error over all cases, float32 / float64: output 9.5e-7 /
2.5e-15, features 6.9e-7 / 2.4e-15, transforms 6.2e-7 / 4.4e-15, queries 6.3e-6 / 8.8e-14, keys 8.8e-7 / 3.2e-15,
frequencies 2.1e-5 ((4, 2, 3, 1); 4.6e-6 elsewhere) / 2.9e-14, distance_transforms 6.6e-7 / 4.7e-15.  (e): head 0's
row maxima up to 1.31, head 1's up to 489, the gap above 104 in all 25 rows; head 0's slices within 1.5e-6.
The unedited kernels pass every case: the matrix found no defect in them.

What the matrix catches.  Three value-only edits of aggregate.hip, each built in a scratch copy and run once:
(1) the forward's second run_rows_heads call gets dens0 for dens1: the 11 cases whose forward has a second component
    fail (float32 (2, 40, 24, 5) and (2, 62, 2, 8) at both N, (4, 1, 29, 12); float64 (2, 30, 8, 5) at both N and on
    both hosts, (2, 37, 2, 7), (4, 1, 14, 14)), output off by 0.07 to 0.15 of its largest entry; the other 32 pass;
(2) the rows kernel's pick_for(hd1) gets hd0: the 17 cases whose rows kernel has a second component fail (float32
    (3, 20, 22, 4), (3, 21, 21, 4) @ 603 and on both hosts and on the torus, (4, 8, 24, 2) at both N, (2, 1, 63, 2),
    (4, 1, 29, 12), (4, 16, 16, 2) @ 2 049 -- both hosts too -- and 8 193; float64 (2, 4, 33, 2), (3, 2, 22, 1),
    (4, 2, 16, 3), (4, 1, 14, 14)), d queries off by 0.4 to 1.8 or, where the frequencies are what lies beyond lane
    63, d frequencies by 0.6 to 6.3; the other 26 pass;
(3) the columns kernel's d features epilogue adds head 0's share H times: all 43 fail, d features off by 0.5 to 5.3.
Under (1) and (2) all 78 tests of tests/test_aggregate_heads_gpu.py and tests/test_aggregate_matrix_gpu.py still pass:
nothing there reaches a second component of a heads kernel.  Under (3) 20 of tests/test_aggregate_heads_gpu.py fail as
well (every comparison with H >= 2): that edit is not particular to a second component and was caught before.
"""
import functools

import pytest
import torch

from oracle import aggregate_sparse as sparse

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float64": torch.float64}
TOL = {"float32": 5e-5, "float64": 1e-10}
HOSTS = ("native", "ctypes")

# ---- the case lists: plain data (tests/test_aggregate_heads_matrix.py reads them without a GPU)
# (a) (dtype, H, L, K, F, N): all-pairs lists of the scene "shapes" of tests/test_aggregate_matrix_gpu.py
SHAPE_CASES = [
    ("float32", 2, 40, 24, 5, 301), ("float32", 2, 40, 24, 5, 601),      # WC 80 / 53 / 128
    ("float32", 3, 20, 22, 4, 301),                                      # WC 52 / 70 / 126: head 2's K-block over lanes 63 | 64
    ("float32", 3, 21, 21, 4, 603),                                      # WC 53 / 67 / 126: the three kernels at 4 / 2 / 1
    ("float32", 4, 8, 24, 2, 301), ("float32", 4, 8, 24, 2, 601),        # WC 24 / 98 / 128
    ("float32", 2, 62, 2, 8, 301), ("float32", 2, 62, 2, 8, 601),        # forward WC 126, L + 4F = 94: 97 280 B
    ("float32", 2, 1, 63, 2, 301),                                       # rows and cols 128: all lanes
    ("float32", 4, 1, 29, 12, 301),                                      # the largest, 140 800 B
    ("float64", 2, 30, 8, 5, 301), ("float64", 2, 30, 8, 5, 601),        # WC 70 / 21 / 76; cols 157 696 B
    ("float64", 2, 37, 2, 7, 301),                                       # WC 93 / 11 / 78: L + 4F = 65, H L = 74
    ("float64", 2, 4, 33, 2, 601), ("float64", 3, 2, 22, 1, 301), ("float64", 4, 2, 16, 3, 301),     # rows 67-68, cols 72-74
    ("float64", 4, 1, 14, 14, 301),                                      # the largest, 162 816 B
] + [(t, H, L, K, F, 301) for t in DTYPES for H, L, K, F in ((4, 1, 1, 0), (4, 2, 3, 1),        # region = H PART; F = 0
                                                             (3, 7, 5, 2),                      # scalar rows
                                                             (2, 16, 16, 6))]                   # vector rows, the model's shape
# (b) (dtype, H, L, K, F, N): grid-built lists of the scene "spread"
VARIANT_CASES = [("float32", 4, 16, 16, 2, 2049), ("float32", 3, 16, 16, 2, 4097), ("float32", 4, 16, 16, 2, 8193),
                 ("float64", 4, 8, 8, 2, 2049), ("float64", 3, 8, 8, 2, 4097), ("float64", 3, 8, 8, 2, 8193)]
# (c) (dtype, generator, N, H, L, K, F): lists of the torus
PERIODIC_CASES = [(t, "torus", N, 3, 4, 1, 3) for t in DTYPES for N in (400, 2500)] + [("float32", "torus", 400, 3, 21, 21, 4)]
# (d) cases of (a) and (b) through GaussianSampler(..., host=...), both hosts
HOST_CASES = [("float32", 3, 21, 21, 4, 603), ("float64", 2, 30, 8, 5, 301), ("float32", 4, 16, 16, 2, 2049)]

# waves per Gaussian (forward, rows, cols) of every case, as tests/test_aggregate_heads_matrix.py predicts them
WAVES = {
    ("float32", 2, 40, 24, 5, 301): (4, 4, 2),
    ("float32", 2, 40, 24, 5, 601): (2, 2, 1),
    ("float32", 3, 20, 22, 4, 301): (4, 4, 2),
    ("float32", 3, 21, 21, 4, 603): (4, 2, 1),
    ("float32", 4, 8, 24, 2, 301): (4, 2, 2),
    ("float32", 4, 8, 24, 2, 601): (4, 1, 1),
    ("float32", 2, 62, 2, 8, 301): (2, 4, 2),
    ("float32", 2, 62, 2, 8, 601): (1, 4, 1),
    ("float32", 2, 1, 63, 2, 301): (4, 2, 2),
    ("float32", 4, 1, 29, 12, 301): (4, 2, 2),
    ("float64", 2, 30, 8, 5, 301): (2, 4, 2),
    ("float64", 2, 30, 8, 5, 601): (1, 4, 1),
    ("float64", 2, 37, 2, 7, 301): (2, 4, 2),
    ("float64", 2, 4, 33, 2, 601): (4, 1, 1),
    ("float64", 3, 2, 22, 1, 301): (4, 2, 2),
    ("float64", 4, 2, 16, 3, 301): (4, 2, 2),
    ("float64", 4, 1, 14, 14, 301): (2, 2, 2),
    ("float32", 4, 1, 1, 0, 301): (4, 4, 4),
    ("float32", 4, 2, 3, 1, 301): (4, 4, 4),
    ("float32", 3, 7, 5, 2, 301): (4, 4, 4),
    ("float32", 2, 16, 16, 6, 301): (4, 4, 4),
    ("float64", 4, 1, 1, 0, 301): (4, 4, 4),
    ("float64", 4, 2, 3, 1, 301): (4, 4, 4),
    ("float64", 3, 7, 5, 2, 301): (4, 4, 4),
    ("float64", 2, 16, 16, 6, 301): (2, 2, 2),
    ("float32", 4, 16, 16, 2, 2049): (4, 4, 4),
    ("float32", 3, 16, 16, 2, 4097): (2, 2, 2),
    ("float32", 4, 16, 16, 2, 8193): (1, 1, 1),
    ("float64", 4, 8, 8, 2, 2049): (4, 4, 4),
    ("float64", 3, 8, 8, 2, 4097): (2, 2, 2),
    ("float64", 3, 8, 8, 2, 8193): (1, 1, 1),
    ("float32", 3, 4, 1, 3, 400): (4, 4, 4),
    ("float32", 3, 4, 1, 3, 2500): (4, 4, 4),
    ("float64", 3, 4, 1, 3, 400): (4, 4, 4),
    ("float64", 3, 4, 1, 3, 2500): (4, 4, 4),
    ("float32", 3, 21, 21, 4, 400): (4, 4, 2),
}


# ---- scenes: the lists the library built and their pairs, shared between the cases
LONERS = 6


def scene_inputs(dtype, gen, N):
    """means, conics of a scene, rounded to ``dtype`` (float64 on the CPU): those of tests/test_aggregate_matrix_gpu.py.
    Its scene "shapes" has no short list (at N = 301 the rows hold 182 to 289 entries, the columns 85 to 301), so here
    its last LONERS Gaussians are moved out of the crowd and made small: each reaches nobody but itself (a column of
    one entry: three of a Gaussian's four waves without a round) and is reached by itself and by the one Gaussian that
    reaches everybody (a row of two)."""
    import test_aggregate_matrix_gpu as G
    means, conics = (x.clone() for x in G.inputs(dtype, gen, N))
    if gen == "shapes":
        k = torch.arange(LONERS, dtype=means.dtype)
        means[N - LONERS:] = torch.stack((3.0 + 0.5 * k, torch.full_like(k, -3.0)), dim=-1)
        conics[N - LONERS:] = torch.tensor([2500.0, 0.0, 2500.0], dtype=conics.dtype)       # standard deviation 0.02
    return means, conics


@functools.lru_cache(maxsize=None)
def scene(dtype, gen, N):
    """(lists, means, conics, I, column) of a scene: the pair list is read back from the built lists, rows and
    columns alike; on the torus column = k N + j over the 9N images and means / conics are those images'."""
    import test_aggregate_matrix_gpu as G
    from pigs_amd.aggregate import NeighborLists
    periodic = gen in G.PERIODIC_GENERATORS
    means, conics = scene_inputs(dtype, gen, N)
    nb = NeighborLists(means.cuda(), conics.cuda(), G.Q_MAX, periodic=(G.LO, G.PERIOD) if periodic else None)
    M = 9 * N if periodic else N
    rows = G.list_keys(nb.row_counts, nb.row_lists, M, N, periodic, False).sort().values
    cols = G.list_keys(nb.col_counts, nb.col_lists, M, N, periodic, True).sort().values
    assert torch.equal(rows, cols) and int(nb.overflow.item()) == 0
    m64, c64 = means.double(), conics.double()
    if periodic:
        m64, c64 = sparse.periodic_images(m64, c64, G.LO, G.PERIOD)
    return nb, m64, c64, rows // M, rows % M


def pairs_of_sampler(s, N):
    from test_aggregate_heads_gpu import pairs_of
    return pairs_of(s._neighbors, N)


def assert_rounds(nb, N, wpg):
    """Rows and columns from under 64 entries to a second round of 64 in every wave of the widest launch."""
    need = 256 if max(wpg) == 4 and N < 449 else 64 * (2 * max(wpg) - 1)
    for counts in (nb.row_counts.cpu(), nb.col_counts.cpu()):
        assert int(counts.min()) < 64 and int(counts.max()) > need, (int(counts.min()), int(counts.max()), need)


def assert_within(got, want, tol, what):
    """tests/test_aggregate_heads_gpu.py's, with the empty gradient of F = 0 (no entry to be wrong)."""
    from test_aggregate_heads_gpu import NAMES
    from test_aggregate_matrix_gpu import rel_err
    err = {}
    for name, a, b in zip(("out",) + NAMES, got, want):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err[name] = rel_err(a, b)
    print(f"{what}: bar {tol:g}, errors " + ", ".join(f"{n} {e:.2g}" for n, e in err.items()))
    for name, e in err.items():
        assert e < tol * (10 if name == "frequencies" else 1), (what, name, e, err)


def check_case(dtype, gen, N, H, L, K, F, host=None):
    import test_aggregate_heads_matrix as M
    from pigs_amd import aggregate as A
    from test_aggregate_heads_gpu import expected, head_arguments, on_gpu, run, weights
    dt = DTYPES[dtype]
    assert A.heads_refusal(dt, H, L, K, F) is None and M.admitted(dtype, H, L, K, F)
    wpg = tuple(M.waves(dtype, N, H, L, K, F)[k] for k in M.KERNELS)
    nb, m64, c64, I, col = scene(dtype, gen, N)
    periodic = m64.shape[0] != N
    if periodic:            # the torus's lists are short: what they add is the images and the <T, true> instantiations
        assert int(nb.row_counts.min()) >= 1 and int(nb.col_counts.min()) >= 1
    else:
        assert_rounds(nb, N, wpg)
    args = on_gpu(head_arguments(N, H, L, K, F), dt)
    r = weights(N, H, L, dt)
    assert bool((r.abs().amax(dim=(0, 2)) > 0).all())                  # no head without an incoming gradient
    if host is None:
        got = run(lambda *a: A.aggregate_heads(nb, *a), args, r)
    else:
        from test_aggregate_heads_gpu import sampler_on
        s = sampler_on(nb.means, nb.conics, host=host)
        own = pairs_of_sampler(s, N)
        assert torch.equal(own[0], I) and torch.equal(own[1], col)     # the sampler's lists hold the scene's pairs
        got = run(s.aggregate_neighbors_heads, args, r)
    assert got[0].shape == (N, H, L) and got[0].dtype == dt

    def single(f, tr, q, k, fr, dist):
        if periodic:
            return sparse.aggregate(N, I, col, m64, c64, f.repeat(9, 1), tr, q, k.repeat(9, 1), fr, dist)
        return sparse.aggregate(N, I, col, m64, c64, f, tr, q, k, fr, dist)
    want = expected(single, args, r)
    what = f"heads matrix {gen} N={N} H={H} L={L} K={K} F={F} {dtype}" + (f" host={host}" if host else "")
    assert_within(got, want, TOL[dtype], f"{what}, waves {wpg}, {I.numel()} pairs")


@pytest.mark.parametrize("dtype,H,L,K,F,N", SHAPE_CASES)
def test_shapes_match_the_sparse_checker_per_head(hip_lib, dtype, H, L, K, F, N):
    check_case(dtype, "shapes", N, H, L, K, F)


@pytest.mark.parametrize("dtype,H,L,K,F,N", VARIANT_CASES)
def test_grid_lists_match_the_sparse_checker_per_head(hip_lib, dtype, H, L, K, F, N):
    check_case(dtype, "spread", N, H, L, K, F)


@pytest.mark.parametrize("dtype,gen,N,H,L,K,F", PERIODIC_CASES)
def test_torus_lists_match_the_sparse_checker_per_head(hip_lib, dtype, gen, N, H, L, K, F):
    check_case(dtype, gen, N, H, L, K, F)
    nb, _, _, I, col = scene(dtype, gen, N)
    assert bool((col // N != 0).any())                                  # some pairs reach through an image


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("dtype,H,L,K,F,N", HOST_CASES)
def test_both_hosts_match_the_sparse_checker_per_head(hip_lib, dtype, H, L, K, F, N, host):
    check_case(dtype, "shapes" if N <= 2048 else "spread", N, H, L, K, F, host=host)


# ---- a softmax state per head, float32
def test_float32_softmax_state_is_per_head(hip_lib):
    """tests/test_aggregate_heads_gpu.py::test_softmax_state_is_per_head cannot catch a running maximum shared between
    the heads in float32: a scale that makes exp(s_0 - m_1) underflow puts the rounding of head 1's own scores beyond
    the bar.  Here head 1's queries are x 400 and its incoming gradient is zero, so head 1 adds exactly nothing to the
    gradients of features and frequencies and only head 0's slices are judged, against the float32 bar of that test
    (2e-5); head 1's own entries have to be finite.  With m shared, head 0's weights exp(s_0 - m_1) are all 0 in every
    row whose maxima differ by more than 104 (the smallest float32 is e^-103.3): 0 / 0."""
    from oracle import aggregate_torch as dense
    from test_aggregate_heads_gpu import expected, head_arguments, on_gpu, rel, run, sampler_on, small_scene, weights
    means, conics, nb = small_scene("float32")
    N, H, L, K, F = 25, 2, 2, 4, 5
    a64 = head_arguments(N, H, L, K, F)
    a64[2][:, 1] *= 400.0
    args = on_gpu(a64, torch.float32)
    r = weights(N, H, L, torch.float32)
    r[:, 1] = 0
    q, k = args[2].detach().double().cpu(), args[3].detach().double().cpu()
    top = [((q[:, h] @ k[:, h].t()) / 2.0).masked_fill(~nb[0], -float("inf")).amax(dim=1) for h in range(2)]     # / sqrt(K)
    gap = top[1] - top[0]
    print(f"row maxima: head 0 up to {float(top[0].max()):.3g}, head 1 up to {float(top[1].max()):.3g}; "
          f"rows with a gap above 104: {int((gap > 104).sum())} of {N}")
    assert float(top[1].max() - top[0].max()) > 104 and int((gap > 104).sum()) > N // 2
    got = run(sampler_on(means, conics).aggregate_neighbors_heads, args, r)
    want = expected(lambda *a: dense.aggregate(*nb, *a), args, r)
    out, g_f, g_tr, g_q, g_k, g_fr, g_dist = got
    w_out, w_f, w_tr, w_q, w_k, w_fr, w_dist = want
    err = {"out[:, 0]": rel(out[:, 0], w_out[:, 0]), "features": rel(g_f, w_f), "transforms[0]": rel(g_tr[0], w_tr[0]),
           "queries[:, 0]": rel(g_q[:, 0], w_q[:, 0]), "keys[:, 0]": rel(g_k[:, 0], w_k[:, 0]), "frequencies": rel(g_fr, w_fr),
           "distance_transforms[0]": rel(g_dist[0], w_dist[0])}
    print("float32 softmax state per head: " + ", ".join(f"{n} {e:.2g}" for n, e in err.items()))
    for name, e in err.items():
        assert e < 2e-5 * (10 if name == "frequencies" else 1), (name, e, err)
    for name, t in (("out[:, 1]", out[:, 1]), ("transforms[1]", g_tr[1]), ("queries[:, 1]", g_q[:, 1]), ("keys[:, 1]", g_k[:, 1]),
                    ("distance_transforms[1]", g_dist[1])):
        assert bool(torch.isfinite(t).all()), name
