"""CPU: the sparse checker of the aggregation (oracle/aggregate_sparse.py) against the dense one, and the table that says
the GPU matrix (tests/test_aggregate_matrix_gpu.py) reaches every launch variant of the aggregation's launchers.

Which list build a size takes, the waves per Gaussian, the splits of the sums over N, each kernel's LDS request and the
size rule are asked of the launchers' own functions (pigs_amd/csrc/aggregate_choice.h) through the stand-alone program
tests/launch_choice_main.cpp (tests/host_program.py); nothing here restates them.  What stays in Python describes the
kernels' insides, which no launcher computes -- the ``WC > 64`` branches (``second_component``) and ``for_row``'s
vector and scalar rows (``vector_rows``, ``dacc_rows``) -- and this file's own vocabulary: the tags, the tags that are
expected, and the coverage logic."""
import ctypes
import itertools

import pytest
import torch

import host_program as hp
from oracle import aggregate_sparse as sparse
from oracle import aggregate_torch as dense

SIZEOF = {"float32": 4, "float64": 8}
KERNELS = hp.KERNELS


def K_(name):
    """a constant of aggregate_choice.h"""
    return hp.constants()[name]


def ceil_div(a, b):
    return -(-a // b)


def choice(dtype, N, L, K, F, H=1):
    """choose_aggregate_forward / _backward with the regions and the size rule: .lds, .waves and .grids per kernel"""
    return hp.aggregate(dtype, H, N, L, K, F)


def lds_bytes(dtype, L, K, F):
    """Dynamic LDS of the forward, the backward by rows and the backward by columns, as the launchers ask for it."""
    return choice(dtype, 1, L, K, F).lds


def admitted(dtype, L, K, F):
    """aggregate_admitted, one head"""
    return choice(dtype, 1, L, K, F).admitted


def second_component(L, K, F):
    """Which kernels run the acc1 / lane + 64 branches (inside the kernels: no launcher computes it)."""
    return {"forward": L + 8 * F > 64, "rows": K + F > 64, "cols": L + K > 64}


def vector_rows(dtype, n):
    """for_row takes 16-byte loads for a row of n values when n is a multiple of V = 16 / sizeof(T) and the row starts
    on 16 bytes.  Rows of a contiguous [*, n] tensor (keys, queries: n = K; features: n = L; the base is aligned): n a
    multiple of V -- every row start is then aligned too."""
    return n % (16 // SIZEOF[dtype]) == 0


def dacc_rows(dtype, L, F):
    """The backward by columns reads its L-row out of dacc [N, W], W = L + 8F + 2: row i starts at i W values, so with
    L a multiple of V all rows take 16-byte loads when W is one too, and the rows whose i W is ('mixed': the lanes of
    a wave part ways) when it is not.  W - L = 2 (4F + 1) is 2 mod 4: float32 never has 'vector', float64 (V = 2)
    never 'mixed'."""
    V = 16 // SIZEOF[dtype]
    return "scalar" if L % V else "vector" if (L + 8 * F + 2) % V == 0 else "mixed"


@pytest.fixture(scope="module")
def largest():
    """The most LDS an admitted shape of each dtype asks for.  A kernel's request depends on two of the sizes: the
    forward's on L and F, the backward by rows' on K and F, the backward by columns' on L + K."""
    probes = {"forward": [(L, 1, F) for L in range(1, 127) for F in range(0, 16)],
              "rows": [(1, K, F) for K in range(1, 128) for F in range(0, 16)],
              "cols": [(n - 1, 1, 0) for n in range(2, 129)]}
    best = {}
    for dtype in SIZEOF:
        sizes = [a.lds[k] for k, shapes in probes.items()
                 for a in hp.aggregate_many([(dtype, 1, 1, L, K, F) for L, K, F in shapes]) if a.components_ok]
        best[dtype] = max(b for b in sizes if b <= K_("AGG_LDS_MAX"))
    return best


def sampling_tags(dtype, periodic, N, L, K, F, largest):
    """The edges of the launchers' selection that one aggregate_neighbors call (forward and backward) sits on."""
    ch = choice(dtype, N, L, K, F)
    assert len(set(ch.waves.values())) == 1           # one head: the three kernels share the rule
    wpg = ch.waves["forward"]
    tags = {f"waves per Gaussian: {wpg}, {'periodic' if periodic else 'plain'} lists of the {hp.list_build(N)} build",
            f"waves per Gaussian: {wpg}", "sums over N: one split" if ch.splits == 1 else "sums over N: atomic splits"}
    if N % (4 // wpg):
        tags.add(f"waves per Gaussian: {wpg}, idle waves in the last workgroup")
    lds, second = ch.lds, second_component(L, K, F)
    for k in KERNELS:
        tags.add(f"{k}: {'second component' if second[k] else 'one component'}")
        if second[k]:       # lanes with lane + 64 < WC carry one: all 64 at WC = 128, the first WC - 64 below
            wc = {"forward": L + 8 * F, "rows": K + F, "cols": L + K}[k]
            tags.add(f"{k}: second component {'in all lanes' if wc == 128 else 'in part of the lanes'}")
        tags.add(f"{k}: LDS {'above' if lds[k] > K_('AGG_LDS_DEFAULT') else 'within'} 64 KB")
        if second[k] and lds[k] <= K_("AGG_LDS_DEFAULT"):
            tags.add("second component within the default LDS")
    tags.add("second component in: " + "+".join(k for k in KERNELS if second[k]))
    tags.add(f"for_row: rows of L {'vector' if vector_rows(dtype, L) else 'scalar'}, "
             f"rows of K {'vector' if vector_rows(dtype, K) else 'scalar'}")
    tags.add(f"for_row: rows of dacc {dacc_rows(dtype, L, F)}")
    if K > 1 and not vector_rows(dtype, K):
        tags.add("for_row: scalar loop over more than one value")
    if F == 0:
        tags.add("no frequencies")
    if L + 8 * F + 2 == 128 and L + K == 128:
        tags.add("two full components per lane: W = 128 and L + K = 128")
    if max(lds.values()) == largest[dtype]:
        tags.add("the most LDS an admitted shape asks for")
    return tags


def list_tags(gen, N, periodic):
    return {f"lists: {'periodic ' if periodic else ''}{hp.list_build(N)} build, {gen}"
            + (f" N={N}" if gen == "spread" else "")}


def expected_tags(dtype):
    want = {f"waves per Gaussian: 4, {p} lists of the {b} build" for p in ("plain", "periodic") for b in ("all-pairs", "grid")}
    want |= {f"waves per Gaussian: {w}, plain lists of the grid build" for w in (2, 1)}
    want |= {f"waves per Gaussian: {w}" for w in (4, 2, 1)}
    # four waves per Gaussian = one Gaussian per workgroup: no workgroup is partly filled
    want |= {f"waves per Gaussian: {w}, idle waves in the last workgroup" for w in (2, 1)}
    want |= {"sums over N: one split", "sums over N: atomic splits"}
    for k in KERNELS:
        want |= {f"{k}: second component", f"{k}: one component", f"{k}: LDS above 64 KB", f"{k}: LDS within 64 KB"}
        want.add(f"{k}: second component in part of the lanes")
    want |= {"second component in: forward+cols", "second component in: rows+cols", "second component in: "}
    if dtype == "float32":     # float64: a second component means a stride of at least 33, 67 584 B
        want.add("second component within the default LDS")
        want.add("two full components per lane: W = 128 and L + K = 128")     # float64: L + K <= 79
        want |= {"rows: second component in all lanes", "cols: second component in all lanes"}     # the forward: L + 8F <= 126
    want |= {f"for_row: rows of dacc {a}" for a in ("scalar", "mixed" if dtype == "float32" else "vector")}
    want |= {f"for_row: rows of L {a}, rows of K {b}" for a in ("vector", "scalar") for b in ("vector", "scalar")}
    want |= {"for_row: scalar loop over more than one value", "no frequencies", "the most LDS an admitted shape asks for"}
    # the lists: the all-pairs build is tests/test_aggregate_gpu.py's; here the grid build at every launch size and edge
    want |= {f"lists: grid build, spread N={N}" for N in (2049, 4097, 8193)}
    want |= {f"lists: grid build, {g}" for g in ("scales", "anisotropic", "clusters", "rank_one")}
    if dtype == "float64":
        want.add("lists: grid build, offset")
    want |= {f"lists: periodic grid build, {g}" for g in ("torus", "torus_small", "torus_wide")}
    want.add("lists: periodic all-pairs build, torus")
    return want


# The issue's table of shapes asks for both dtypes of every row.  These two instances sit on no edge of the mirror that
# another case of their dtype does not reach too (float32: L = 78, K = 50 are scalar rows of more than one value as
# well; float64: L = K = 16 of the launch variants are vector rows as well); every other instance is the only one
# somewhere.
NO_EDGE_OF_ITS_OWN = {(("shape", "scalar_rows"), "float32"), (("shape", "vector_rows"), "float64")}


def all_cases(G):
    """[(name, dtype, tags-function)] of every case of the GPU file: one entry per instance (name, dtype)."""
    out = []
    for t, gen, N in G.LIST_CASES:
        out.append((("lists", gen, N), t, lambda lg, gen=gen, N=N: list_tags(gen, N, False)))
    for t, gen, N in G.PERIODIC_CASES:
        out.append((("periodic lists", gen, N), t, lambda lg, gen=gen, N=N: list_tags(gen, N, True)))
    for t, N, L, K, F in G.VARIANT_CASES:
        out.append((("variant", N), t, lambda lg, a=(t, False, N, L, K, F): sampling_tags(*a, lg)))
    for t, name, L, K, F in G.SHAPE_CASES:
        out.append((("shape", name), t, lambda lg, a=(t, False, G.SHAPE_N, L, K, F): sampling_tags(*a, lg)))
    for t, gen, N, L, K, F in G.PERIODIC_NUMERIC:
        out.append((("periodic", gen, N), t, lambda lg, a=(t, True, N, L, K, F): sampling_tags(*a, lg)))
    return out


def missing(cases, largest):
    seen = {t: set() for t in SIZEOF}
    for _, t, tags in cases:
        seen[t] |= tags(largest)
    return [(t, tag) for t in SIZEOF for tag in sorted(expected_tags(t) - seen[t])]


# ------------------------------------------------------------------------------------------
def test_mirror_tables(largest):
    """The launchers' numbers, as the program answers them."""
    waves_per_gaussian = lambda N: set(choice("float32", N, 16, 16, 6).waves.values())
    splits = lambda N: choice("float32", N, 16, 16, 6).splits
    assert [waves_per_gaussian(N) for N in (1, 4096, 4097, 8192, 8193)] == [{4}, {4}, {2}, {2}, {1}]
    assert [splits(N) for N in (1, 2048, 2049, 4097, 8193, 1 << 20)] == [1, 1, 2, 3, 5, 64]
    assert [hp.list_build(N) for N in (1, 2048, 2049)] == ["all-pairs", "all-pairs", "grid"]
    assert (K_("PART"), K_("AGG_LDS_DEFAULT"), K_("AGG_LDS_MAX")) == (136, 64 * 1024, 160 * 1024)
    # the figures of the LDS limit: every float32 shape of the two-components rule fits, the largest (K + F = 128 in the
    # backward by rows, whose region carries dacc_i as well) at 134 272 B
    assert largest == {"float32": 134272, "float64": 162048}
    assert all(admitted("float32", L, K, F) for L, K, F in ((126, 1, 0), (1, 127, 1), (64, 64, 7), (1, 126, 2)))
    assert lds_bytes("float32", 1, 126, 2)["rows"] == 134272
    assert lds_bytes("float32", 78, 50, 6) == {"forward": 105472, "rows": 60544, "cols": 132096}
    assert lds_bytes("float64", 126, 1, 0)["forward"] == 260096 and not admitted("float64", 126, 1, 0)
    assert lds_bytes("float64", 16, 100, 2) == {"forward": 51200, "rows": 215296, "cols": 239616}
    assert not admitted("float64", 16, 100, 2) and admitted("float32", 16, 100, 2) and admitted("float32", 126, 1, 0)
    assert lds_bytes("float64", 8, 66, 2) == {"forward": 34816, "rows": 145664, "cols": 153600} and admitted("float64", 8, 66, 2)
    assert max(lds_bytes("float64", 13, 66, 11).values()) == 162048 and admitted("float64", 13, 66, 11)
    assert not admitted("float64", 13, 66, 13) and not admitted("float64", 14, 66, 11)       # strides 79 -> 81
    assert not admitted("float32", 78, 51, 6) and not admitted("float32", 79, 50, 6)
    assert second_component(16, 16, 6) == {"forward": False, "rows": False, "cols": False}   # the model's shape: WC = 64 exactly


def test_the_c_api_applies_the_lds_limit_before_any_hip_call(hip_lib):
    """N = 0 returns after the size checks: what they admit is PIGS_OK, what they refuse PIGS_ERR_UNSUPPORTED, on the
    forward as on the backward (the pointers are never read)."""
    P, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)

    def forward(dt, L, K, F):
        return hip_lib.pigs_aggregate_forward(dt, 0, 1, L, K, F, *([P] * 13), NULL)

    def forward_periodic(dt, L, K, F):
        return hip_lib.pigs_aggregate_forward_periodic(dt, 0, 1, L, K, F, 2.0, *([P] * 13), NULL)

    def backward(dt, L, K, F):
        return hip_lib.pigs_aggregate_backward(dt, 0, 1, L, K, F, *([P] * 15), P, 1 << 20, *([P] * 6), NULL)

    def backward_periodic(dt, L, K, F):
        return hip_lib.pigs_aggregate_backward_periodic(dt, 0, 1, L, K, F, 2.0, *([P] * 15), P, 1 << 20, *([P] * 6), NULL)

    shapes = [(126, 1, 0), (16, 100, 2), (8, 66, 2), (13, 66, 11), (13, 66, 13), (78, 50, 6), (16, 16, 6), (1, 1, 0), (2, 77, 0),
              (64, 15, 0), (65, 15, 0), (3, 76, 1)]
    for (code, dtype), (L, K, F) in itertools.product(enumerate(("float32", "float64")), shapes):
        want = 0 if admitted(dtype, L, K, F) else 2
        for call in (forward, forward_periodic, backward, backward_periodic):
            assert call(code, L, K, F) == want, (call.__name__, dtype, L, K, F)
        assert hip_lib.pigs_aggregate_lds_bytes(code, L, K, F) == max(lds_bytes(dtype, L, K, F).values())
    assert {admitted("float64", *s) for s in shapes} == {True, False}
    assert hip_lib.pigs_aggregate_lds_bytes(7, 4, 4, 1) == 0 and hip_lib.pigs_aggregate_lds_bytes(0, 0, 4, 1) == 0
    header = open(__import__("pigs_amd")._lib.HERE + "/../include/pigs_amd.h").read()
    assert f"#define PIGS_AGGREGATE_LDS_MAX {K_('AGG_LDS_MAX')}" in header
    # where the GPU tests read the grid's occupied levels: inside the workspace, and only where a grid is built
    info = (ctypes.c_int64 * 2)()
    for code, N in itertools.product((0, 1), (2049, 2500, 8193)):
        assert hip_lib.pigs_aggregate_grid_info(code, N, info) == 0
        assert 0 <= info[0] <= hip_lib.pigs_aggregate_workspace_bytes(code, N) - 4 and info[0] % 4 == 0
        assert info[1] == {2049: 6, 2500: 6, 8193: 7}[N]          # finest level of G0^2 cells, 4 G0^2 >= N; G0 = 2^(levels - 1)
    assert hip_lib.pigs_aggregate_grid_info(0, K_("AGG_BRUTE_MAX"), info) == 2 and hip_lib.pigs_aggregate_grid_info(7, 4096, info) == 2


def test_the_gpu_matrix_reaches_every_launch_variant(largest):
    import test_aggregate_matrix_gpu as G
    cases = all_cases(G)
    assert len({(name, t) for name, t, _ in cases}) == len(cases)
    for t, name, L, K, F in G.SHAPE_CASES:          # no test launches a shape that the size check refuses
        assert admitted(t, L, K, F), (t, name)
    for t, *_, L, K, F in G.VARIANT_CASES + G.PERIODIC_NUMERIC:
        assert admitted(t, L, K, F)
    assert hp.list_build(G.SHAPE_N) == "all-pairs" and ceil_div(G.SHAPE_N, 64) == 5
    gaps = missing(cases, largest)
    assert not gaps, gaps
    # nothing is expected that no case could reach, and every instance (name, dtype) is the only one at some edge of
    # its dtype -- but for the two that the table of shapes asks for all the same
    redundant = {(name, t) for name, t, _ in cases if not missing([c for c in cases if (c[0], c[1]) != (name, t)], largest)}
    assert redundant == NO_EDGE_OF_ITS_OWN, redundant ^ NO_EDGE_OF_ITS_OWN
    # what the table says about the named shapes
    tag = {(name, t): tags(largest) for name, t, tags in cases}
    assert "second component within the default LDS" in tag[("shape", "forward_cols_second"), "float32"]
    assert "rows: second component in part of the lanes" in tag[("shape", "rows_cols_second"), "float32"]
    assert "rows: second component in all lanes" in tag[("shape", "float32_largest"), "float32"]
    assert "for_row: rows of dacc mixed" in tag[("variant", 2049), "float32"]      # L = 16, W = 34: odd rows start at 8 mod 16
    assert "for_row: rows of dacc vector" in tag[("variant", 2049), "float64"]
    for t, name in (("float32", "float32_largest"), ("float64", "float64_largest")):
        assert "the most LDS an admitted shape asks for" in tag[("shape", name), t]
    assert "for_row: rows of L scalar, rows of K scalar" in tag[("shape", "scalar_rows"), "float64"]
    assert "for_row: rows of L vector, rows of K vector" in tag[("shape", "vector_rows"), "float64"]
    assert "for_row: rows of L scalar, rows of K vector" in tag[("shape", "vector_rows"), "float32"]


# ------------------------------------------------------------------------------------------
# the sparse checker against the dense one
NAMES = ("features", "transform", "queries", "keys", "frequencies", "distance_transform")


def rel(got, want):
    return float((got.detach() - want.detach()).abs().max() / want.detach().abs().max())


def both_checkers(means, conics, q_max, args, r, periodic=None):
    """[out, six gradients] of the dense and of the sparse checker on the same float64 inputs."""
    N = means.shape[0]
    res = []
    for which in ("dense", "sparse"):
        a = [x.detach().clone().requires_grad_(True) for x in args]
        f, tr, q, k, fr, dist = a
        if periodic is None:
            if which == "dense":
                out = dense.aggregate(*dense.neighbor_structure(means, conics, q_max), *a)
            else:
                i, j, _, _ = sparse.brute_pairs(means, conics, q_max, band_units=0.0)
                out = sparse.aggregate(N, i, j, means, conics, *a)
        else:
            m9, c9 = sparse.periodic_images(means, conics, *periodic)
            if which == "dense":
                mask, delta, g = dense.neighbor_structure(m9, c9, q_max)
                out = dense.aggregate(mask, delta, g, f.repeat(9, 1), tr, q.repeat(9, 1), k.repeat(9, 1), fr, dist)[:N]
            else:
                i, j, kk, _, _ = sparse.brute_pairs_periodic(means, conics, q_max, *periodic, band_units=0.0)
                out = sparse.aggregate(N, i, kk * N + j, m9, c9, f.repeat(9, 1), tr, q, k.repeat(9, 1), fr, dist)
        res.append([out] + list(torch.autograd.grad((out * r).sum(), a)))
    return res


def test_sparse_checker_equals_the_dense_one():
    import test_aggregate_matrix_gpu as G
    N, L, K, F = G.SHAPE_N, 6, 5, 3
    means, conics = G.inputs("float64", "shapes", N)
    args = G.arguments(N, L, K, F)
    r = G.randn(torch.Generator().manual_seed(5), N, L)
    d, s = both_checkers(means, conics, G.Q_MAX, args, r)
    mask = dense.neighbor_structure(means, conics, G.Q_MAX)[0]
    assert not mask.all() and int(mask.sum(1).max()) > 256
    for name, a, b in zip(("out",) + NAMES, s, d):
        assert a.shape == b.shape and rel(a, b) < 1e-12, (name, rel(a, b))


def test_periodic_sparse_checker_equals_the_dense_one_on_the_images():
    import test_aggregate_matrix_gpu as G
    N, L, K, F = 64, 4, 3, 2
    g = torch.Generator().manual_seed(3)
    means, conics = G.gen_torus(g, N)
    conics = conics / 2.5 ** 2                   # half extents between half a period and a period: a j through two images
    args = G.arguments(N, L, K, F)
    r = G.randn(torch.Generator().manual_seed(5), N, L)
    d, s = both_checkers(means, conics, 44.0, args, r, periodic=(G.LO, G.PERIOD))
    i, j, k, q, S = sparse.brute_pairs_periodic(means, conics, 44.0, G.LO, G.PERIOD, band_units=0.0)
    assert bool((k != 0).any()) and int(torch.bincount(i).max()) > N
    for name, a, b in zip(("out",) + NAMES, s, d):
        assert a.shape == b.shape and rel(a, b) < 1e-12, (name, rel(a, b))


def test_sparse_checker_passes_gradcheck():
    import test_aggregate_matrix_gpu as G
    N = 25
    g = torch.Generator().manual_seed(2)
    means, conics = G.gen_torus(g, N)
    means = means - 0.31
    i, j, q, S = sparse.brute_pairs(means, conics, G.Q_MAX, band_units=0.0)
    assert N < i.numel() < N * N
    args = [a.requires_grad_(True) for a in G.arguments(N, 2, 4, 2)]
    assert torch.autograd.gradcheck(lambda *a: sparse.aggregate(N, i, j, means, conics, *a), args)


def test_the_band_classification():
    """q_max - 8 u S and q_max + 8 u S bound the band; u is the kernel's unit roundoff."""
    q = torch.tensor([35.0, 36.0 - 1e-4, 36.0, 36.0 + 1e-4, 37.0], dtype=torch.float64)
    S = torch.full_like(q, 400.0)                # 8 u S = 1.9e-4 in float32, 3.6e-13 in float64
    sure, band = sparse.classify(q, S, 36.0, torch.float32)
    assert sure.tolist() == [True, False, False, False, False] and band.tolist() == [False, True, True, True, False]
    sure, band = sparse.classify(q, S, 36.0, torch.float64)
    assert sure.tolist() == [True, True, False, False, False] and band.tolist() == [False, False, True, False, False]
