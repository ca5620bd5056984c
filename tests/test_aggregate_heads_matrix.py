"""CPU: the table that says the GPU matrix (tests/test_aggregate_heads_matrix_gpu.py) reaches every launch variant of
the launchers of aggregate_neighbors_heads.

The regions, each kernel's LDS request, ``components_ok``, ``aggregate_admitted``, ``heads_waves_per_gaussian`` (with
its compute units and workgroups per CU), the list build and the ``splits`` of the sums over N are asked of the
launchers' own functions (pigs_amd/csrc/aggregate_choice.h) through the stand-alone program
tests/launch_choice_main.cpp (tests/host_program.py); nothing here restates them.  What stays in Python describes the
three heads kernels' insides, which no launcher computes -- ``WC`` (``widths``), ``hd0`` / ``hd1`` (``rows_head``,
``cols_head``), ``dens1`` and ``c1 >= HL``, blocks that straddle lanes 63 | 64, ``for_row``'s alignment test on the
heads' row addresses (``vector_rows``, ``dacc_rows``) -- and this file's own vocabulary: the tags, the expected tags
and the coverage logic."""
import ctypes
import itertools

import pytest

import host_program as hp
from test_aggregate_matrix import KERNELS, SIZEOF, K_, ceil_div


def choice(dtype, N, H, L, K, F):
    return hp.aggregate(dtype, H, N, L, K, F)


def regions(H, L, K, F):
    """A wave's region of the forward, the backward by rows and the backward by columns, in values."""
    return choice("float32", 1, H, L, K, F).regions


def lds_bytes(dtype, H, L, K, F):
    return choice(dtype, 1, H, L, K, F).lds


def components_ok(H, L, K, F):
    return choice("float32", 1, H, L, K, F).components_ok


def admitted(dtype, H, L, K, F):
    """aggregate_admitted (the entry points refuse L, K < 1 and F < 0 as invalid before it)."""
    return L >= 1 and K >= 1 and F >= 0 and choice(dtype, 1, H, L, K, F).admitted


def waves(dtype, N, H, L, K, F):
    """Waves per Gaussian of the three kernels of one call."""
    return choice(dtype, N, H, L, K, F).waves


def widths(H, L, K, F):
    """WC of the three kernels: the components a wave's lanes share out, lane and lane + 64 (inside the kernels)."""
    return {"forward": L + 8 * F, "rows": H * K + F, "cols": H * (L + K)}


def rows_head(c, H, K):
    """hd0 / hd1 of the backward by rows: the head of component c, -1 for a frequency."""
    return c // K if c < H * K else -1


def cols_head(c, H, L, K):
    """hd0 / hd1 of the backward by columns, and `second` (c >= HL: the component is a d keys one)."""
    return (c // L, False) if c < H * L else ((c - H * L) // K, True)


def straddles(blocks, n):
    """A block of n components that starts before lane 64 and ends beyond it."""
    return any(b * n < 64 < (b + 1) * n for b in range(blocks))


def vector_rows(dtype, n):
    """for_row takes 16-byte loads for a row of n values when n is a multiple of V = 16 / sizeof(T) and the row starts
    on 16 bytes.  The heads' rows keys + j H K + h K, queries + (i H + h) K (n = K) and features + j L (n = L) start
    at multiples of n values from an aligned base: n a multiple of V aligns every one of them."""
    return n % (16 // SIZEOF[dtype]) == 0


def dacc_rows(dtype, H, L, F):
    """The backward by columns reads its L-rows out of dacc [N, H, W], W = L + 8F + 2, at (i H + h) W values.  With L a
    multiple of V every row takes 16-byte loads when W is one too, and those whose (i H + h) W is when it is not
    ('mixed': the lanes of a wave part ways).  W - L is 2 mod 4: float32 never has 'vector', float64 never 'mixed'."""
    V = 16 // SIZEOF[dtype]
    W = L + 8 * F + 2
    if L % V:
        return "scalar"
    starts = {((i * H + h) * W) % V for i in range(V) for h in range(H)}
    return "vector" if starts == {0} else "mixed"


@pytest.fixture(scope="module")
def largest():
    """The most LDS an admitted shape of H >= 2 heads asks for, per dtype, with the shapes that ask for it."""
    shapes = [(H, L, K, F) for H in range(2, K_("HMAX") + 1) for L, K, F in itertools.product(range(1, 64), range(1, 64), range(0, 16))]
    best = {}
    for t in SIZEOF:
        answers = hp.aggregate_many([(t, H, 1, L, K, F) for H, L, K, F in shapes])
        top = max(a.lds_bytes for a in answers if a.admitted)
        best[t] = (top, [s for s, a in zip(shapes, answers) if a.admitted and a.lds_bytes == top])
    return best


def sampling_tags(dtype, periodic, N, H, L, K, F, largest):
    """The edges of the launchers' selection that one aggregate_neighbors_heads call (forward and backward) sits on."""
    lds, wpg, wc = lds_bytes(dtype, H, L, K, F), waves(dtype, N, H, L, K, F), widths(H, L, K, F)
    HK, HL = H * K, H * L
    grid = hp.list_build(N) == "grid"
    tags = set()
    for k in KERNELS:
        if not grid:
            tags.add(f"{k}: {wpg[k]} waves per Gaussian on all-pairs lists")
            if N % (4 // wpg[k]):
                tags.add(f"{k}: idle waves in the last workgroup at {wpg[k]} waves per Gaussian")
        second = wc[k] > 64
        tags.add(f"{k}: {'second component in ' + ('all' if wc[k] == 128 else 'part of the') + ' lanes' if second else 'one component'}")
        tags.add(f"{k}: LDS {'above' if lds[k] > K_('AGG_LDS_DEFAULT') else 'within'} 64 KB")
        if second:          # the epilogue merges component lane + 64 of wpg partial results
            tags.add(f"{k}: second component at {wpg[k]} waves per Gaussian")
    if wpg["rows"] != wpg["cols"]:
        tags.add("backward: rows and columns at different waves per Gaussian")
    if wpg["forward"] != wpg["rows"] or wpg["forward"] != wpg["cols"]:
        tags.add("forward and backward at different waves per Gaussian")
    if grid:
        w = wpg["forward"]
        assert set(wpg.values()) == {w}
        if H >= 3:
            tags.add(f"grid lists: {w} waves per Gaussian with H >= 3")
        if H == 4:
            tags.add("grid lists: H = 4")
    if H >= 3:
        tags.add("sums over N: one split with H >= 3" if choice(dtype, N, H, L, K, F).splits == 1 else "sums over N: atomic splits with H >= 3")
    # forward: component c1 = lane + 64 reads the parked value c1 (features, sin / cos) below L + 4F, else c1 - 4F under
    # the density's weight (dens1)
    if wc["forward"] > 64:
        tags.add("forward: second component " + ("straddles values and density terms" if L + 4 * F > 64 else "all density terms"))
    if wc["rows"] > 64:
        heads = {rows_head(c, H, K) for c in range(64, wc["rows"])}
        if heads == {-1}:
            tags.add("rows: the frequencies alone in the second component")
        if HK > 64 and straddles(H, K):
            tags.add("rows: a head's K-block straddles lanes 63 | 64")
            if H == 3:
                tags.add("rows: H = 3, a head's K-block straddles lanes 63 | 64")
        if H == 3:
            tags.add("rows: H = 3 with a second component")
    if wc["cols"] > 64:
        second = {cols_head(c, H, L, K) for c in range(64, wc["cols"])}
        if HL <= 64:
            assert all(s for _, s in second)
            tags.add("cols: second component all query / key part")
        else:
            assert len({h for h, s in second if not s}) >= 1
            tags.add("cols: feature shares of the heads in the second component")
        if (HL > 64 and straddles(H, L)) or (HL < 64 and any(HL + b * K < 64 < HL + (b + 1) * K for b in range(H))):
            tags.add("cols: a head's block straddles lanes 63 | 64")
        if H == 3:
            tags.add("cols: H = 3 with a second component")
    if any(wc[k] > 64 for k in KERNELS):
        tags.add(f"H = {H} on a second-component case")
        if periodic:
            tags.add("periodic: a second component")
    if regions(H, L, K, F)["forward"] == H * K_("PART"):
        tags.add("forward_region = H PART")
    if max(lds.values()) == largest[dtype][0]:
        tags.add("the most LDS an admitted shape of H >= 2 asks for")
    if F == 0:
        tags.add("F = 0")
    if K == 1:
        tags.add("K = 1")
    if L == 1:
        tags.add("L = 1")
    if vector_rows(dtype, K) or K > 1:
        tags.add(f"for_row: head rows of K {'vector' if vector_rows(dtype, K) else 'scalar'}")
    tags.add(f"for_row: rows of L {'vector' if vector_rows(dtype, L) else 'scalar'}")
    tags.add(f"for_row: rows of dacc {dacc_rows(dtype, H, L, F)}")
    if periodic and H == 3:
        tags.add(f"periodic: {'grid' if grid else 'all-pairs'} lists with H = 3")
    return tags


def host_tags(dtype, N, H, L, K, F):
    """What a case of HOST_CASES puts through the native host's launch body (and the ctypes one)."""
    lds, wpg = lds_bytes(dtype, H, L, K, F), waves(dtype, N, H, L, K, F)
    tags = set()
    if len(set(wpg.values())) == 3:
        tags.add("both hosts: the three kernels at three different waves per Gaussian")
    if max(lds.values()) > K_("AGG_LDS_DEFAULT") and dtype == "float64":
        tags.add("both hosts: float64 above 64 KB of LDS")
    if choice(dtype, N, H, L, K, F).splits > 1:
        tags.add("both hosts: grid lists and atomic splits")
    return tags


def expected_tags(dtype):
    want = set()
    for k in KERNELS:
        want |= {f"{k}: {w} waves per Gaussian on all-pairs lists" for w in (4, 2, 1)}
        # four waves per Gaussian = one Gaussian per workgroup: no workgroup is partly filled
        want |= {f"{k}: idle waves in the last workgroup at {w} waves per Gaussian" for w in (2, 1)}
        want |= {f"{k}: one component", f"{k}: second component in part of the lanes", f"{k}: LDS above 64 KB", f"{k}: LDS within 64 KB"}
    # a second component at four waves per Gaussian: in float64 it asks for 133 120 B or more in the two backward kernels,
    # one workgroup a CU, which halves the waves from N = 257 on, and no grid case of float64 has one
    want |= {f"{k}: second component at {w} waves per Gaussian" for k in KERNELS for w in (4, 2, 1)
             if dtype == "float32" or w < 4}
    want |= {"backward: rows and columns at different waves per Gaussian", "forward and backward at different waves per Gaussian"}
    want |= {f"grid lists: {w} waves per Gaussian with H >= 3" for w in (4, 2, 1)} | {"grid lists: H = 4"}
    want |= {"sums over N: one split with H >= 3", "sums over N: atomic splits with H >= 3"}
    if dtype == "float32":     # float64: a stride of 129 is 264 192 B
        want |= {"rows: second component in all lanes", "cols: second component in all lanes", "periodic: a second component"}
    want |= {"forward: second component all density terms", "forward: second component straddles values and density terms"}
    want |= {"rows: a head's K-block straddles lanes 63 | 64", "rows: the frequencies alone in the second component",
             "rows: H = 3 with a second component", "rows: H = 3, a head's K-block straddles lanes 63 | 64"}
    want |= {"cols: second component all query / key part", "cols: feature shares of the heads in the second component",
             "cols: a head's block straddles lanes 63 | 64", "cols: H = 3 with a second component"}
    want |= {f"H = {h} on a second-component case" for h in (2, 3, 4)}
    want |= {"forward_region = H PART", "the most LDS an admitted shape of H >= 2 asks for", "F = 0", "K = 1", "L = 1"}
    want |= {f"for_row: head rows of K {a}" for a in ("vector", "scalar")} | {f"for_row: rows of L {a}" for a in ("vector", "scalar")}
    want |= {f"for_row: rows of dacc {a}" for a in ("scalar", "mixed" if dtype == "float32" else "vector")}
    want |= {f"periodic: {b} lists with H = 3" for b in ("all-pairs", "grid")}
    if dtype == "float32":
        want |= {"both hosts: the three kernels at three different waves per Gaussian", "both hosts: grid lists and atomic splits"}
    else:
        want.add("both hosts: float64 above 64 KB of LDS")
    return want


# Instances (name, dtype) that sit on no edge of the mirror that another case of their dtype does not reach too.  They
# stay for what the tags do not tell apart: the same second components under another combination of the three
# kernels' waves (the two N of (2, 40, 24, 5), the lower N of (2, 62, 2, 8), (4, 8, 24, 2) and (2, 30, 8, 5), (3, 21,
# 21, 4) at 4 / 2 / 1, which both hosts run as well), all lanes by rows AND by columns in one backward ((2, 1, 63, 2)),
# H = 4 with the frequencies alone beyond lane 63 ((4, 2, 16, 3)), H PART with F > 0 ((4, 2, 3, 1)), scalar rows of K,
# L and dacc at once ((3, 7, 5, 2)), the model's shape ((2, 16, 16, 6)), and the torus's all-pairs lists in float32
# next to the case with a second component there.  Every other instance is the only one somewhere: deleting it from
# the GPU file fails test_the_gpu_matrix_reaches_every_heads_variant.
NO_EDGE_OF_ITS_OWN = {
    (("shape", 2, 40, 24, 5, 301), "float32"), (("shape", 2, 40, 24, 5, 601), "float32"), (("shape", 2, 62, 2, 8, 301), "float32"),
    (("shape", 4, 8, 24, 2, 301), "float32"), (("shape", 2, 1, 63, 2, 301), "float32"), (("shape", 3, 21, 21, 4, 603), "float32"),
    (("shape", 2, 30, 8, 5, 301), "float64"), (("shape", 4, 2, 16, 3, 301), "float64"),
    (("shape", 4, 2, 3, 1, 301), "float32"), (("shape", 4, 2, 3, 1, 301), "float64"),
    (("shape", 3, 7, 5, 2, 301), "float32"), (("shape", 3, 7, 5, 2, 301), "float64"),
    (("shape", 2, 16, 16, 6, 301), "float32"), (("shape", 2, 16, 16, 6, 301), "float64"),
    (("periodic", 3, 4, 1, 3, 400), "float32")}


def all_cases(G):
    """[(name, dtype, tags-function)] of every case of the GPU file: one entry per instance (name, dtype)."""
    out = []
    for t, H, L, K, F, N in G.SHAPE_CASES:
        out.append((("shape", H, L, K, F, N), t, lambda lg, a=(t, False, N, H, L, K, F): sampling_tags(*a, lg)))
    for t, H, L, K, F, N in G.VARIANT_CASES:
        out.append((("variant", H, L, K, F, N), t, lambda lg, a=(t, False, N, H, L, K, F): sampling_tags(*a, lg)))
    for t, gen, N, H, L, K, F in G.PERIODIC_CASES:
        out.append((("periodic", H, L, K, F, N), t, lambda lg, a=(t, True, N, H, L, K, F): sampling_tags(*a, lg)))
    for t, H, L, K, F, N in G.HOST_CASES:
        out.append((("hosts", H, L, K, F, N), t, lambda lg, a=(t, N, H, L, K, F): host_tags(*a)))
    return out


def shapes_of(G):
    return [(t, H, L, K, F, N) for t, H, L, K, F, N in G.SHAPE_CASES + G.VARIANT_CASES + G.HOST_CASES] + \
           [(t, H, L, K, F, N) for t, _, N, H, L, K, F in G.PERIODIC_CASES]


def missing(cases, largest):
    seen = {t: set() for t in SIZEOF}
    for _, t, tags in cases:
        seen[t] |= tags(largest)
    return [(t, tag) for t in SIZEOF for tag in sorted(expected_tags(t) - seen[t])]


REFUSED = [("float64", 3, 16, 16, 2), ("float32", 2, 78, 50, 6), ("float64", 4, 16, 16, 6), ("float32", 4, 20, 16, 2),
           ("float32", 2, 8, 64, 6), ("float64", 2, 30, 10, 3), ("float64", 4, 1, 15, 14), ("float32", 4, 1, 30, 12)]


# ------------------------------------------------------------------------------------------
def test_mirror_tables(largest):
    """The launchers' numbers, as the program answers them."""
    heads_waves_per_gaussian, PART = hp.heads_waves, K_("PART")
    assert (K_("AGG_CUS"), K_("AGG_WORKGROUPS_PER_CU"), K_("HMAX"), PART) == (256, 8, 4, 136)
    # the model's shape at the model's N: one wave per Gaussian in all three kernels, both dtypes
    assert lds_bytes("float32", 2, 16, 16, 6) == {"forward": 41984, "rows": 44288, "cols": 66560}
    assert lds_bytes("float64", 2, 16, 16, 6) == {"forward": 83968, "rows": 88576, "cols": 133120}
    for t in SIZEOF:
        assert waves(t, 1600, 2, 16, 16, 6) == {"forward": 1, "rows": 1, "cols": 1}
    assert widths(2, 16, 16, 6) == {"forward": 64, "rows": 38, "cols": 64}         # on the edge: no second component
    assert widths(2, 17, 17, 6)["cols"] == 68                                       # L = K = 17 crosses it
    # what tests/test_aggregate_heads_gpu.py ran before this matrix: 4 waves at N = 25 and 144, 1 at 1 600, widths <= 64
    for H, L, K, F, N in ((2, 2, 4, 5, 25), (3, 2, 4, 5, 25), (4, 2, 4, 5, 25), (2, 16, 16, 6, 144), (2, 4, 4, 3, 64)):
        assert set(waves("float32", N, H, L, K, F).values()) == {4} and max(widths(H, L, K, F).values()) <= 64
    assert [heads_waves_per_gaussian(N, 66560) for N in (512, 513, 1024, 1025, 2048, 2049, 4097, 8193)] == [4, 2, 2, 1, 1, 4, 2, 1]
    assert [heads_waves_per_gaussian(N, 1024) for N in (2048, 2049)] == [4, 4]      # eight workgroups a CU: 2 048 resident
    assert [heads_waves_per_gaussian(N, 140800) for N in (256, 257, 512, 513)] == [4, 2, 2, 1]
    # the largest requests
    assert largest["float32"][0] == 140800 and (4, 1, 29, 12) in largest["float32"][1]
    assert largest["float64"][0] == 162816 and (4, 1, 14, 14) in largest["float64"][1]
    assert lds_bytes("float32", 4, 1, 29, 12)["rows"] == 140800 and lds_bytes("float64", 4, 1, 14, 14)["rows"] == 162816
    assert not admitted("float64", 3, 16, 16, 2) and lds_bytes("float64", 3, 16, 16, 2)["cols"] == 198656
    assert not admitted("float32", 2, 78, 50, 6) and not components_ok(2, 78, 50, 6)
    assert admitted("float32", 4, 16, 16, 6) and not admitted("float64", 4, 16, 16, 6)
    assert regions(4, 1, 1, 0)["forward"] == 4 * PART and regions(4, 2, 3, 1)["forward"] == 4 * PART
    assert regions(2, 2, 4, 5)["forward"] == 64 * 23
    # the lanes' heads: H = 3, K = 22 -- head 2's block is components 44 .. 65, lanes 44 .. 63 and 0, 1 of the second
    assert [rows_head(c, 3, 22) for c in (43, 44, 63, 64, 65, 66)] == [1, 2, 2, 2, 2, -1]
    assert [cols_head(c, 3, 20, 22) for c in (59, 60, 63, 64, 81, 82, 104, 125)] == \
        [(2, False), (0, True), (0, True), (0, True), (0, True), (1, True), (2, True), (2, True)]
    assert dacc_rows("float32", 2, 16, 6) == "mixed" and dacc_rows("float64", 2, 16, 6) == "vector"
    assert dacc_rows("float32", 3, 21, 4) == "scalar" and dacc_rows("float64", 3, 7, 2) == "scalar"


def test_the_mirror_matches_the_library(hip_lib):
    import test_aggregate_heads_matrix_gpu as G
    from test_aggregate_heads import calls
    forward, backward = calls(hip_lib)
    shapes = sorted({(t, H, L, K, F) for t, H, L, K, F, _ in shapes_of(G)}) + REFUSED
    for t, H, L, K, F in shapes:
        code = list(SIZEOF).index(t)
        want = max(lds_bytes(t, H, L, K, F).values()) if components_ok(H, L, K, F) else 0
        assert hip_lib.pigs_aggregate_heads_lds_bytes(code, H, L, K, F) == want, (t, H, L, K, F)
        for call in (forward, backward):
            assert call(code, H, L, K, F) == (0 if admitted(t, H, L, K, F) else 2), (t, H, L, K, F)
            assert call(code, H, L, K, F, period=2.0) == (0 if admitted(t, H, L, K, F) else 2), (t, H, L, K, F)
    assert not any(admitted(*s) for s in REFUSED)
    assert {components_ok(*s[1:]) for s in REFUSED} == {True, False}               # refused by either half of the rule
    assert ctypes.sizeof(ctypes.c_float) == SIZEOF["float32"]


def test_the_gpu_matrix_reaches_every_heads_variant(largest):
    import test_aggregate_heads_matrix_gpu as G
    cases = all_cases(G)
    assert len({(name, t) for name, t, _ in cases}) == len(cases)
    for t, H, L, K, F, N in shapes_of(G):               # no test launches a shape that the size rule refuses
        assert 2 <= H <= K_("HMAX") and admitted(t, H, L, K, F), (t, H, L, K, F)
    assert all(hp.list_build(N) == "all-pairs" for *_, N in G.SHAPE_CASES) and all(hp.list_build(N) == "grid" for *_, N in G.VARIANT_CASES)
    for case in G.HOST_CASES:                           # a host case is a case of the matrix run through both hosts
        assert case in G.SHAPE_CASES + G.VARIANT_CASES
    gaps = missing(cases, largest)
    assert not gaps, gaps
    # nothing is expected that no case could reach, and every instance (name, dtype) is the only one at some edge of
    # its dtype, but for the named ones
    redundant = {(name, t) for name, t, _ in cases if not missing([c for c in cases if (c[0], c[1]) != (name, t)], largest)}
    assert redundant == NO_EDGE_OF_ITS_OWN, redundant ^ NO_EDGE_OF_ITS_OWN
    # the waves per Gaussian (forward / rows / cols) that the GPU file's docstring quotes
    for (t, H, L, K, F, N), want in G.WAVES.items():
        assert tuple(waves(t, N, H, L, K, F)[k] for k in KERNELS) == want, (t, H, L, K, F, N)
    assert set(G.WAVES) == set(shapes_of(G))
    # what the table says about some named shapes
    tag = {(name, t): tags(largest) for name, t, tags in cases}
    assert ceil_div(603, 2) == 302
    assert "rows: H = 3, a head's K-block straddles lanes 63 | 64" in tag[("shape", 3, 20, 22, 4, 301), "float32"]
    assert "rows: the frequencies alone in the second component" in tag[("shape", 3, 21, 21, 4, 603), "float32"]
    assert "forward: second component straddles values and density terms" in tag[("shape", 2, 62, 2, 8, 301), "float32"]
    assert "cols: second component in all lanes" in tag[("shape", 2, 1, 63, 2, 301), "float32"]
