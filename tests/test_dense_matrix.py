"""CPU: the table that says the GPU matrix (tests/test_dense_matrix_gpu.py) runs every instantiation (dtype, d, c, covering
mask) of pigs_amd/csrc/dense.hip through every launch variant it can take, at the edges of each.

Which variant a launch takes, its thresholds, the accumulator counts, the rows chunk and ``covering_mask_of`` are asked of
the launchers' own functions (pigs_amd/csrc/dense_choice.h, instances.h) through the stand-alone program
tests/launch_choice_main.cpp (tests/host_program.py); nothing here restates them.  What stays in Python is this file's
own vocabulary: the tags that name the edges of the selection, the tags every instantiation is expected to reach, and
the coverage logic over the GPU file's case list."""
import itertools

import host_program as hp

DTYPES = hp.DTYPES


def masks():
    """the masks compiled for every (d, c): instances.h's plain list, in its order"""
    return hp.instances("dense", 1, 1)


def instances():
    import test_dense_matrix_gpu as G
    return G.INSTANCES


def K(name):
    """a named threshold of dense_choice.h"""
    return hp.constants()[name]


def ceil_div(a, b):
    return -(-a // b)


def choice(dtype, d, c, mask, N, M):
    """choose_dense_forward and choose_dense_backward, with the instantiation's can_rows, can_w16 and rows chunk"""
    return hp.dense(dtype, d, c, mask, N, M)


def forward_tags(dtype, d, c, mask, N, M):
    """The variant a forward takes, and the edges of its selection that this shape sits on.  (Tag vocabulary: this
    file's; the variant and the thresholds: the program's.)"""
    ch, blocks = choice(dtype, d, c, mask, N, M), ceil_div(M, 64)
    v = ch.forward
    tags = {v}
    if v == "rows":
        if N > ch.rows_chunk:
            tags.add("rows: more than one chunk")
        if N == K("ROWS_MIN_N"):
            tags.add("rows: smallest N")
        if blocks == K("ROWS_MAX_BLOCKS"):
            tags.add("rows: most blocks")
    else:
        if N == K("ROWS_MIN_N") - 1 and blocks <= K("ROWS_MAX_BLOCKS"):
            tags.add(v + ": N one below rows")
        if N == K("W16_MIN_N") - 1:
            tags.add(v + ": N one below w16")
        if blocks == K("ROWS_MAX_BLOCKS") + 1 and N >= K("ROWS_MIN_N"):
            tags.add(v + ": blocks one above rows")
        if blocks == K("W16_BLOCKS_BELOW") and N >= K("W16_MIN_N"):
            tags.add(v + ": blocks one above w16")
    return tags


def backward_tags(N, M):
    ch = choice("float32", 1, 1, 1, N, M)           # the backward's choice reads the sizes alone
    v = ch.backward
    tags = {v}
    if v == "staged64" and ceil_div(N, 256) * ceil_div(M, 64) == K("STAGED64_MIN_WORKGROUPS"):
        tags.add("staged64: fewest workgroups")
    if v == "staged64" and ceil_div(M, 64) == ceil_div(K("STAGED_MAX_M"), 64):
        tags.add("staged64: last 64 points it takes")
    if v == "split_atomic" and ceil_div(M, 64) == ceil_div(K("STAGED_MAX_M"), 64) + 1:
        tags.add("split_atomic: first 64 points past staged")
    if v == "split_atomic" and ch.gy == ceil_div(M, 256) and ceil_div(M, 64) >= K("W16_BLOCKS_BELOW"):
        tags.add("split_atomic: a slice per 256 points, many")
    return tags


def expected_forward_tags(dtype, d, c, mask):
    """The tags an instantiation must reach: those of the variants it can take."""
    ch = choice(dtype, d, c, mask, 1, 1)
    mid = "w16" if ch.can_w16 else "w4"
    want = {"w4", mid + ": N one below rows", "w4: N one below w16", mid + ": blocks one above rows",
            "w4: blocks one above w16"}
    if ch.can_rows:
        want |= {"rows", "rows: more than one chunk", "rows: smallest N", "rows: most blocks"}
    if ch.can_w16:
        want.add("w16")
    return want


EXPECTED_BACKWARD_TAGS = {"staged32", "staged64", "staged64: fewest workgroups", "staged64: last 64 points it takes",
                          "split_atomic", "split_atomic: first 64 points past staged",
                          "split_atomic: a slice per 256 points, many"}


def masks_of(orders, backward_orders=None):
    """(forward, backward) covering masks of one sample() call whose loss reads ``backward_orders`` (default: all)."""
    bit = lambda o: 16 if o == "lap" else 1 << o
    fwd = sum(bit(o) for o in orders)
    bwd = sum(bit(o) for o in (orders if backward_orders is None else backward_orders))
    return hp.covering(fwd), hp.covering(bwd)


def coverage(cases, order_sets, residual_masks):
    """{(dtype, d, c, mask): (forward tags, backward tags)} of a case list [(dtype, d, c, name, N, M)]."""
    seen = {}
    pairs = [masks_of(o, b) for o, b in order_sets] + [(m, m) for m in residual_masks]
    hp.dense_many([(dtype, d, c, fm, N, M) for dtype, d, c, _, N, M in cases for fm, _ in pairs] +       # one run of the program
                  [("float32", 1, 1, 1, N, M) for *_, N, M in cases] +
                  [(dtype, d, c, m, 1, 1) for dtype, d, c in instances() for m in masks()])
    for dtype, d, c, _, N, M in cases:
        for fm, bm in pairs:
            seen.setdefault((dtype, d, c, fm), (set(), set()))[0].update(forward_tags(dtype, d, c, fm, N, M))
            seen.setdefault((dtype, d, c, bm), (set(), set()))[1].update(backward_tags(N, M))
    return seen


def missing(cases, order_sets, residual_masks):
    seen = coverage(cases, order_sets, residual_masks)
    out = []
    for (dtype, d, c), mask in itertools.product(instances(), masks()):
        fwd, bwd = seen.get((dtype, d, c, mask), (set(), set()))
        for tag in sorted(expected_forward_tags(dtype, d, c, mask) - fwd) + sorted(EXPECTED_BACKWARD_TAGS - bwd):
            out.append((dtype, d, c, mask, tag))
    return out


# ------------------------------------------------------------------------------------------
def test_mirror_tables():
    """Accumulator counts (FwdLayout), chunk sizes of the rows forward, and which instantiations keep four waves: the
    program's answers."""
    MASKS = masks()
    nacc = lambda d, c, m: choice("float32", d, c, m, 1, 1).accumulators
    rows_chunk = lambda t, d, c: choice(t, d, c, 1, 1, 1).rows_chunk
    can_rows = lambda t, d, c, m: bool(choice(t, d, c, m, 1, 1).can_rows)
    can_w16 = lambda t, d, c, m: bool(choice(t, d, c, m, 1, 1).can_w16)
    assert MASKS == (1, 2, 4, 8, 7, 15, 16, 19, 32, 64)
    assert instances() == [(t, d, c) for t in ("float32", "float64") for d in (1, 2) for c in (1, 2, 3, 4)]
    assert [nacc(2, 3, m) for m in MASKS] == [3, 6, 9, 12, 18, 30, 3, 12, 3, 12]
    assert [nacc(1, 2, m) for m in MASKS] == [2, 2, 2, 2, 6, 8, 2, 6, 2, 6]
    assert rows_chunk("float32", 2, 1) == 1536 and rows_chunk("float32", 1, 1) == 3072
    assert rows_chunk("float64", 2, 4) == 512
    assert not can_rows("float32", 2, 3, 15) and can_rows("float32", 2, 2, 15) and not can_rows("float64", 2, 2, 15)
    assert can_w16("float32", 2, 1, 7) and not can_w16("float32", 2, 2, 7) and not can_w16("float64", 2, 1, 7)
    assert can_w16("float64", 2, 3, 1) and not can_w16("float64", 1, 4, 1)
    assert [hp.covering(m) for m in (5, 6, 9, 10, 17, 18, 3, 11)] == [7, 7, 15, 15, 19, 19, 7, 15]
    # of the 160 instantiations: the widest accumulator set that takes rows has 24 words (the next has 30), the widest
    # that takes sixteen waves 6 (the next has 8)
    every = [(t, d, c, m) for (t, d, c), m in itertools.product(instances(), MASKS)]
    assert len(every) == 160
    assert sum(can_rows(*i) for i in every) == 149 and sum(can_w16(*i) for i in every) == 84


def test_the_bench_size_is_one_short_of_the_direct_store():
    b = lambda N, M: choice("float32", 2, 1, 7, N, M)
    assert b(65536, 1 << 20).backward == "split_atomic" and b(65536, 1 << 20).gy == 2
    assert b(65537, 16385).backward == "split_store"
    assert b(65537, 16384).backward == "staged64"


def test_every_instantiation_runs_through_every_variant_it_can_take():
    import test_dense_matrix_gpu as G
    MASKS = masks()
    assert len(G.CASES) == 16 * 7 and len(set(G.CASES)) == len(G.CASES)
    assert sorted({(t, d, c) for t, d, c, *_ in G.CASES}) == sorted(instances())
    gaps = missing(G.CASES, G.ORDER_SETS, G.RESIDUAL_MASKS)
    assert not gaps, gaps[:10]
    # every shape is the only one at some edge: without it the table has a hole
    for name in sorted({s for _, _, _, s, _, _ in G.CASES}):
        rest = [cs for cs in G.CASES if cs[3] != name]
        assert missing(rest, G.ORDER_SETS, G.RESIDUAL_MASKS), name
    # what the table says about each shape
    for dtype, d, c, name, N, M in G.CASES:
        ch = {m: choice(dtype, d, c, m, N, M) for m in MASKS}
        f = {m: ch[m].forward for m in MASKS}
        rows = {m for m in MASKS if ch[m].can_rows}
        w16 = {m for m in MASKS if ch[m].can_w16}
        b = ch[MASKS[0]].backward
        if name in ("S1", "S2", "S5"):
            assert {m for m in MASKS if f[m] == "rows"} == rows and all(f[m] == "w4" for m in set(MASKS) - rows)
        if name == "S1":       # the GPU file writes the sixteen sizes out: each is its instantiation's chunk + 33
            assert N == ch[MASKS[0]].rows_chunk + 33 and M == 81 and b == "staged32"
        if name in ("S3", "S6"):
            assert {m for m in MASKS if f[m] == "w16"} == w16 and all(f[m] == "w4" for m in set(MASKS) - w16)
        if name in ("S4", "S7"):
            assert set(f.values()) == {"w4"}
        assert b == {"S1": "staged32", "S2": "staged32", "S3": "staged32", "S4": "staged32", "S5": "staged64",
                     "S6": "split_atomic", "S7": "split_atomic"}[name]
        if name == "S6":
            assert ch[MASKS[0]].gy == 65 and ceil_div(M, 65) == 253
        if name == "S7":
            assert ch[MASKS[0]].gy == 256


def test_the_direct_store_cases():
    import test_dense_matrix_gpu as G
    assert len(G.STORE_CASES) == 4
    for dtype, d, c, what in G.STORE_CASES:
        ch = choice(dtype, d, c, 7, G.STORE_N, G.STORE_M)
        assert ch.backward == "split_store"
        assert ch.forward != "rows"
