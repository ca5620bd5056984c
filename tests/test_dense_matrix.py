"""CPU: which kernel the dense launchers pick for a problem, mirrored in Python, and the table that says the GPU matrix
(tests/test_dense_matrix_gpu.py) runs every instantiation (dtype, d, c, covering mask) of pigs_amd/csrc/dense.hip
through every launch variant it can take, at the edges of each.

The selection below is a restatement of ``launch_dense_forward`` and ``launch_dense_backward`` (pigs_amd/csrc/dense.hip)
and of ``covering_mask_of`` (pigs_amd/csrc/launch.h); a threshold changed there is changed here, or the coverage test of
this file no longer describes what the GPU matrix runs."""
import itertools

MASKS = (1, 2, 4, 8, 7, 15, 16, 19, 32, 64)       # dispatch_mask's cases
SIZEOF = {"float32": 4, "float64": 8}
INSTANCES = [(t, d, c) for t in ("float32", "float64") for d in (1, 2) for c in (1, 2, 3, 4)]

# ---- launch_dense_forward
ROWS_MAX_WORDS = 28          # can_rows: NACC * (sizeof(T) / 4) <= 28
ROWS_MAX_BLOCKS = 256        # ... and blocks <= 256
ROWS_MIN_N = 128             # ... and N >= 128
ROWS_CHUNK_BYTES = 36 * 1024
W16_MAX_WORDS = 7            # can16: NACC * (sizeof(T) / 4) <= 7
W16_MAX_BYTES = 64           # ... and 15 * NACC * 64 * sizeof(T) <= 60 KiB
W16_BLOCKS_BELOW = 1024      # ... and blocks < 1024
W16_MIN_N = 64               # ... and N >= 64
# ---- launch_dense_backward
STAGED_MAX_M = 16384
STAGED64_MIN_WORKGROUPS = 512
SPLIT_WORKGROUPS = 2048


def ceil_div(a, b):
    return -(-a // b)


def covering_mask(mask):
    """covering_mask_of (launch.h): the compiled mask that serves a request (0: none)."""
    if mask in (32, 64):
        return mask
    if mask & 16:
        return 16 if mask == 16 else 19 if mask & ~19 == 0 else 0
    if mask in (1, 2, 4, 8):
        return mask
    return 7 if mask & ~7 == 0 else 15


def nacc(d, c, mask):
    """FwdLayout<D, C, MASK>::N (pair_math.h)"""
    nf, n3 = d * (d + 1) // 2, d * (d + 1) * (d + 2) // 6
    per = {1: 1, 16: 1, 32: 1, 2: d, 4: nf, 8: n3, 7: 1 + d + nf, 15: 1 + d + nf + n3, 19: 2 + d, 64: 2 + d}[mask]
    return per * c


def rows_chunk(dtype, d, c):
    """Gaussians per LDS chunk of dense_forward_rows_kernel"""
    return ROWS_CHUNK_BYTES // ((d + d * (d + 1) // 2 + c) * SIZEOF[dtype])


def can_rows(dtype, d, c, mask):
    return nacc(d, c, mask) * (SIZEOF[dtype] // 4) <= ROWS_MAX_WORDS


def can_w16(dtype, d, c, mask):
    n = nacc(d, c, mask)
    return n * (SIZEOF[dtype] // 4) <= W16_MAX_WORDS and n * SIZEOF[dtype] <= W16_MAX_BYTES


def forward_variant(dtype, d, c, mask, N, M):
    blocks = ceil_div(M, 64)
    if can_rows(dtype, d, c, mask) and blocks <= ROWS_MAX_BLOCKS and N >= ROWS_MIN_N:
        return "rows"
    if can_w16(dtype, d, c, mask) and blocks < W16_BLOCKS_BELOW and N >= W16_MIN_N:
        return "w16"
    return "w4"


def backward_ysplit(N, M):
    return max(1, min(SPLIT_WORKGROUPS // ceil_div(N, 64), ceil_div(M, 256), 65535))


def backward_variant(N, M):
    if M <= STAGED_MAX_M:
        return "staged64" if ceil_div(N, 256) * ceil_div(M, 64) >= STAGED64_MIN_WORKGROUPS else "staged32"
    return "split_atomic" if backward_ysplit(N, M) > 1 else "split_store"


def forward_tags(dtype, d, c, mask, N, M):
    """The variant a forward takes, and the edges of its selection that this shape sits on."""
    v, blocks = forward_variant(dtype, d, c, mask, N, M), ceil_div(M, 64)
    tags = {v}
    if v == "rows":
        if N > rows_chunk(dtype, d, c):
            tags.add("rows: more than one chunk")
        if N == ROWS_MIN_N:
            tags.add("rows: smallest N")
        if blocks == ROWS_MAX_BLOCKS:
            tags.add("rows: most blocks")
    else:
        if N == ROWS_MIN_N - 1 and blocks <= ROWS_MAX_BLOCKS:
            tags.add(v + ": N one below rows")
        if N == W16_MIN_N - 1:
            tags.add(v + ": N one below w16")
        if blocks == ROWS_MAX_BLOCKS + 1 and N >= ROWS_MIN_N:
            tags.add(v + ": blocks one above rows")
        if blocks == W16_BLOCKS_BELOW and N >= W16_MIN_N:
            tags.add(v + ": blocks one above w16")
    return tags


def backward_tags(N, M):
    v = backward_variant(N, M)
    tags = {v}
    if v == "staged64" and ceil_div(N, 256) * ceil_div(M, 64) == STAGED64_MIN_WORKGROUPS:
        tags.add("staged64: fewest workgroups")
    if v == "staged64" and ceil_div(M, 64) == ceil_div(STAGED_MAX_M, 64):
        tags.add("staged64: last 64 points it takes")
    if v == "split_atomic" and ceil_div(M, 64) == ceil_div(STAGED_MAX_M, 64) + 1:
        tags.add("split_atomic: first 64 points past staged")
    if v == "split_atomic" and backward_ysplit(N, M) == ceil_div(M, 256) and ceil_div(M, 64) >= W16_BLOCKS_BELOW:
        tags.add("split_atomic: a slice per 256 points, many")
    return tags


def expected_forward_tags(dtype, d, c, mask):
    rows, w16 = can_rows(dtype, d, c, mask), can_w16(dtype, d, c, mask)
    mid = "w16" if w16 else "w4"
    want = {"w4", mid + ": N one below rows", "w4: N one below w16", mid + ": blocks one above rows",
            "w4: blocks one above w16"}
    if rows:
        want |= {"rows", "rows: more than one chunk", "rows: smallest N", "rows: most blocks"}
    if w16:
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
    return covering_mask(fwd), covering_mask(bwd)


def coverage(cases, order_sets, residual_masks):
    """{(dtype, d, c, mask): (forward tags, backward tags)} of a case list [(dtype, d, c, name, N, M)]."""
    seen = {}
    for dtype, d, c, _, N, M in cases:
        pairs = [masks_of(o, b) for o, b in order_sets] + [(m, m) for m in residual_masks]
        for fm, bm in pairs:
            seen.setdefault((dtype, d, c, fm), (set(), set()))[0].update(forward_tags(dtype, d, c, fm, N, M))
            seen.setdefault((dtype, d, c, bm), (set(), set()))[1].update(backward_tags(N, M))
    return seen


def missing(cases, order_sets, residual_masks):
    seen = coverage(cases, order_sets, residual_masks)
    out = []
    for (dtype, d, c), mask in itertools.product(INSTANCES, MASKS):
        fwd, bwd = seen.get((dtype, d, c, mask), (set(), set()))
        for tag in sorted(expected_forward_tags(dtype, d, c, mask) - fwd) + sorted(EXPECTED_BACKWARD_TAGS - bwd):
            out.append((dtype, d, c, mask, tag))
    return out


# ------------------------------------------------------------------------------------------
def test_mirror_tables():
    """Accumulator counts (FwdLayout), chunk sizes of the rows forward, and which instantiations keep four waves."""
    assert [nacc(2, 3, m) for m in MASKS] == [3, 6, 9, 12, 18, 30, 3, 12, 3, 12]
    assert [nacc(1, 2, m) for m in MASKS] == [2, 2, 2, 2, 6, 8, 2, 6, 2, 6]
    assert rows_chunk("float32", 2, 1) == 1536 and rows_chunk("float32", 1, 1) == 3072
    assert rows_chunk("float64", 2, 4) == 512
    assert not can_rows("float32", 2, 3, 15) and can_rows("float32", 2, 2, 15) and not can_rows("float64", 2, 2, 15)
    assert can_w16("float32", 2, 1, 7) and not can_w16("float32", 2, 2, 7) and not can_w16("float64", 2, 1, 7)
    assert can_w16("float64", 2, 3, 1) and not can_w16("float64", 1, 4, 1)
    assert [covering_mask(m) for m in (5, 6, 9, 10, 17, 18, 3, 11)] == [7, 7, 15, 15, 19, 19, 7, 15]
    # of the 160 instantiations: the widest accumulator set that takes rows has 24 words (the next has 30), the widest
    # that takes sixteen waves 6 (the next has 8)
    every = [(t, d, c, m) for (t, d, c), m in itertools.product(INSTANCES, MASKS)]
    assert len(every) == 160
    assert sum(can_rows(*i) for i in every) == 149 and sum(can_w16(*i) for i in every) == 84


def test_the_bench_size_is_one_short_of_the_direct_store():
    assert backward_variant(65536, 1 << 20) == "split_atomic" and backward_ysplit(65536, 1 << 20) == 2
    assert backward_variant(65537, 16385) == "split_store"
    assert backward_variant(65537, 16384) == "staged64"


def test_every_instantiation_runs_through_every_variant_it_can_take():
    import test_dense_matrix_gpu as G
    assert len(G.CASES) == 16 * 7 and len(set(G.CASES)) == len(G.CASES)
    assert sorted({(t, d, c) for t, d, c, *_ in G.CASES}) == sorted(INSTANCES)
    gaps = missing(G.CASES, G.ORDER_SETS, G.RESIDUAL_MASKS)
    assert not gaps, gaps[:10]
    # every shape is the only one at some edge: without it the table has a hole
    for name in sorted({s for _, _, _, s, _, _ in G.CASES}):
        rest = [cs for cs in G.CASES if cs[3] != name]
        assert missing(rest, G.ORDER_SETS, G.RESIDUAL_MASKS), name
    # what the table says about each shape
    for dtype, d, c, name, N, M in G.CASES:
        f = {m: forward_variant(dtype, d, c, m, N, M) for m in MASKS}
        rows = {m for m in MASKS if can_rows(dtype, d, c, m)}
        w16 = {m for m in MASKS if can_w16(dtype, d, c, m)}
        b = backward_variant(N, M)
        if name in ("S1", "S2", "S5"):
            assert {m for m in MASKS if f[m] == "rows"} == rows and all(f[m] == "w4" for m in set(MASKS) - rows)
        if name == "S1":
            assert N == rows_chunk(dtype, d, c) + 33 and M == 81 and b == "staged32"
        if name in ("S3", "S6"):
            assert {m for m in MASKS if f[m] == "w16"} == w16 and all(f[m] == "w4" for m in set(MASKS) - w16)
        if name in ("S4", "S7"):
            assert set(f.values()) == {"w4"}
        assert b == {"S1": "staged32", "S2": "staged32", "S3": "staged32", "S4": "staged32", "S5": "staged64",
                     "S6": "split_atomic", "S7": "split_atomic"}[name]
        if name == "S6":
            assert backward_ysplit(N, M) == 65 and ceil_div(M, 65) == 253
        if name == "S7":
            assert backward_ysplit(N, M) == 256


def test_the_direct_store_cases():
    import test_dense_matrix_gpu as G
    assert len(G.STORE_CASES) == 4
    for dtype, d, c, what in G.STORE_CASES:
        assert backward_variant(G.STORE_N, G.STORE_M) == "split_store"
        assert forward_variant(dtype, d, c, 7, G.STORE_N, G.STORE_M) != "rows"
