"""CPU: the table that says the GPU matrix of the binned path (tests/test_binned_matrix_gpu.py) runs every instantiation
of pigs_amd/csrc/plan.hip's sampling kernels -- tile_forward_kernel<C, MASK>, tile_backward_kernel<C, MASK> and the
plan_lists_forward_kernel<C, MASK> of the fused first launch -- in every tile mode, and that the table describes the
source.

Restated by hand: ``covering_mask_of`` (tests/test_dense_matrix.py covering_mask), the two ``PIGS_CASE`` tables of
``plan_forward_c`` / ``plan_backward_c`` as INSTANCES, ``fused_first_compiled`` as FUSED_FIRST, the four tile modes, and
``list_cap_for`` / the finest grid of ``make_plan_layout`` (pigs_amd/csrc/plan.h).  An instantiation added to plan.hip
without a row here fails the source test; a scene dropped from the GPU module fails the coverage test."""
import os
import re

from test_dense_matrix import masks_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_MASKS = (1, 2, 4, 8, 7, 15, 16, 19, 32, 64)
C2_MASKS = (128, 256, 512)                               # ORDV, ORDC, ORDN: two channels only
NAMED = {"ORDR": 32, "ORDG": 64, "ORDV": 128, "ORDC": 256, "ORDN": 512}
INSTANCES = {(1, m) for m in PLAIN_MASKS} | {(2, m) for m in PLAIN_MASKS + C2_MASKS}
FUSED_FIRST = {(1, 1), (1, 7), (1, 19), (1, 32), (2, 7)}
MODES = ("list", "groups", "ranges", "points")
DIRECTIONS = ("forward", "backward")
# every mode where the points are sorted into cells (plain stores, or the staging records), LIST also on an index-tiled
# lattice (streamed stores): the sites of fwd_store<..., MASK, stream> and Gsym::load_* per mask
SITES = (("list", "lattice"), ("list", "sorted"), ("groups", "sorted"), ("ranges", "sorted"), ("points", "sorted"))
# the helper waves' second trip through their queue does not depend on the template: two instantiations stand for all
SECOND_TRIP = {(1, 7), (2, 512)}

# ---- plan.h
POINTS_MODE_MIN_CELLS, POINTS_MODE_MIN_LIST, POINTS_MODE_BLOCK_CELLS, POINT_HELPER_BLOCKS = 16.0, 96, 64.0, 256
LISTS_SMALL_TILES = 4096          # build_choice.h: up to here a list wave builds one tile (its box is the "block" of the criteria)
GRID_MARGIN = 1.1251              # gauss_grid: s0 = extent * 1.1251 / G0


def list_cap_for(N):
    return min(max((N + 15) // 16 * 16, 16), 512)


def finest_grid(N):
    """make_plan_layout: G0, about 4 Gaussians per finest cell"""
    g = 1
    while g * g * 4 < N and g < 1024:
        g <<= 1
    return g


def coverage(scenes, runs, kind_of):
    """{(c, mask, mode, point order or "second trip", direction)} of the runs [(scene, c, order sets, fused kinds)]"""
    seen = set()
    for name, c, order_sets, kinds in runs:
        if name not in scenes:
            continue
        mode, order, _, _, claims, _ = scenes[name]
        pairs = [masks_of(o, b) for o, b in order_sets] + [(kind_of[k], kind_of[k]) for k in kinds]
        for fm, bm in pairs:
            for tag in (order,) + (("second trip",) if "second trip" in claims else ()):
                seen.add((c, fm, mode, tag, "forward"))
                seen.add((c, bm, mode, tag, "backward"))
    return seen


def missing(scenes, runs, kind_of):
    seen = coverage(scenes, runs, kind_of)
    want = {(c, m, mode, order, dr) for c, m in INSTANCES for mode, order in SITES for dr in DIRECTIONS}
    want |= {(c, m, "points", "second trip", dr) for c, m in SECOND_TRIP for dr in DIRECTIONS}
    return sorted(want - seen)


def fused_missing(scenes, names, calls):
    seen = set()
    for name in names:
        if name in scenes:
            for c, first in calls:
                seen.add((c, 32 if first == "linear residual" else masks_of(first)[0], scenes[name][0]))
    return sorted({(c, m, mode) for c, m in FUSED_FIRST for mode in MODES} - seen)


# ------------------------------------------------------------------------------------------
def test_every_instantiation_runs_in_every_tile_mode():
    import test_binned_matrix_gpu as G
    gaps = missing(G.SCENES, G.RUNS, G.KIND_MASKS)
    assert not gaps, gaps
    assert set(G.MODE_CODES) == set(MODES) and {s[0] for s in G.SCENES.values()} == set(MODES)
    assert len({(n, c) for n, c, _, _ in G.RUNS}) == len(G.RUNS) and {n for n, *_ in G.RUNS} == set(G.SCENES)
    # every scene is the only one somewhere: without it the table has a hole
    for name in G.SCENES:
        rest = {k: v for k, v in G.SCENES.items() if k != name}
        assert missing(rest, G.RUNS, G.KIND_MASKS), name
    # both channel counts of a scene are needed too
    for name, c, _, _ in G.RUNS:
        assert missing(G.SCENES, [r for r in G.RUNS if (r[0], r[1]) != (name, c)], G.KIND_MASKS), (name, c)


def test_every_fused_first_instantiation_runs_in_every_tile_mode():
    import test_binned_matrix_gpu as G
    assert not fused_missing(G.SCENES, G.FUSED_FIRST_SCENES, G.FUSED_FIRST_CALLS)
    assert "P-stride" not in G.FUSED_FIRST_SCENES
    for mode in MODES:          # a mode's scenes removed: its five cells are missing
        rest = {k: v for k, v in G.SCENES.items() if v[0] != mode}
        assert len(fused_missing(rest, G.FUSED_FIRST_SCENES, G.FUSED_FIRST_CALLS)) == 5, mode
    for k in range(len(G.FUSED_FIRST_CALLS)):
        assert fused_missing(G.SCENES, G.FUSED_FIRST_SCENES, G.FUSED_FIRST_CALLS[:k] + G.FUSED_FIRST_CALLS[k + 1:]), k


def source(name):
    with open(os.path.join(ROOT, "pigs_amd", "csrc", name)) as f:
        return f.read()


def body_of(text, head):
    """the text of the function whose definition starts with ``head``, up to the closing brace in column 0"""
    start = text.index(head)
    return text[start:text.index("\n}\n", start)]


def invoked(text, macro):
    """the arguments of the macro's invocations (its own #define apart), as masks"""
    return [NAMED[a] if a in NAMED else int(a) for a in re.findall(macro + r"\((\w+)\)", text) if a != "MK"]


def test_the_tables_describe_the_source():
    assert len(INSTANCES) == 23 and len(FUSED_FIRST) == 5
    plan = source("plan.hip")
    for head in ("static int plan_forward_c(", "static int plan_backward_c("):
        body = body_of(plan, head)
        both, two = body.split("if constexpr (C == 2)")
        assert "PIGS_CASE" in both and "PIGS_CASE" in two
        got = {(c, m) for c in (1, 2) for m in invoked(both, "PIGS_CASE")} | {(2, m) for m in invoked(two, "PIGS_CASE")}
        assert got == INSTANCES, (head, sorted(got ^ INSTANCES))
        assert len(invoked(both, "PIGS_CASE")) == len(PLAIN_MASKS) and len(invoked(two, "PIGS_CASE")) == len(C2_MASKS)
    fwd = body_of(plan, "static int plan_forward_c(")
    one, two = fwd[fwd.index("if constexpr (C == 1)"):fwd.index("#undef PIGS_FUSED")].split("} else {")
    got = {(1, m) for m in invoked(one, "PIGS_FUSED")} | {(2, m) for m in invoked(two, "PIGS_FUSED")}
    assert got == FUSED_FIRST, sorted(got ^ FUSED_FIRST)
    compiled = re.search(r"fused_first_compiled\(int mask\) \{ return C == 1 \? \((.*?)\) : (.*?); \}", plan)
    masks = lambda expr: {int(m) for m in re.findall(r"mask == (\d+)", expr)}
    assert {(1, m) for m in masks(compiled.group(1))} | {(2, m) for m in masks(compiled.group(2))} == FUSED_FIRST
    assert "PIGS_FUSED" not in body_of(plan, "static int plan_backward_c(")
    pair_math = source("pair_math.h")
    for name, value in NAMED.items():
        assert re.search(rf"constexpr int {name} = {value};", pair_math), name
    assert f"constexpr uint32_t LISTS_SMALL_TILES = {LISTS_SMALL_TILES};" in source("build_choice.h")
    # plan.h: the constants the scenes' comments rely on
    plan_h = source("plan.h")
    assert f"constexpr float POINTS_MODE_MIN_CELLS = {POINTS_MODE_MIN_CELLS:g}.f;" in plan_h
    assert f"constexpr uint32_t POINTS_MODE_MIN_LIST = {POINTS_MODE_MIN_LIST}u;" in plan_h
    assert f"constexpr float POINTS_MODE_BLOCK_CELLS = {POINTS_MODE_BLOCK_CELLS:g}.f;" in plan_h
    assert f"constexpr uint32_t POINT_HELPER_BLOCKS = {POINT_HELPER_BLOCKS}u;" in plan_h
    assert ("constexpr uint32_t TILE_MODE_LIST = 0u, TILE_MODE_RANGES = 1u, TILE_MODE_GROUPS = 2u, TILE_MODE_POINTS = 3u;"
            in plan_h)
    cap = body_of(plan_h, "inline uint32_t list_cap_for(int64_t N)")
    for line in ("int64_t cap = (N + 15) / 16 * 16;", "if (cap < 16) cap = 16;", "if (cap > 512) cap = 512;"):
        assert line in cap, line
    assert "while ((int64_t)g * g * 4 < N && g < 1024) g <<= 1;" in body_of(plan_h, "inline PlanLayout make_plan_layout(")
    assert f"g.s0 = ext * {GRID_MARGIN}f / (float)G0;" in plan_h
    assert [list_cap_for(n) for n in (1, 16, 17, 512, 513, 100000)] == [16, 16, 32, 512, 512, 512]
    assert [finest_grid(n) for n in (1, 4, 5, 1024, 1025, 4096, 4097)] == [1, 1, 2, 16, 32, 32, 64]


def test_scene_arithmetic():
    """What the scenes' sizes promise before any GPU is asked: the finest grid and the slab of each N, the ragged last
    tile and quad, and the two criteria that send the P scenes' tiles to the per-point walk."""
    import test_binned_matrix_gpu as G
    S = G.SCENES
    assert {n: (finest_grid(s[2]), list_cap_for(s[2])) for n, s in S.items()} == {
        "L-lattice": (16, 512), "L-sorted": (16, 512), "R": (16, 512), "G": (32, 512), "P": (32, 512), "P-stride": (64, 512)}
    assert (S["L-lattice"][2], S["L-lattice"][3]) == (24 * 24, 64 * 64)
    assert S["R"][2] > 512                                      # a slab of 512 entries that 700 Gaussians can overflow
    for name, (mode, order, N, M, claims, q_max) in S.items():
        assert N * M <= 5_000_000 or name == "P-stride", name    # (P-stride: two short runs)
        if "ragged tile" in claims:
            assert 1 <= M % 64 <= 15, name
        if "ragged quad" in claims:
            assert M % 4 != 0, name
        assert -(-M // 64) <= LISTS_SMALL_TILES
    cells_of_domain = lambda N: (finest_grid(N) / GRID_MARGIN) ** 2      # finest cells under the points' box
    # P: uniform points, a tile's box is about 1 / tiles of the domain: more than POINTS_MODE_BLOCK_CELLS
    _, _, N, M, _, _ = S["P"]
    assert cells_of_domain(N) / -(-M // 64) > POINTS_MODE_BLOCK_CELLS
    # P-stride: more than 64 tiles besides the ragged last one, so that the POINT_HELPER_BLOCKS * 4 helper waves (four
    # points each: 16 quads a tile) come round a second time; their boxes hold fewer cells than the block criterion asks
    # for and more than POINTS_MODE_MIN_CELLS: it is the long group lists that send them to the walk
    _, _, N, M, _, _ = S["P-stride"]
    assert M >= 4160 and N > 4096 and M // 64 > 64 and (M // 64) * 16 > POINT_HELPER_BLOCKS * 4
    assert POINTS_MODE_MIN_CELLS < cells_of_domain(N) / -(-M // 64) < POINTS_MODE_BLOCK_CELLS
