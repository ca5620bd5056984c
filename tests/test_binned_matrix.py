"""CPU: the table that says the GPU matrix of the binned path (tests/test_binned_matrix_gpu.py) runs every instantiation
of pigs_amd/csrc/plan.hip's sampling kernels -- tile_forward_kernel<C, MASK>, tile_backward_kernel<C, MASK> and the
plan_lists_forward_kernel<C, MASK> of the fused first launch -- in every tile mode.

Which (C, MASK) are compiled and which of them have a fused first launch is read from the lists that generate plan.hip's
switches (pigs_amd/csrc/instances.h), and ``covering_mask_of``, ``list_cap_for``, the finest grid of ``make_plan_layout``
and the constants of plan.h and build_choice.h from the library's own headers, all through the stand-alone program
tests/launch_choice_main.cpp (tests/host_program.py): an instantiation added to instances.h without a scene in the
matrix fails the coverage test, and so does a scene dropped from the GPU module.  What stays in Python describes the
kernels' insides and this file's own bookkeeping, not a launcher's choice: the four tile modes, the sites of the
stores per mode, and the coverage logic."""
import host_program as hp
from test_dense_matrix import masks_of

MODES = ("list", "groups", "ranges", "points")
DIRECTIONS = ("forward", "backward")
# every mode where the points are sorted into cells (plain stores, or the staging records), LIST also on an index-tiled
# lattice (streamed stores): the sites of fwd_store<..., MASK, stream> and Gsym::load_* per mask
SITES = (("list", "lattice"), ("list", "sorted"), ("groups", "sorted"), ("ranges", "sorted"), ("points", "sorted"))
# the helper waves' second trip through their queue does not depend on the template: two instantiations stand for all
SECOND_TRIP = {(1, 7), (2, 512)}


def compiled():
    """{(c, mask)} of tile_forward_kernel / tile_backward_kernel"""
    return {(c, m) for c in (1, 2) for m in hp.instances("binned", c)}


def fused_first():
    """{(c, mask)} of plan_lists_forward_kernel"""
    return {(c, m) for c in (1, 2) for m in hp.instances("fused", c)}


def list_cap(N):
    return hp.plan_sizes(N)[0]


def finest(N):
    """G0 of make_plan_layout: about 4 Gaussians per finest cell"""
    return hp.plan_sizes(N)[1]


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
    want = {(c, m, mode, order, dr) for c, m in compiled() for mode, order in SITES for dr in DIRECTIONS}
    want |= {(c, m, "points", "second trip", dr) for c, m in SECOND_TRIP for dr in DIRECTIONS}
    return sorted(want - seen)


def fused_missing(scenes, names, calls):
    seen = set()
    for name in names:
        if name in scenes:
            for c, first in calls:
                seen.add((c, 32 if first == "linear residual" else masks_of(first)[0], scenes[name][0]))
    return sorted({(c, m, mode) for c, m in fused_first() for mode in MODES} - seen)


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


def test_the_tables_describe_the_source():
    """The instantiations and the constants, as the library's headers state them."""
    K = hp.constants()
    plain, two = hp.instances("binned", 1), hp.instances("binned", 2)
    assert len(compiled()) == 23 and len(fused_first()) == 5
    assert plain == (1, 2, 4, 8, 7, 15, 16, 19, 32, 64) and two == plain + (128, 256, 512)      # ten for both, three for two channels
    assert plain == hp.instances("dense", 1, 1)
    assert fused_first() == {(1, 1), (1, 7), (1, 19), (1, 32), (2, 7)} and fused_first() <= compiled()
    assert {n: K[n] for n in ("ORDR", "ORDG", "ORDV", "ORDC", "ORDN")} == {"ORDR": 32, "ORDG": 64, "ORDV": 128, "ORDC": 256, "ORDN": 512}
    assert K["LISTS_SMALL_TILES"] == 4096
    # plan.h: the constants the scenes' comments rely on
    assert (K["POINTS_MODE_MIN_CELLS"], K["POINTS_MODE_MIN_LIST"], K["POINTS_MODE_BLOCK_CELLS"], K["POINT_HELPER_BLOCKS"]) == (16, 96, 64, 256)
    assert (K["TILE_MODE_LIST"], K["TILE_MODE_RANGES"], K["TILE_MODE_GROUPS"], K["TILE_MODE_POINTS"]) == (0, 1, 2, 3)
    assert abs(K["GRID_MARGIN"] - 1.1251) < 1e-7            # gauss_grid: s0 = extent * GRID_MARGIN / G0, a float32
    assert [list_cap(n) for n in (1, 16, 17, 512, 513, 100000)] == [16, 16, 32, 512, 512, 512]
    assert [finest(n) for n in (1, 4, 5, 1024, 1025, 4096, 4097)] == [1, 1, 2, 16, 32, 32, 64]
    assert finest(4 * 1024 * 1024 + 1) == 1024 and finest(1 << 30) == 1024       # the grid stops at 1 024 x 1 024


def test_scene_arithmetic():
    """What the scenes' sizes promise before any GPU is asked: the finest grid and the slab of each N, the ragged last
    tile and quad, and the two criteria that send the P scenes' tiles to the per-point walk."""
    import test_binned_matrix_gpu as G
    S = G.SCENES
    K = hp.constants()
    LISTS_SMALL_TILES, GRID_MARGIN, POINT_HELPER_BLOCKS = K["LISTS_SMALL_TILES"], K["GRID_MARGIN"], K["POINT_HELPER_BLOCKS"]
    POINTS_MODE_MIN_CELLS, POINTS_MODE_BLOCK_CELLS = K["POINTS_MODE_MIN_CELLS"], K["POINTS_MODE_BLOCK_CELLS"]
    assert {n: (finest(s[2]), list_cap(s[2])) for n, s in S.items()} == {
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
    cells_of_domain = lambda N: (finest(N) / GRID_MARGIN) ** 2      # finest cells under the points' box
    # P: uniform points, a tile's box is about 1 / tiles of the domain: more than POINTS_MODE_BLOCK_CELLS
    _, _, N, M, _, _ = S["P"]
    assert cells_of_domain(N) / -(-M // 64) > POINTS_MODE_BLOCK_CELLS
    # P-stride: more than 64 tiles besides the ragged last one, so that the POINT_HELPER_BLOCKS * 4 helper waves (four
    # points each: 16 quads a tile) come round a second time; their boxes hold fewer cells than the block criterion asks
    # for and more than POINTS_MODE_MIN_CELLS: it is the long group lists that send them to the walk
    _, _, N, M, _, _ = S["P-stride"]
    assert M >= 4160 and N > 4096 and M // 64 > 64 and (M // 64) * 16 > POINT_HELPER_BLOCKS * 4
    assert POINTS_MODE_MIN_CELLS < cells_of_domain(N) / -(-M // 64) < POINTS_MODE_BLOCK_CELLS
