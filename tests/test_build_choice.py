"""CPU: which launches a build of the binned path issues (pigs_amd/csrc/build_choice.h, choose_build) and what the
library's two memories make of a landed copy (OrderState, PointsState).  Results never depend on the path a build takes,
so no GPU test can see a wrong condition here; this one states every rule again, in Python, and holds the C++ to it
through a small stand-alone program (tests/build_choice_main.cpp, host code only) -- exhaustively over the request's
seven booleans, `order` and the memory's answers, each combination with several draws of the sizes and settings, and over
the full cross of sizes and settings on the requests that reach the most paths."""
import itertools
import random
from collections import namedtuple

import pytest

import host_program

BBOX, ZERO, COUNT, SCAN, SCATTER, BINSORT16, BINSORT1, LISTS_SMALL, LISTS = range(9)      # build_choice.h, BuildKernel
RFS = (0, 8, 12, 128, 1024)
# (2048^2: an eighth of the count's blocks is more than the 256 workgroups that may meet at a device-wide barrier)
MS = (63, 64, 4095, 4096, 16384, 2 ** 17 - 1, 2 ** 17, 2 ** 19, 1024 * 1024, 2048 * 2048, 4096 * 4096)
NS = (0, 1023, 1024, 65536)
Q_MAX = 36.0
Q_BS = ("-1", "0", "nan", "36", "72")

Req = namedtuple("Req", "do_samples do_plan ws_clean no_lookback build_lists defer_lists fwd_only order N M q_b")
Env = namedtuple("Env", "lattice trust samples_order strips bbox no_ahead")
Mem = namedtuple("Mem", "coarse rf box_ok trust takes_strips")
Layout = namedtuple("Layout", "s_scan h_scan h_wgs h_chunk cells_per_bin ntiles p_scan")


@pytest.fixture(scope="module")
def program():
    return lambda lines: host_program.ask("build_choice_main", lines)


@pytest.fixture(scope="module")
def layouts(program):
    keys = [(n, m) for n in NS for m in MS]
    return {k: Layout(*map(int, line.split())) for k, line in zip(keys, program([f"L {n} {m} 1" for n, m in keys]))}


def ceil_div(a, b):
    return -(-a // b)


def expected(r, e, m, lay):
    """The rules of the build path, as the issue that introduced build_choice.h states them."""
    N, M = r.N, r.M
    order = e.samples_order or r.order                      # the setting overrules the caller's flag
    coarse = bool(r.do_samples and lay.cells_per_bin <= 12288 and (order == 2 or (order == 0 and M >= 2 ** 17 and m.coarse)))
    rf = m.rf if r.do_samples else 0
    bbox = 512 if (e.bbox == 512 or (e.bbox < 0 and M >= 2 ** 19 and rf == 0)) else 256
    q_b = float(r.q_b)
    if not q_b >= Q_MAX:
        q_b = Q_MAX
    fwd_only = bool(r.fwd_only and r.do_plan and r.build_lists and not r.defer_lists)
    if fwd_only:
        q_b = Q_MAX
    no_lattice = (e.lattice == 0) if e.lattice >= 0 else M < 4096
    ahead = bool(r.do_samples and r.do_plan and r.ws_clean and not coarse and not r.no_lookback and not e.no_ahead
                 and rf != 0 and not no_lattice and m.box_ok and lay.s_scan <= 1024)
    lists = bool(r.do_plan and r.build_lists and not r.defer_lists)
    strips = bool(lists and not r.no_lookback and ((e.strips == 1) if e.strips >= 0 else (N >= 1024 and m.takes_strips)))
    trusted = bool(ahead and strips and m.trust and r.order == 0 and rf >= 8 and rf % 8 == 0 and M >= 64 and M % rf == 0
                   and (M // rf) % 8 == 0)
    gb = ceil_div(N, 256) if r.do_plan else 0
    blocks = ceil_div(M, 1024)
    eighth = ceil_div(blocks, 8)
    if trusted:
        launches = [(COUNT, gb, 256, 0)]
    elif ahead and strips:
        launches = [(BBOX, bbox + gb, 256, 0), (COUNT, min(eighth, 256), 256, 0)]
    elif ahead:
        launches = [(BBOX, bbox + gb, 256, 0), (COUNT, lay.p_scan + eighth, 256, 0), (SCATTER, gb + ceil_div(M, 256), 256, 0)]
    else:
        launches = []
        if r.do_samples:
            launches.append((BBOX, bbox, 256, 0))
        elif not r.ws_clean:
            launches.append((ZERO, 64, 256, 0))
        count = lay.h_wgs if coarse else eighth if rf and not no_lattice else blocks
        launches.append((COUNT, gb + (count if r.do_samples else 0), 256, 0))
        scan = (lay.p_scan if r.do_plan and not strips else 0) + ((lay.h_scan if coarse else lay.s_scan) if r.do_samples else 0)
        if scan:
            launches.append((SCAN, scan, 256, 0))
        staged = coarse and lay.h_chunk <= 2048
        scatter = (0 if strips else gb) + ((lay.h_wgs if staged else ceil_div(M, 256)) if r.do_samples else 0)
        if scatter:
            launches.append((SCATTER, scatter, 256, lay.h_chunk * 16 + 2 * 256 * 4 if staged else 0))
        if coarse:
            if lay.cells_per_bin * 16 <= 12288:
                launches.append((BINSORT16, 256, 1024, lay.cells_per_bin * 16 * 4))
            else:
                launches.append((BINSORT1, 256, 1024, lay.cells_per_bin * 4))
    if lists:
        small = lay.ntiles <= 4096
        launches.append((LISTS_SMALL, ceil_div(lay.ntiles, 4), 256, 0) if small else (LISTS, ceil_div(lay.ntiles, 16), 256, 0))
    flags = dict(coarse=coarse, no_lattice=no_lattice, rf_hint=rf, bbox_blocks=bbox, fwd_only=fwd_only,
                 ahead=ahead and not trusted, s_scan_in_scatter=ahead and not strips, sort_in_count=ahead and strips and not trusted,
                 strips=strips, trusted=trusted, s_blocks=0 if trusted else blocks, q_max_b=q_b)
    return flags, launches, dict(ahead=ahead, lists=lists, gb=gb, eighth=eighth)


def command(r, e, m):
    return (f"C {r.do_samples} {r.do_plan} {r.ws_clean} {r.no_lookback} {r.build_lists} {r.defer_lists} {r.fwd_only} {r.order} "
            f"{r.N} {r.M} 1 {Q_MAX} {r.q_b}  {e.lattice} {e.trust} {e.samples_order} {e.strips} {e.bbox} {e.no_ahead}  "
            f"{m.coarse} {m.rf} {m.box_ok} {m.trust} {m.takes_strips}")


def parse(line):
    w = line.split()
    names = ("coarse", "no_lattice", "rf_hint", "bbox_blocks", "fwd_only", "ahead", "s_scan_in_scatter", "sort_in_count",
             "strips", "trusted", "s_blocks")
    flags = {k: int(v) for k, v in zip(names, w)}
    flags["q_max_b"] = float(w[11])
    launches = [tuple(map(int, x.split(":"))) for x in w[13:]]
    assert len(launches) == int(w[12]) <= 7
    return flags, launches


def cases():
    rng = random.Random(0)
    settings = [Env(*s) for s in itertools.product((-1, 0, 1), (-1, 0, 1), (0, 1, 2), (-1, 0, 1), (-1, 256, 512), (0, 1))]
    # every combination of the request's booleans, order and the memory's answers, each with several draws of the rest
    for bits in itertools.product((0, 1), repeat=7):
        for order in (0, 1, 2):
            for mem in itertools.product((0, 1), repeat=4):
                for _ in range(4):
                    r = Req(*bits, order, rng.choice(NS), rng.choice(MS), rng.choice(Q_BS))
                    yield r, rng.choice(settings), Mem(mem[0], rng.choice(RFS), *mem[1:])
    # every size and setting, on the requests that reach the most paths and with a memory that allows everything
    for n, m_, rf, q_b in itertools.product(NS, MS, RFS, Q_BS):
        for e in rng.sample(settings, 12) + [Env(-1, -1, 0, -1, -1, 0)]:
            for bits in ((1, 1, 1, 0, 1, 0, 0), (1, 1, 0, 0, 1, 0, 1), (0, 1, 0, 0, 1, 0, 0), (1, 0, 0, 0, 1, 0, 0)):
                yield Req(*bits, 0, n, m_, q_b), e, Mem(1, rf, 1, 1, 1)
    # each setting absent, 0 and 1 with everything else at its default
    for e in settings:
        if sum(v != d for v, d in zip(e, (-1, -1, 0, -1, -1, 0))) <= 1:
            for n, m_, rf in itertools.product(NS, MS, RFS):
                yield Req(1, 1, 1, 0, 1, 0, 0, 0, n, m_, "36"), e, Mem(1, rf, 1, 1, 1)


def test_the_largest_point_count_leaves_the_ahead_path(layouts):
    assert layouts[(1024, 4096 * 4096)].s_scan > 1024
    assert all(layouts[(1024, m)].s_scan <= 1024 for m in MS[:-1])
    assert -(-(2048 * 2048 // 1024) // 8) > 256
    # both per-bin sorts are in reach of the sizes
    assert layouts[(1024, MS[-1])].cells_per_bin * 16 > 12288 >= layouts[(1024, MS[-1])].cells_per_bin
    assert layouts[(1024, 2 ** 19)].cells_per_bin * 16 <= 12288


def test_choose_build_follows_the_rules(program, layouts):
    all_cases = list(cases())
    seen = set()
    for (r, e, m), line in zip(all_cases, program([command(*c) for c in all_cases])):
        lay = layouts[(r.N, r.M)]
        flags, launches, x = expected(r, e, m, lay)
        got_flags, got_launches = parse(line)
        assert got_flags == {k: (v if k == "q_max_b" else int(v)) for k, v in flags.items()}, (r, e, m)
        assert got_launches == launches, (r, e, m)
        # what the four shapes promise, whatever the formulas above say
        kernels = [k for k, *_ in launches]
        build, tail = (launches[:-1], launches[-1:]) if x["lists"] else (launches, [])
        # no launch of zero workgroups (N = 0 is no plan -- run_build turns it away before it chooses -- and a request for
        # neither half is never made)
        sane = (r.do_samples or r.do_plan) and not (r.do_plan and r.N == 0)
        assert all((grid > 0 or not sane) and block in (256, 1024) for _, grid, block, _ in launches)
        assert (LISTS in kernels or LISTS_SMALL in kernels) == x["lists"] and (not r.defer_lists or not tail)
        if flags["trusted"]:
            assert build == [(COUNT, ceil_div(r.N, 256), 256, 0)] and len(tail) == 1
            shape = "trusted"
        elif flags["sort_in_count"]:
            assert kernels[:2] == [BBOX, COUNT] and len(build) == 2 and build[1][1] <= 256
            shape = "ahead, strips"
        elif flags["ahead"]:
            assert kernels[:3] == [BBOX, COUNT, SCATTER] and len(build) == 3
            shape = "ahead"
        else:
            assert not x["ahead"] and kernels.count(COUNT) == 1
            shape = "chain"
            if flags["strips"]:      # nothing of the Gaussians in scan and scatter
                assert dict((k, g) for k, g, *_ in build).get(SCAN, 0) == (0 if not r.do_samples else lay.h_scan if flags["coarse"] else lay.s_scan)
                assert (SCATTER in kernels) == bool(r.do_samples)
            assert (BINSORT16 in kernels or BINSORT1 in kernels) == flags["coarse"]
            if flags["coarse"]:
                assert (BINSORT16 in kernels) == (lay.cells_per_bin * 16 <= 12288)
        seen.add((shape, bool(flags["coarse"]), bool(flags["strips"]), bool(r.do_samples), bool(r.do_plan)))
    assert {s[0] for s in seen} == {"trusted", "ahead, strips", "ahead", "chain"}
    assert {("chain", c, s, True, True) for c in (False, True) for s in (False, True)} <= seen


def order_state(program, commands):
    names = ("answer", "coarse", "rf", "axis", "box_seen", "box_stable", "same", "streak", "broken")
    return [dict(zip(names, map(int, line.split()))) for line in program(["O " + c for c in commands])]


def test_order_state(program):
    box, other = "-1 -1 1 1", "-1 -1 1 2"
    lat = lambda b, rf=128, axis=0: f"absorb {b} 0 0 {axis} {rf}"
    st = order_state(program, ["reset", lat(box), lat(box), lat(box), lat(other), lat(other), lat(other, 64), lat(other, 64),
                               "turn"])
    # stable only from the second identical finite box on; `same` counts copies that repeat (row length, box)
    assert [(s["box_seen"], s["box_stable"], s["same"]) for s in st[1:8]] == [
        (1, 0, 0), (1, 1, 1), (1, 1, 2), (1, 0, 0), (1, 1, 1), (1, 1, 0), (1, 1, 1)]
    assert st[7]["rf"] == 64 and st[8] == dict(st[7], rf=0, same=0, box_stable=0, streak=0, broken=1)
    # a box that is not finite or is empty is never stable
    for bad in ("-1 -1 inf 1", "nan -1 1 1", "-1 -1 -1 1", "1 1 -1 -1", "-inf -inf inf inf"):
        st = order_state(program, ["reset", lat(bad), lat(bad), lat(bad)])
        assert [(s["box_seen"], s["box_stable"]) for s in st[1:]] == [(0, 0)] * 3, bad
    # the streak survives copies that say the same and ends with a changed row length, a changed box or no row length
    st = order_state(program, ["reset", lat(box), lat(box), "set 128 2 70 1", lat(box), lat(box, 64), "set 128 2 70 1", lat(other),
                               "set 128 2 70 1", lat(other, 0)])
    assert (st[4]["same"], st[4]["streak"]) == (3, 70) and (st[5]["same"], st[5]["streak"]) == (0, 0)
    assert (st[7]["same"], st[7]["streak"]) == (0, 0) and (st[9]["same"], st[9]["streak"], st[9]["box_stable"]) == (0, 0, 1)
    # coarse: more than 55 % runs per point, no statistic keeps the last word, a row length clears it
    stat = lambda runs, points, rf=0: f"absorb {box} {runs} {points} 0 {rf}"
    st = order_state(program, ["reset", stat(55, 100), stat(56, 100), stat(0, 0), stat(100, 100, 128), stat(551, 1000), stat(550, 1000)])
    assert [s["coarse"] for s in st[1:]] == [0, 1, 1, 0, 1, 0]
    assert order_state(program, ["reset", f"absorb {box} 0 0 1 128"])[1]["axis"] == 1
    # trusts: mode 0 never; mode 1 with a row length and a stable box; the memory itself after three copies and 64 builds
    for rf, same, streak, stable in itertools.product((0, 128), (0, 1, 2, 3), (0, 63, 64, 65), (0, 1)):
        st = order_state(program, [f"set {rf} {same} {streak} {stable}", "trusts 0", "trusts 1", "trusts -1"])
        base = rf != 0 and stable == 1
        assert [s["answer"] for s in st[1:]] == [0, int(base), int(base and same >= 2 and streak >= 64)], (rf, same, streak, stable)
    # copy_due: the first two builds always, then every 16th, every 8th with a row length, every 32nd once it has held
    for rf, same in itertools.product((0, 128), (0, 1, 2, 5)):
        mask = 15 if rf == 0 else 31 if same >= 2 else 7
        st = order_state(program, [f"set {rf} {same} 0 1"] + [f"due {n}" for n in range(100)])
        assert [s["answer"] for s in st[1:]] == [int(n < 2 or n & mask == 0) for n in range(100)], (rf, same)


def points_state(program, commands):
    out = []
    for line in program(["P " + c for c in commands]):
        w = line.split()
        out.append(dict(answer=int(w[0]), has_points=int(w[1]), cover=float(w[2]), strips=int(w[3]), same=int(w[4])))
    return out


def test_points_state(program):
    absorb = lambda n=0, cover="10", strips=1, wanted=0, broken=0: f"absorb {n} {cover} {strips} {wanted} {broken}"
    st = points_state(program, ["reset", "takes", absorb(cover="nan"), "takes", absorb(cover="-1"), absorb(cover="64"), "takes",
                                absorb(cover="64.5"), "takes", absorb(cover="0"), "takes"])
    assert st[0]["cover"] == -1.0 and st[1]["answer"] == 0                       # nothing known: the cells
    assert st[2]["cover"] == pytest.approx(3e38) and st[3]["answer"] == 0       # a NaN cover is as bad as it gets
    assert st[4]["cover"] == pytest.approx(3e38)
    assert [st[k]["answer"] for k in (6, 8, 10)] == [1, 0, 1]
    # has_points from word 0 or word 3; such a plan keeps the cells
    for n, wanted in itertools.product((0, 3), (0, 2)):
        st = points_state(program, ["reset", absorb(n=n, wanted=wanted), "takes"])
        assert st[1]["has_points"] == int(n != 0 or wanted != 0) and st[2]["answer"] == int(n == 0 and wanted == 0)
    # `same` counts copies that led to the same choice; lattice_broken is reported to the caller
    st = points_state(program, ["reset", absorb(), absorb(), absorb(cover="20", strips=0), absorb(cover="100"), absorb(cover="200"),
                                absorb(broken=1), absorb(n=1)])
    assert [s["same"] for s in st[1:]] == [0, 1, 2, 0, 1, 0, 0]
    assert [s["answer"] for s in st[1:]] == [0, 0, 0, 0, 0, 1, 0] and [s["strips"] for s in st[1:4]] == [1, 1, 0]
    # copy_due: 7 trusted, 7 / 31 with strips, 15 otherwise; the first two builds always
    for strips, same, trusted in itertools.product((0, 1), (0, 1, 2, 4), (0, 1)):
        mask = 7 if trusted else 15 if not strips else 31 if same >= 2 else 7
        st = points_state(program, [f"set {strips} {same}"] + [f"due {n} {trusted}" for n in range(100)])
        assert [s["answer"] for s in st[1:]] == [int(n < 2 or n & mask == 0) for n in range(100)], (strips, same, trusted)
