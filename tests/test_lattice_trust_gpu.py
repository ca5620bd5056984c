"""GPU: TRUSTED cold builds (include/pigs_amd.h, pigs_samples_trust_info; build_choice.h, choose_build: `trusted`,
and OrderState::trusts; plan.hip, run_build).  Once point sets of a
size have long been the same compact lattice, a cold build stops looking at the points in front of its list launch: the
Gaussians' pack writes the samples header the decision launch would have written, the list launch reads the points
through it and holds every tile's real box against the remembered one (plan_lists.h, the guard).  Results never depend
on it -- bit for bit the verified build's on a lattice, the oracle's on anything else -- and points that are no such
lattice turn the library's memory around within 8 builds.

Shapes: 32 x 32 lattice Gaussians (N = 1 024, the smallest count that keeps the caller's order) under 64 x 64 lattices
of points (M = 4 096, the smallest point set that is index-tiled at all); a broken build is 4 M pairs."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle
from pigs_amd import synthetic
from test_lattice_gpu import grid, lattice_of

pytestmark = pytest.mark.gpu
TRUST_MIN_BUILDS = 64          # build_choice.h
TOL = 1e-5
ORDERS = (0, 1, 2)


def rel(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def trust_info(lib, M):
    """[next build trusted?, trusted builds so far, times the guard turned the memory around, verified streak]"""
    info = (ctypes.c_int64 * 4)()
    assert lib.pigs_samples_trust_info(M, info) == 0
    return list(info)


class env:
    """Environment variables for the builds inside the block (the library reads them at every build); None: unset."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.values}
        for k, v in self.values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def library_decides(monkeypatch):
    for k in ("PIGS_LATTICE", "PIGS_LATTICE_TRUST", "PIGS_GAUSS_STRIPS", "PIGS_NO_AHEAD", "PIGS_SAMPLES_ORDER"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def gaussians():
    gs = synthetic.lattice_gaussians(32, 32, 0.5, seed=0)
    t = {k: gs[k].float().cuda() for k in ("means", "values", "conics")}
    args = [t[k].cpu().double().numpy() for k in ("means", "conics", "values")]       # the oracle's order
    return t, args


def f32(points):
    return np.asarray(points, dtype=np.float32).astype(np.float64)      # the coordinates the device sees


LATTICE = f32(grid(64, 64, lo=(-1.0, -1.0), hi=(1.0, 1.0)))
M = LATTICE.shape[0]


@functools.lru_cache(maxsize=None)
def lattice_oracle():
    return c_oracle.forward(*gaussians()[1], LATTICE, orders=ORDERS)


def make_sampler(host=None):
    from diff_gaussian_sampling import GaussianSampler
    return GaussianSampler(False, backend="binned", fuse="all", reuse_samples=False, host=host)


def step(s, points):
    """One cold step on a fresh copy of the points; the outputs, cloned."""
    t, _ = gaussians()
    p = torch.as_tensor(points, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        s.preprocess(t["means"], t["values"], None, t["conics"], p)
        outs = [o.clone() for o in s.sample(ORDERS)]
    torch.cuda.synchronize()
    return outs


def check_oracle(outs, points, exp=None):
    """Within TOL of the oracle at the points whose coordinates are finite, and finite there."""
    points = np.asarray(points)
    keep = np.isfinite(points).all(1)
    if exp is None:
        exp = c_oracle.forward(*gaussians()[1], points[keep], orders=ORDERS)
        exp = {o: exp[o] for o in ORDERS}
    else:
        exp = {o: exp[o][keep] for o in ORDERS}
    idx = torch.as_tensor(np.flatnonzero(keep), device="cuda")
    for o in ORDERS:
        got = outs[o][idx]
        assert bool(torch.isfinite(got).all()), o
        assert rel(got, exp[o]) < TOL, (o, rel(got, exp[o]))


def until_trusted(s, lib, points, limit, want=None):
    """Cold steps on `points` until the library would trust the next build of their count (and, with `want`, has
    taken them as that lattice); the number of steps it took -- three at least: a sampler's third plan is the first
    that is built into a recycled workspace, which a trusted build needs."""
    n = points.shape[0]
    for k in range(limit + 1):
        if k >= 3 and trust_info(lib, n)[0] == 1 and (want is None or lattice_of(s, lib) == want):
            return k
        step(s, points)
    raise AssertionError(("no trust after", limit, "builds", trust_info(lib, n)))


def trusted_and_verified(s, lib, points):
    """The outputs of a step that WAS trusted and of a verified step (PIGS_LATTICE_TRUST=0) on the same points."""
    n = points.shape[0]
    for _ in range(4):      # (the Gaussians' side of the decision -- their strips' statistic -- may still be on its way)
        before = trust_info(lib, n)
        assert before[0] == 1
        trusted = step(s, points)
        after = trust_info(lib, n)
        if after[1] == before[1] + 1:
            break
    assert after[1] == before[1] + 1 and after[2] == before[2], (before, after)
    with env(PIGS_LATTICE_TRUST="0"):
        assert trust_info(lib, n)[0] == 0
        verified = step(s, points)
        assert trust_info(lib, n)[1] == after[1]
    return trusted, verified


def test_trust_sets_in_by_itself_and_changes_nothing(hip_lib):
    """No override: whatever earlier tests left in the memory of this size is first turned around by points in no
    order; from there the lattice is trusted after TRUST_MIN_BUILDS verified builds at the earliest (the streak and
    three agreeing statistic copies) and 4 x that at the latest.  Trusted builds are counted, and their outputs are
    the verified build's bit for bit."""
    s = make_sampler()
    rng = np.random.default_rng(41)
    for _ in range(64):
        info = trust_info(hip_lib, M)
        if info[0] == 0 and info[3] == 0:
            break
        step(s, f32(rng.uniform(-1, 1, LATTICE.shape)))
    assert info[0] == 0 and info[3] == 0, info
    builds = until_trusted(s, hip_lib, LATTICE, 4 * TRUST_MIN_BUILDS)
    assert TRUST_MIN_BUILDS <= builds <= 4 * TRUST_MIN_BUILDS, builds
    base = trust_info(hip_lib, M)[1]
    for k in range(3):
        step(s, LATTICE)
        assert trust_info(hip_lib, M)[1] == base + k + 1
    trusted, verified = trusted_and_verified(s, hip_lib, LATTICE)
    for a, b in zip(trusted, verified):
        assert torch.equal(a, b)
    check_oracle(trusted, LATTICE, lattice_oracle())
    step(s, LATTICE)
    assert lattice_of(s, hip_lib) == (64, 64)


SHAPES = [
    ("72 x 64: odd tile count along the rows", f32(grid(72, 64, lo=(-1.0, -1.0), hi=(1.0, 1.0))), (72, 64)),
    ("64 x 72, ij order: fast axis y", f32(grid(72, 64, indexing="ij", lo=(-1.0, -1.0), hi=(1.0, 1.0))), (64, 72)),
]


@pytest.mark.parametrize("name,points,want", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes_the_index_arithmetic_can_get_wrong(hip_lib, name, points, want):
    """The serpentine's 1 x 4 blocks at its turning edge, and rows along y: the header a trusted build writes spells the
    same order as the decision launch's.  (Both shapes have the same count: the second meets the memory of the first,
    whose guard turns it around, and is learned in its place.)"""
    s = make_sampler()
    with env(PIGS_LATTICE_TRUST="1"):
        until_trusted(s, hip_lib, points, 96, want)
        trusted, verified = trusted_and_verified(s, hip_lib, points)
        assert lattice_of(s, hip_lib) == want
    for a, b in zip(trusted, verified):
        assert torch.equal(a, b)
    check_oracle(trusted, points)


def test_the_expectation_breaks(hip_lib):
    """Point sets of the trusted count that are not the remembered lattice: every step is the oracle's; a lattice that
    shrank and moved stays trusted, one that grew trips the guard, and so do a permutation, points in no order and
    (through its infinite coordinate) a lattice with non-finite points; afterwards the lattice is learned again."""
    s = make_sampler()
    rng = np.random.default_rng(43)
    bad = LATTICE.copy()
    bad[1000, 0] = np.nan
    bad[3000, 1] = np.inf
    with env(PIGS_LATTICE_TRUST="1"):
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))

        # shrunk and moved: the guard is silent
        before = trust_info(hip_lib, M)
        moved = f32(LATTICE * 0.5 + 0.25)
        for k in range(9):
            check_oracle(step(s, moved), moved)
        after = trust_info(hip_lib, M)
        assert after[0] == 1 and after[2] == before[2] and after[1] == before[1] + 9, (before, after)
        assert lattice_of(s, hip_lib) == (64, 64)

        def breaks(points, limit=9):
            """Steps on `points` until the guard's word is home; every one against the oracle."""
            fired = trust_info(hip_lib, M)[2]
            for k in range(limit):
                check_oracle(step(s, points), points)
                if trust_info(hip_lib, M)[2] > fired:
                    return
            raise AssertionError(("the guard did not fire in", limit, "builds", trust_info(hip_lib, M)))

        breaks(f32(LATTICE * 3.0))                                   # grown past twice its share
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))
        breaks(LATTICE[rng.permutation(M)])
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))

        # points in no order: the memory turns around within 8 builds and the next one sorts
        fired = trust_info(hip_lib, M)[2]
        for k in range(1 + 8 + 1):
            points = f32(rng.uniform(-1, 1, LATTICE.shape))
            check_oracle(step(s, points), points)
            if lattice_of(s, hip_lib) == (0, 0):
                break
        info = trust_info(hip_lib, M)
        assert info[2] >= 1 and info[2] > fired and info[0] == 0 and lattice_of(s, hip_lib) == (0, 0), info
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))             # trust returns

        for k in range(9):                                           # NaN / inf coordinates
            check_oracle(step(s, bad), bad)
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))
        check_oracle(step(s, LATTICE), LATTICE, lattice_oracle())


def test_a_backward_capable_plan_under_trust(hip_lib):
    """means / values / conics require grad: the plan holds tile lists and wide masks; the trusted build's outputs are
    the verified build's bit for bit, its gradients the verified build's up to the order of the backward's atomic sums
    (the bar tests/test_forward_only_gpu.py sets for two builds of the same inputs)."""
    from diff_gaussian_sampling import GaussianSampler
    t, _ = gaussians()
    gen = torch.Generator().manual_seed(47)
    rs = [(torch.rand(sh, generator=gen) * 2 - 1).cuda() for sh in ((M, 1), (M, 2, 1), (M, 2, 2, 1))]
    s = GaussianSampler(False, backend="binned", fuse="all", reuse_samples=False)

    def run():
        leaves = [t[k].clone().requires_grad_(True) for k in ("means", "values", "conics")]
        p = torch.as_tensor(LATTICE, dtype=torch.float32, device="cuda")
        s.preprocess(leaves[0], leaves[1], None, leaves[2], p)
        assert not s._plan.forward_only
        outs = s.sample(ORDERS)
        grads = torch.autograd.grad(sum((o * r).sum() for o, r in zip(outs, rs)), leaves)
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], grads

    with env(PIGS_LATTICE_TRUST="1"):
        for _ in range(96):
            before = trust_info(hip_lib, M)
            got = run()
            if trust_info(hip_lib, M)[1] == before[1] + 1:
                break
        assert trust_info(hip_lib, M)[1] == before[1] + 1, "no trusted build of a full plan"
    with env(PIGS_LATTICE_TRUST="0"):
        before = trust_info(hip_lib, M)
        want = run()
        assert trust_info(hip_lib, M)[1] == before[1]
    for a, b in zip(got[0], want[0]):
        assert torch.equal(a, b)
    check_oracle(got[0], LATTICE, lattice_oracle())
    for x, y in zip(got[1], want[1]):
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())


@pytest.mark.parametrize("host", ["native", "ctypes"])
def test_both_hosts(hip_lib, host):
    """Neither host knows about trust: each asks for a cold build as ever and gets the same outputs either way."""
    s = make_sampler(host)
    with env(PIGS_LATTICE_TRUST="1"):
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))
        step(s, LATTICE)                 # (this sampler's own plan workspaces are recycled ones from here on)
        step(s, LATTICE)
        trusted, verified = trusted_and_verified(s, hip_lib, LATTICE)
        assert lattice_of(s, hip_lib) == (64, 64)
    for a, b in zip(trusted, verified):
        assert torch.equal(a, b)
    check_oracle(trusted, LATTICE, lattice_oracle())


def test_a_capture_is_never_trusted(hip_lib):
    """A preprocess + sample recorded into a graph while the memory would trust an eager build keeps the verified chain
    (a graph outlives the moment's memory): no trusted build is counted, and its replay is the eager step's result."""
    t, _ = gaussians()
    s = make_sampler()
    p = torch.as_tensor(LATTICE, dtype=torch.float32, device="cuda")

    def run():
        with torch.no_grad():
            s.preprocess(t["means"], t["values"], None, t["conics"], p)
            return s.sample(ORDERS)

    with env(PIGS_LATTICE_TRUST="1"):
        until_trusted(s, hip_lib, LATTICE, 96, (64, 64))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):           # warm up on the capture stream: its plan workspaces are recycled ones
                eager = [o.clone() for o in run()]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        before = trust_info(hip_lib, M)
        assert before[0] == 1 and before[1] >= 1
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = run()
        graph.replay()
        torch.cuda.synchronize()
        after = trust_info(hip_lib, M)
        assert after[1] == before[1], (before, after)
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    check_oracle(outs, LATTICE, lattice_oracle())
