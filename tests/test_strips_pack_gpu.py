"""GPU: the pack of a build that keeps the caller's order (plan_build.h, gauss_pack_part) forms the records from the
registers of its one load round trip and writes what a plan of strips reads -- records, strip and super-strip boxes, the
way back -- and no `gbox` (the walk through the cells alone reads it).

Shapes: a 64 x 64 lattice of points (index-tiled, so a strips build and a build through the cells group the same points)
over N = 4 096 lattice Gaussians (whole strips and super-strips) and N = 4 096 + 17 (a ragged last strip of one Gaussian
in a ragged last super-strip of 17), one and two channels, full and forward-only plans.  Forward orders 0-2 and the
backward against the oracle at the bar of tests/test_strips_gpu.py (check_case, gradients within the accumulation
bound); the group lists entry for entry against a build under PIGS_GAUSS_STRIPS=0; one case with a NaN conic."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle
from pigs_amd import synthetic
from test_binned_gpu import TOL, check_case, dev32, random_gaussians, rel
from test_lattice_gpu import grid
from test_plan_lists_gpu import lattice_of, read_plan, strips_of

pytestmark = pytest.mark.gpu
ORDERS = (0, 1, 2)
POINTS = grid(64, 64, lo=(-1.0, -1.0), hi=(1.0, 1.0)).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def Sampler(hip_lib):
    from diff_gaussian_sampling import GaussianSampler
    return GaussianSampler


@functools.lru_cache(maxsize=None)
def gaussians(N, c):
    """64 x 64 lattice Gaussians (kappa = 0.5) and, behind them, N - 4 096 small ones anywhere; float32-rounded"""
    gs = synthetic.lattice_gaussians(64, 64, 0.5, seed=2, c=c)
    means, con, values = (gs[k].float().double().numpy() for k in ("means", "conics", "values"))
    if N > 4096:
        m, k, v = random_gaussians(np.random.default_rng(67), N - 4096, c)
        means, con, values = np.concatenate((means, m)), np.concatenate((con, k)), np.concatenate((values, v))
    return tuple(a.astype(np.float32).astype(np.float64) for a in (means, con, values))


@functools.lru_cache(maxsize=None)
def oracle_forward(N, c):
    means, con, values = gaussians(N, c)
    return c_oracle.forward(means, con, values, POINTS, orders=ORDERS)


def forward_only_step(Sampler, means, con, values):
    s = Sampler(False, backend="binned", fuse="all")
    with torch.no_grad():
        s.preprocess(dev32(means), dev32(values), None, dev32(con), dev32(POINTS))
        outs = [o.clone() for o in s.sample(ORDERS)]
    torch.cuda.synchronize()
    assert s._plan.forward_only
    return s, outs


def full_plan(Sampler, means, con, values):
    t = [dev32(a).requires_grad_(True) for a in (means, values, con)]
    s = Sampler(True, backend="binned", fuse="none")
    s.preprocess(t[0], t[1], None, t[2], dev32(POINTS))
    s.sample(ORDERS)
    torch.cuda.synchronize()
    assert not s._plan.forward_only
    return s


def group_lists(plan, hip_lib):
    """tile modes and, per tile and group, the CALLER's indices of the listed Gaussians, sorted"""
    hdr, tlist, glist, g2o = read_plan(plan, hip_lib)
    mode = hdr[:, 0] >> 30
    assert np.isin(mode, (0, 2)).all(), np.bincount(mode, minlength=4)      # tile list + group lists, or group lists alone
    ng = hdr[:, 1:5]
    return mode, [[np.sort(g2o[glist[t, g, :ng[t, g]]].astype(np.int64)) for g in range(4)] for t in range(hdr.shape[0])]


def same_group_lists(strips_plan, cells_plan, hip_lib):
    assert strips_of(strips_plan, hip_lib) == 1 and strips_of(cells_plan, hip_lib) == 0
    assert lattice_of(strips_plan, hip_lib) == lattice_of(cells_plan, hip_lib) == (64, 64)      # the same points per group
    ms, ls = group_lists(strips_plan, hip_lib)
    mc, lc = group_lists(cells_plan, hip_lib)
    assert np.array_equal(ms, mc)
    total = 0
    for t in range(len(ls)):
        for g in range(4):
            assert np.array_equal(ls[t][g], lc[t][g]), (t, g, ls[t][g], lc[t][g])
            total += len(ls[t][g])
    assert total > 0
    return ls


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("N", [4096, 4096 + 17])
def test_full_plans(Sampler, hip_lib, monkeypatch, N, c):
    means, con, values = gaussians(N, c)
    monkeypatch.setenv("PIGS_GAUSS_STRIPS", "1")
    s = check_case(Sampler, means, con, values, POINTS, orders=ORDERS, gtol="bound")
    assert not s._plan.forward_only
    g2o = read_plan(s._plan, hip_lib)[3]
    assert np.array_equal(g2o, np.arange(N))      # the way back: plan_unpermute_kernel and the aggregation read it
    monkeypatch.setenv("PIGS_GAUSS_STRIPS", "0")
    cells = full_plan(Sampler, means, con, values)
    same_group_lists(s._plan, cells._plan, hip_lib)


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("N", [4096, 4096 + 17])
def test_forward_only_plans(Sampler, hip_lib, monkeypatch, N, c):
    means, con, values = gaussians(N, c)
    exp = oracle_forward(N, c)
    monkeypatch.setenv("PIGS_GAUSS_STRIPS", "1")
    s, outs = forward_only_step(Sampler, means, con, values)
    for o in ORDERS:
        assert outs[o].shape == exp[o].shape
        assert rel(outs[o], exp[o]) < TOL, (o, rel(outs[o], exp[o]))
    monkeypatch.setenv("PIGS_GAUSS_STRIPS", "0")
    cells, _ = forward_only_step(Sampler, means, con, values)
    same_group_lists(s._plan, cells._plan, hip_lib)


def test_a_nan_conic(Sampler, hip_lib, monkeypatch):
    """Half extents that are no number make the Gaussian's strip and super-strip reach everywhere: the Gaussian is a
    candidate of every tile, as it is through the cells (top level, a box without bounds), and the exact test lists it
    in every group.  Lists and outputs are those of the build through the cells; the other Gaussians' sums stand
    wherever that build's are numbers."""
    means, con, values = (a.copy() for a in gaussians(4096 + 17, 1))
    bad = 1000
    con[bad, 0] = np.nan
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PIGS_GAUSS_STRIPS", mode)
        got[mode] = forward_only_step(Sampler, means, con, values)
    lists = same_group_lists(got["1"][0]._plan, got["0"][0]._plan, hip_lib)
    assert all((lists[t][g] == bad).any() for t in range(len(lists)) for g in range(4))
    for a, b in zip(got["1"][1], got["0"][1]):
        nan = torch.isnan(b)
        assert torch.equal(torch.isnan(a), nan)
        if bool((~nan).any()):
            assert rel(a[~nan], b[~nan].cpu().double().numpy()) < 2e-6      # (tests/test_strips_gpu.py, strips against cells)
