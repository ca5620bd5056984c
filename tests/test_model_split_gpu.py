"""GPU: the second half of Model.forward(t, dt, split=True) through the HIP operators -- split_criterion, split_gaussians,
refine_index, build_covariances, advance_gaussians in front -- against a RECORDED forward of the reference:
tests/golden/model_pn_split/*.npz (tools/gen_model_split.py).  Only the fixtures are read; every comparison is
tests/test_model_split.py's hold_chain, whose bars that file shows to catch eight deliberate mistakes.

    pieces     each operator from the inputs the reference recorded for it (rounded to the dtype): split_criterion gives the
               recorded split, its metric lies within BAND of the quantile (float32) / 1e-11 of its scale (float64) of the
               recorded one; prune then split give out/ -- every copy and u / 2 bit for bit, the children at BAR of
               tests/test_refine_gpu.py; the covariance builders on the result give out/ at the bar of
               tests/test_covariances_gpu.py
    chain      INTEGRATION.md section 4 from in/ and the deltas: advance_gaussians (with the wrap), the prune line,
               build_covariances, split_criterion, split_gaussians, the flags through source / child; the decisions exact,
               the arrays at advance's bar (tests/test_advance_gpu.py) on top of the pieces'
    one call   refine_index / split_gaussians with keep AND split in one call: the rows of the two-call route, bit for bit

Samplers: float32 dense and binned, float64 dense, on both hosts; NOT periodic, for NAVIER_STOKES as well: the stand-in
that served the reference sums no images, and the wrap belongs to the update alone.  N = 117 ... 149.
Each case prints its worst error over its bar.

MEASURED (MI355X), worst over the fixtures, in units of the bar: split_criterion's metric 0.0057 dense / 0.021 binned in
float32 (bar 2e-4 of the quantile), 0.0003 in float64 (bar 1e-11 of its scale), its three fields 0.029 (bar 1e-5 of scale); the
children of prune-then-split 0.30 float32 / 0.0018 float64; the covariance builders 0.24 / 0.50; the whole chain 0.031
float32 (the previous field), 0.00016 float64 (the metric).  Every keep and split decision was the recorded one: no band row
exists in the fixtures, so none was left out.
"""
import types

import numpy as np
import pytest
import torch

import test_covariances_gpu as tcov
from test_model_split import CHAIN, FIXTURES, PIECES, PRUNE_NORM, STATE, fixture, hold_chain, worst

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "float64": torch.float64}
SAMPLERS = [(dtype, backend, host) for dtype, backend in (("float32", "dense"), ("float32", "binned"), ("float64", "dense"))
            for host in ("native", "ctypes")]
SAMPLER_IDS = ["-".join(s) for s in SAMPLERS]


@pytest.fixture(scope="module")
def refine(hip_lib):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from pigs_amd import refine
    return refine


def dev(a, dtype=None):
    return torch.tensor(np.array(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def make_sampler(backend, host_name):
    from diff_gaussian_sampling import GaussianSampler
    return GaussianSampler(True, backend=backend, host=host_name)


def criterion_with_stats(refine, sampler, cur, prev, boundary_mask):
    """split_criterion, then the three fields and the metric behind its mask: the sampler is left bound to the last pass
    (the previous Gaussians at the current means), the first pass is run again.  cur / prev: (means, u, covariances, conics)"""
    mask = refine.split_criterion(sampler, *cur, *prev, boundary_mask)
    n, c = cur[1].shape
    assert mask.dtype == torch.bool and mask.shape == (n,)
    prev_sample_u = sampler.sample_gaussians()
    ones = torch.ones((n, 1), dtype=cur[1].dtype, device="cuda")
    if refine._one_pass(sampler, n, c):
        sampler.preprocess(cur[0], torch.cat((cur[1], ones), -1), cur[2], cur[3], cur[0])
        both = sampler.sample_gaussians()
        sample_u, density = both[:, :c], both[:, c:]
    else:
        sampler.preprocess(cur[0], cur[1], cur[2], cur[3], cur[0])
        sample_u = sampler.sample_gaussians()
        sampler.preprocess(cur[0], ones, cur[2], cur[3], cur[0])
        density = sampler.sample_gaussians()
    again, metric, _ = refine.split_mask(sample_u, prev_sample_u, density, boundary_mask, return_stats=True)
    assert torch.equal(again, mask)
    return mask, host(metric), tuple(host(f) for f in (sample_u, density, prev_sample_u))


def flags_through(fx, dtype, *maps):
    """boundaries and boundary_mask of in/ through (source, child) of every call in turn: the children 0 and True"""
    boundaries, mask = dev(fx["in/boundaries"], dtype), dev(fx["in/boundary_mask"])
    for source, child in maps:
        fresh = (child >= 0)[:, None]
        boundaries = torch.where(fresh, torch.zeros_like(boundaries[:1]), boundaries.index_select(0, source))
        mask = torch.where(fresh, torch.ones_like(mask[:1]), mask.index_select(0, source))
    return boundaries, mask


# ---- pieces ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,backend,host_name", SAMPLERS, ids=SAMPLER_IDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_split_criterion_on_the_recorded_gaussians(refine, name, dtype, backend, host_name):
    from pigs_amd.covariances import build_covariances
    fx, dt = fixture(name), DTYPES[dtype]
    cur = tuple(dev(fx["pruned/" + k], dt) for k in ("means", "u", "covariances", "conics"))
    prev = (dev(fx["in/means"], dt), dev(fx["in/u"], dt)) + tuple(build_covariances(dev(fx["in/scaling"], dt), dev(fx["in/transforms"], dt)))
    free = dev(fx["in/boundary_mask"][fx["keep"]])
    mask, metric, fields = criterion_with_stats(refine, make_sampler(backend, host_name), cur, prev, free)
    got = types.SimpleNamespace(split=host(mask), metric=metric, fields=fields)
    fig = hold_chain(got, fx, PIECES[dtype])
    print(f"[figure] split_criterion {name} {dtype} {backend} {host_name}: split exact, worst error / bar {worst(fig)}; metric "
          f"{fig['metric']:.3g} of its bar")


def two_calls(refine, fx, dt):
    state = [dev(fx["updated/" + k], dt) for k in ("means", "scaling", "transforms", "u")]
    p = refine.split_gaussians(*state, None, dev(fx["keep"]))
    r = refine.split_gaussians(p.means, p.scaling, p.transforms, p.values, dev(fx["split"]))
    return state, p, r


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_prune_then_split_on_the_recorded_update(refine, name, dtype):
    from pigs_amd.covariances import build_covariances
    fx, dt = fixture(name), DTYPES[dtype]
    state, p, r = two_calls(refine, fx, dt)
    assert (p.child == -1).all() and torch.equal(p.source, torch.nonzero(dev(fx["keep"])).squeeze(-1))
    boundaries, mask = flags_through(fx, dt, (p.source, p.child), (r.source, r.child))
    cov, con = build_covariances(p.scaling, p.transforms)
    got = types.SimpleNamespace(means=host(r.means), u=host(r.values), scaling=host(r.scaling), transforms=host(r.transforms),
                                boundaries=host(boundaries), boundary_mask=host(mask),
                                pruned={"means": host(p.means), "u": host(p.values), "covariances": host(cov), "conics": host(con)})
    fig = hold_chain(got, fx, PIECES[dtype])
    fresh = r.child >= 0
    assert torch.equal(r.values[fresh], 0.5 * p.values.index_select(0, r.source)[fresh])
    print(f"[figure] prune, split {name} {dtype}: copies and u / 2 bit for bit, children {fig['children']:.3g} of their bar")


def hold_covariances(what, dtype, got, want, single):
    """tests/test_covariances_gpu.py's bar, element by element against the recording: float64 1e-12 of the element,
    float32 4 err_torch32 + 1e-6 of the element; returns the worst err / bound"""
    figure = 0.0
    for k, name in enumerate(("covariances", "conics", "full_covariances", "full_conics")):
        g, w = got[k].astype(np.float64).reshape(want[k].shape), want[k]
        err = np.abs(g - w)
        assert np.isfinite(g).all(), f"{what} {name}: not finite"
        if dtype == "float64":
            bound = 1e-12 * np.abs(w)
        else:
            err_t = np.abs(single[k].reshape(w.shape) - w)
            bound = 4.0 * np.where(np.isfinite(err_t), err_t, np.inf) + 1e-6 * np.abs(w)
        exact = (bound == 0) & (err == 0)
        ratio = np.where(exact, 0.0, err / np.where(bound == 0, 1e-300, bound))
        figure = max(figure, float(ratio.max()))
        assert ratio.max() <= 1.0, f"{what} {name}: {ratio.max():.3g} x its bound"
    return figure


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_covariance_builders_on_the_split_rows(refine, name, dtype):
    from pigs_amd import covariances
    fx, dt = fixture(name), DTYPES[dtype]
    _, _, r = two_calls(refine, fx, dt)
    cov, con = covariances.build_covariances(r.scaling, r.transforms)
    full_cov, full_con = covariances.build_full_covariances(r.scaling, r.transforms)
    assert torch.equal(full_cov.reshape(-1, 4), cov[:, [0, 1, 1, 2]]) and torch.equal(full_con.reshape(-1, 4), con[:, [0, 1, 1, 2]])
    single = None
    if dtype == "float32":
        flat = [host(x).astype(np.float64) for x in tcov.torch_chain(r.scaling, r.transforms)]
        single = flat + [x[:, [0, 1, 1, 2]] for x in flat]
    want = [fx["out/" + k] for k in ("covariances", "conics", "full_covariances", "full_conics")]
    figure = hold_covariances(f"{name} {dtype}", dtype, [host(x) for x in (cov, con, full_cov, full_con)], want, single)
    print(f"[figure] covariance builders on the split rows, {name} {dtype}: worst err / bound {figure:.3g}")


# ---- the whole chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,backend,host_name", SAMPLERS, ids=SAMPLER_IDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_whole_chain_from_the_incoming_state(refine, name, dtype, backend, host_name):
    """INTEGRATION.md section 4, 'Model.forward(split=True)', line for line, behind advance_gaussians"""
    from pigs_amd import advance_gaussians
    from pigs_amd.covariances import build_covariances, build_full_covariances
    fx, dt = fixture(name), DTYPES[dtype]
    means, u, scaling, transforms = (dev(fx["in/" + k], dt) for k in STATE)
    boundaries, boundary_mask = dev(fx["in/boundaries"], dt), dev(fx["in/boundary_mask"])
    prev = (means, u) + tuple(build_covariances(scaling, transforms))          # in the loop: the last step's out.covariances
    wrap = tuple(fx["wrap"].tolist()) or None
    out = advance_gaussians(means, u, scaling, transforms, dev(fx["deltas"], dt), boundary_mask, wrap=wrap)
    got = types.SimpleNamespace(updated={k: host(getattr(out, k)) for k in STATE})

    keep = (torch.norm(torch.abs(out.u), dim=-1) > PRUNE_NORM) | ~boundary_mask.squeeze(-1)          # :703-704
    p = refine.split_gaussians(out.means, out.scaling, out.transforms, out.u, None, keep)            # :705-714
    boundary_mask, boundaries = boundary_mask.index_select(0, p.source), boundaries.index_select(0, p.source)
    cov, con = build_covariances(p.scaling, p.transforms)
    got.keep = host(keep)
    got.pruned = {"means": host(p.means), "u": host(p.values), "covariances": host(cov), "conics": host(con)}

    indices, got.metric, got.fields = criterion_with_stats(refine, make_sampler(backend, host_name),
                                                           (p.means, p.values, cov, con), prev, boundary_mask)
    got.split = host(indices)

    r = refine.split_gaussians(p.means, p.scaling, p.transforms, p.values, indices)                  # :764
    fresh = (r.child >= 0)[:, None]
    boundaries = torch.where(fresh, torch.zeros_like(boundaries[:1]), boundaries.index_select(0, r.source))
    boundary_mask = torch.where(fresh, torch.ones_like(boundary_mask[:1]), boundary_mask.index_select(0, r.source))
    cov, con = build_covariances(r.scaling, r.transforms)
    full_cov, full_con = build_full_covariances(r.scaling, r.transforms)
    got.means, got.u, got.scaling, got.transforms = host(r.means), host(r.values), host(r.scaling), host(r.transforms)
    got.boundaries, got.boundary_mask = host(boundaries), host(boundary_mask)
    got.covariances, got.conics, got.full_covariances, got.full_conics = host(cov), host(con), host(full_cov), host(full_con)
    assert torch.equal(r.values[fresh[:, 0]], 0.5 * p.values.index_select(0, r.source)[fresh[:, 0]])
    fig = hold_chain(got, fx, CHAIN[dtype])
    print(f"[figure] whole chain {name} {dtype} {backend} {host_name}: keep and split exact, worst error / bar {worst(fig)}; "
          f"metric {fig['metric']:.3g}, children {fig['children']:.3g}")


# ---- prune and split in one call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_one_call_gives_the_rows_of_two(refine, name, dtype):
    """INTEGRATION.md's one-read-back route: keep and split over the SAME N rows in one call"""
    fx, dt = fixture(name), DTYPES[dtype]
    state, p, r = two_calls(refine, fx, dt)
    whole = np.zeros(len(fx["keep"]), bool)
    whole[np.flatnonzero(fx["keep"])[fx["split"]]] = True
    one = refine.split_gaussians(*state, dev(whole), dev(fx["keep"]))
    for a, b in zip(one[:4], r[:4]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert torch.equal(one.source, p.source.index_select(0, r.source)) and torch.equal(one.child, r.child)
    source, child = refine.refine_index(dev(fx["keep"]), dev(whole))
    assert torch.equal(source, one.source) and torch.equal(child, one.child)
    boundaries, mask = flags_through(fx, dt, (source, child))
    got = types.SimpleNamespace(means=host(one.means), u=host(one.values), scaling=host(one.scaling),
                                transforms=host(one.transforms), boundaries=host(boundaries), boundary_mask=host(mask))
    fig = hold_chain(got, fx, PIECES[dtype])
    print(f"[figure] one call {name} {dtype}: the rows of two calls bit for bit; children {fig['children']:.3g} of their bar")
