"""CPU: the second half of Model.forward(t, dt, split=True) -- the prune, the criterion, the split -- held to a RECORDED
forward of the reference: tests/golden/model_pn_split/*.npz (tools/gen_model_split.py).  No GPU call is made here.

Until these fixtures the checkers of that half (refine_oracle and reference_split_restated of tests/test_refine.py,
criterion_oracle of tests/test_criterion.py, the recipe of INTEGRATION.md section 4) were held only to the maintainers' own
reading of model_pn.py:703-764 and :578-610.  Here the reading meets what the reference itself produced:

    fixture          the conditions the generator promised hold on the committed files (rows split and pruned, the margins)
    float64 chain    the recipe composed from the float64 checkers -- prune line, oracle/covariances_numpy, oracle/dense_numpy,
                     criterion_oracle, refine_oracle, the flags through source / child -- reproduces the recording at
                     CHAIN[float64]: decisions exact, copies and u / 2 bit for bit, children 1e-12 lambda_max
    hold_chain()     the one function that does every comparison; tests/test_model_split_gpu.py imports it
    discrimination   each of eight deliberate mistakes planted in the float64 chain misses CHAIN[float32], the loosest bar
                     the GPU tests use, on every fixture where the mistake can show at all

A child pair is compared after the pair-order canonicalisation of tests/test_refine.py (e_x > 0, or e_x = 0 and e_y > 0): the
reference's order follows the sign LAPACK's eig returns, this project's the convention; the set of Gaussians is the same.

MEASURED, the factor by which each mistake misses CHAIN[float32] (smallest over the fixtures it shows on; inf: a decision,
a flag or a row count differs): values_not_halved 1.1e+04 (u), children_in_front 2.1e+05 (conics; inf on the flags where
there are boundary rows), prune_without_boundary_clause inf (keep), density_without_min_shift 3.7e+03 (metric),
quantile_per_channel inf (split), mask_without_boundary_product inf (split), previous_pruned 1.3e+03 (metric, the previous
field), children_mask_inherited inf, but only on top of mask_without_boundary_product: see test_the_bar_discriminates.
The unmistaken float64 chain stands at 2e-3 of PIECES[float64] at the most (a child, navier_stokes).

WHAT THE RECORDING SHOWED.  Nothing to correct: the maintainers' reading of those lines, and the recipe of INTEGRATION.md,
agree with the recorded forward in every decision, row, flag and order (beyond the documented pair order).  And one fact
about the model itself: in neither set-up that tools/gen_model_step.py records does a boundary row ever reach the quantile
(40 seeds of DIFFUSION; NAVIER_STOKES has no boundary row), so there the product with boundary_mask decides nothing and no
recording could tell whether it is taken.  The third fixture, diffusion_frozen, freezes a seeded quarter of the lattice as
boundary rows (an input, recorded), one of which exceeds the quantile and is NOT split.
"""
import collections
import os
import types

import numpy as np
import pytest

from test_criterion import BAND, BAND_ROWS, criterion_oracle
from test_refine import canonical_sign, eigh_displacement, reference_split_restated, refine_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_pn_split")
FIXTURES = ("diffusion", "navier_stokes", "diffusion_frozen")
STATE = ("means", "u", "scaling", "transforms")
COVARIANCES = ("covariances", "conics", "full_covariances", "full_conics")
PRUNE_NORM, PRUNE_MARGIN = 0.01, 1e-4
MAX_BYTES = 430_000

# state: of each tensor's scale, 0 = bit for bit (in the dtype of what is compared); children: of lambda_max, on top of
# `state` of the means' scale; metric: of the recorded quantile ("quantile") or of the metric's scale ("scale"); fields and
# covariances: of each tensor's scale / of the largest entry of each Gaussian's matrix (None: not compared)
Bar = collections.namedtuple("Bar", "state children metric metric_unit fields covariances")
# from recorded inputs (rounded to the dtype): copies and u / 2 exact, the children at BAR of tests/test_refine_gpu.py
PIECES = {"float32": Bar(0.0, 1e-5, BAND, "quantile", 1e-5, None), "float64": Bar(0.0, 1e-12, 1e-11, "scale", 1e-11, 1e-12)}
# through advance_gaussians first: its bar (tests/test_advance_gpu.py) on every array
CHAIN = {"float32": Bar(1e-5, 1e-5, BAND, "quantile", 1e-5, 1e-5), "float64": Bar(1e-11, 1e-12, 1e-11, "scale", 1e-11, 1e-11)}

_fixtures = {}


def fixture(name):
    """the arrays of a fixture, loaded once and shared; never written"""
    if name not in _fixtures:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            fx = {k: z[k] for k in z.files}
        for a in fx.values():
            a.setflags(write=False)
        _fixtures[name] = fx
    return _fixtures[name]


def band_rows(fx):
    """the rows with a metric entry within BAND of the quantile: the only ones a mask comparison may leave out"""
    return (np.abs(fx["metric"] - fx["quantile"]) <= BAND * fx["quantile"]).any(-1)


def scale_of(a):
    return max(float(np.abs(a).max()), 1e-300) if a.size else 1.0


def canonical_pairs(children):
    """[2 n, 2] adjacent pairs (mu - e, mu + e) -> the same pairs with e in the sign convention of test_refine.py"""
    p = np.asarray(children, np.float64).reshape(-1, 2, 2)
    e = 0.5 * (p[:, 1] - p[:, 0])
    flip = (canonical_sign(e) != e).any(-1)
    return np.where(flip[:, None, None], p[:, ::-1], p).reshape(-1, 2)


# ---- the one comparison ---------------------------------------------------------------------------------------------
def chain_figures(got, fx, bar):
    """Every comparison of a result with a fixture, as {name: error / bar}; inf where something exact differs.

    ``got``: a namespace; a field that is absent or None is not compared.  keep [N], split [n_kept] (bool); metric
    [n_kept, c]; fields = (sample_u, density, prev_sample_u); updated = {means, u, scaling, transforms} (the state in front of
    the prune); pruned = {means, u, covariances, conics}; means, u, scaling,
    transforms, boundaries, boundary_mask [N_out, ...]; covariances, conics, full_covariances, full_conics."""
    inf, fig = float("inf"), {}

    def get(name):
        v = getattr(got, name, None)
        return None if v is None else np.asarray(v)

    def close(name, g, want, tol):
        """of the tensor's scale; tol = 0: bit for bit in the dtype of ``g``"""
        if g.size != want.size or len(g) != len(want):
            fig[name] = inf
        elif tol == 0.0:
            fig[name] = 0.0 if np.array_equal(g.reshape(want.shape), want.astype(g.dtype)) else inf
        else:
            fig[name] = float(np.abs(g.reshape(want.shape).astype(np.float64) - want).max()) / (tol * scale_of(want))

    def per_matrix(name, g, want, tol):
        if g.size != want.size or len(g) != len(want):
            fig[name] = inf
            return
        w = want.reshape(len(want), -1)
        err = np.abs(g.reshape(w.shape).astype(np.float64) - w)
        fig[name] = float((err / (tol * np.abs(w).max(-1, keepdims=True))).max())

    keep, split = fx["keep"], fx["split"]
    n_kept, n_split = len(split), int(split.sum())
    n_plain = n_kept - n_split
    if get("keep") is not None:
        g = get("keep").astype(bool).reshape(-1)
        fig["keep"] = 0.0 if g.shape == keep.shape and np.array_equal(g, keep) else inf
    if get("split") is not None:
        g = get("split").astype(bool).reshape(-1)
        band = band_rows(fx)
        assert int(band.sum()) <= BAND_ROWS
        fig["split"] = 0.0 if g.shape == split.shape and not ((g != split) & ~band).any() else inf
        if fig["split"] == 0.0 and (g != split).any():
            fig["rows (the split differs inside the band: nothing recorded to compare with)"] = inf
    if get("metric") is not None:
        unit = float(fx["quantile"]) if bar.metric_unit == "quantile" else scale_of(fx["metric"])
        g = get("metric")
        fig["metric"] = (float(np.abs(g.astype(np.float64) - fx["metric"]).max()) / (bar.metric * unit)
                         if g.shape == fx["metric"].shape else inf)
    if getattr(got, "fields", None) is not None and bar.fields is not None:
        for name, g in zip(("sample_u", "density", "prev_sample_u"), got.fields):
            close("field " + name, np.asarray(g), fx["pruned/" + name], bar.fields)
    if getattr(got, "updated", None) is not None:
        for name in STATE:
            close("updated " + name, np.asarray(got.updated[name]), fx["updated/" + name], bar.state)
    if getattr(got, "pruned", None) is not None:
        for name in ("means", "u"):
            close("pruned " + name, np.asarray(got.pruned[name]), fx["pruned/" + name], bar.state)
        if bar.covariances is not None:
            for name in ("covariances", "conics"):
                per_matrix("pruned " + name, np.asarray(got.pruned[name]), fx["pruned/" + name], bar.covariances)
    for name in ("u", "scaling", "transforms"):
        if get(name) is not None:
            close(name, get(name), fx["out/" + name], bar.state)
    if get("means") is not None:
        g, want = get("means"), fx["out/means"]
        if g.shape != want.shape:
            fig["means"] = fig["children"] = inf
        else:
            close("means", g[:n_plain], want[:n_plain], bar.state)
            pruned_s, pruned_t = fx["updated/scaling"][keep], fx["updated/transforms"][keep]
            lam = np.repeat(eigh_displacement(pruned_s[split], pruned_t[split, 0])[1], 2)[:, None]
            err = np.abs(canonical_pairs(g[n_plain:]) - canonical_pairs(want[n_plain:]))
            fig["children"] = float((err / (bar.children * lam + bar.state * scale_of(want))).max()) if n_split else 0.0
    for name in ("boundaries", "boundary_mask"):
        if get(name) is not None:
            g, want = get(name), fx["out/" + name]
            fig[name] = 0.0 if g.size == want.size and np.array_equal(g.reshape(want.shape).astype(want.dtype), want) else inf
    if bar.covariances is not None:
        for name in COVARIANCES:
            if get(name) is not None:
                per_matrix(name, get(name), fx["out/" + name], bar.covariances)
    return fig


def hold_chain(got, fx, bar):
    """every comparison of chain_figures within its bar; returns the figures"""
    fig = chain_figures(got, fx, bar)
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, "outside the bar (error / bar): " + ", ".join(f"{k} {v:.3g}" for k, v in bad.items())
    return fig


def worst(fig):
    name = max(fig, key=fig.get)
    return f"{fig[name]:.3g} ({name})"


# ---- the float64 chain ----------------------------------------------------------------------------------------------
MISTAKES = {          # mistake -> the fixtures on which it can show
    "values_not_halved": FIXTURES,
    "children_in_front": FIXTURES,
    "prune_without_boundary_clause": ("diffusion", "diffusion_frozen"),      # navier_stokes has no boundary row
    "density_without_min_shift": FIXTURES,
    "quantile_per_channel": ("navier_stokes",),                               # c = 1 has one channel
    "mask_without_boundary_product": ("diffusion_frozen",),                   # the only one with a boundary row above the quantile
    "previous_pruned": FIXTURES,
    "children_mask_inherited": ("diffusion_frozen",),                         # on top of the one before: see the test
}


def full_conics(scaling, transforms):
    from oracle import covariances_numpy
    cov, con = covariances_numpy.build_covariances(scaling, transforms)
    return cov, con, con[:, [0, 1, 1, 2]].reshape(-1, 2, 2)


def float64_chain(fx, mistakes=()):
    """INTEGRATION.md section 4, 'Model.forward(split=True)', from the recorded update on, composed from the float64
    checkers.  ``mistakes``: names of MISTAKES planted on purpose."""
    from oracle import dense_numpy
    wrong = set(mistakes)
    assert wrong <= set(MISTAKES)
    got = types.SimpleNamespace()
    means, u, scaling, transforms = (fx["updated/" + k] for k in STATE)
    free, boundaries = fx["in/boundary_mask"].reshape(-1), fx["in/boundaries"].reshape(-1)
    c = u.shape[1]
    # the prune
    got.keep = np.linalg.norm(np.abs(u), axis=-1) > PRUNE_NORM
    if "prune_without_boundary_clause" not in wrong:
        got.keep = got.keep | ~free
    p = refine_oracle(means, scaling, transforms, u, got.keep, None)
    free, boundaries = free[p.source], boundaries[p.source]
    cov, con, full = full_conics(p.scaling, p.transforms)
    got.pruned = {"means": p.means, "u": p.values, "covariances": cov, "conics": con}
    # the criterion: the current field and the density at the kept means, the previous (unpruned, pre-update) field there
    both = dense_numpy.forward(p.means, full, np.concatenate((p.values, np.ones((len(p.means), 1))), -1), p.means, orders=(0,))[0]
    old = {k: fx["in/" + k][got.keep] if "previous_pruned" in wrong else fx["in/" + k] for k in STATE}
    prev = dense_numpy.forward(old["means"], full_conics(old["scaling"], old["transforms"])[2], old["u"], p.means, orders=(0,))[0]
    got.fields = (both[:, :c], both[:, c:], prev)
    density = both[:, c]
    o = criterion_oracle(both[:, :c], prev, density, None)
    if "density_without_min_shift" in wrong:                      # w = 1 - D / D.max()
        o.metric = (both[:, :c] - prev) ** 2 * (1.0 - density / density.max())[:, None]
        o.quantile = np.quantile(o.metric, 0.98)
    quantile = np.quantile(o.metric, 0.98, axis=0) if "quantile_per_channel" in wrong else o.quantile
    got.metric = o.metric
    got.split = (o.metric > quantile).any(-1)
    if "mask_without_boundary_product" not in wrong:
        got.split = got.split & free
    # the split
    r = refine_oracle(p.means, p.scaling, p.transforms, p.values, None, got.split,
                      value_scale=1.0 if "values_not_halved" in wrong else 0.5)
    order = np.arange(len(r.source))
    if "children_in_front" in wrong:
        order = np.concatenate((order[r.child >= 0], order[r.child < 0]))
    fresh = (r.child >= 0)[order]
    got.means, got.u, got.scaling = r.means[order], r.values[order], r.scaling[order]
    got.transforms = r.transforms[order][:, None]
    got.boundaries = np.where(fresh, 0.0, boundaries[r.source[order]])
    got.boundary_mask = free[r.source[order]] if "children_mask_inherited" in wrong else fresh | free[r.source[order]]
    got.covariances, got.conics, got.full_conics = full_conics(got.scaling, got.transforms)
    got.full_covariances = got.covariances[:, [0, 1, 1, 2]].reshape(-1, 2, 2)
    return got


# ---- the fixtures themselves ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_keeps_what_the_generator_promised(name):
    fx = fixture(name)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= MAX_BYTES
    N, c = fx["in/u"].shape
    keep, split = fx["keep"], fx["split"]
    free = fx["in/boundary_mask"].reshape(-1)
    n_kept, n_split, n_out = int(keep.sum()), int(split.sum()), len(fx["out/means"])
    assert keep.shape == (N,) and split.shape == (n_kept,) and n_out == n_kept + n_split
    assert fx["deltas"].shape == (N, 5 + c) and len(fx["pruned/means"]) == n_kept
    assert fx["wrap"].tolist() == ([-1.0, 1.0] if name == "navier_stokes" else [])
    for k in STATE:
        assert fx["in/" + k].shape == fx["updated/" + k].shape and fx["out/" + k].shape[0] == n_out
        assert np.array_equal(fx["in/" + k][~free], fx["updated/" + k][~free])        # a boundary row does not move
    assert n_split >= (2 if name == "diffusion_frozen" else 3)
    norm = np.linalg.norm(fx["updated/u"], axis=-1)
    small_kept = int(((norm <= PRUNE_NORM) & ~free & keep).sum())
    if name.startswith("diffusion"):
        assert N - n_kept >= 2 and small_kept >= 50
    if name == "navier_stokes":
        assert N - n_kept >= 1 and free.all()
    assert not (np.abs(norm[free] - PRUNE_NORM) <= PRUNE_MARGIN).any()
    band = band_rows(fx)
    assert int(band.sum()) <= BAND_ROWS
    above = (fx["metric"] > fx["quantile"]).any(-1)
    boundary_above = int((above & ~free[keep]).sum())
    assert boundary_above >= (1 if name == "diffusion_frozen" else 0)
    assert np.array_equal(split, above & free[keep]) or band.any()
    nearest = np.abs(fx["metric"] - fx["quantile"]).min() / fx["quantile"]
    print(f"[figure] {name}: seed {int(fx['seed'])}, N in {N}, pruned {N - n_kept}, split {n_split}, N out {n_out}; {small_kept} "
          f"small rows kept through ~boundary_mask; boundary rows above the quantile {boundary_above}; nearest metric entry "
          f"{nearest:.3g} quantiles from the quantile, {int(band.sum())} band rows")


# ---- the float64 checkers reproduce the recording -------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_float64_chain_reproduces_the_recording(name):
    """prune line, criterion_oracle, refine_oracle, the flags through source / child, covariances_numpy: at
    PIECES[float64], every copy and u / 2 bit for bit"""
    fx = fixture(name)
    fig = hold_chain(float64_chain(fx), fx, PIECES["float64"])
    assert {"keep", "split", "metric", "children", "boundary_mask", "boundaries", "full_conics", "pruned conics"} <= set(fig)
    print(f"[figure] {name}: float64 chain, worst error / bar {worst(fig)}; " + ", ".join(f"{k} {v:.2g}" for k, v in fig.items() if v))


@pytest.mark.parametrize("name", FIXTURES)
def test_checkers_piece_by_piece_on_the_recorded_inputs(name):
    """each checker on what the REFERENCE handed on, not on the chain's own intermediate: criterion_oracle on the three
    recorded fields, refine_oracle and reference_split_restated on updated/ with the derived keep and split"""
    fx = fixture(name)
    keep, split = fx["keep"], fx["split"]
    free = fx["in/boundary_mask"].reshape(-1)
    o = criterion_oracle(fx["pruned/sample_u"], fx["pruned/prev_sample_u"], fx["pruned/density"], free[keep])
    got = types.SimpleNamespace(split=o.mask, metric=o.metric)
    whole = np.zeros(len(keep), bool)
    whole[np.flatnonzero(keep)[split]] = True
    state = [np.array(fx["updated/" + k]) for k in ("means", "scaling", "transforms", "u")]
    r = refine_oracle(*state, keep, whole)
    got.means, got.scaling, got.transforms, got.u = r.means, r.scaling, r.transforms, r.values
    fresh = r.child >= 0
    got.boundaries = np.where(fresh, 0.0, fx["in/boundaries"].reshape(-1)[r.source])
    got.boundary_mask = fresh | free[r.source]
    fig = hold_chain(got, fx, PIECES["float64"])
    assert o.quantile == fx["quantile"] or abs(o.quantile - fx["quantile"]) <= 4 * np.spacing(fx["quantile"])
    # prune and split in one call or in two: the same rows
    p = refine_oracle(*state, keep, None)
    two = refine_oracle(p.means, p.scaling, p.transforms, p.values, None, split)
    assert np.array_equal(two.means, r.means) and np.array_equal(p.source[two.source], r.source)
    # the older restatement, on which tests/test_refine.py leans
    m, s, t, v = reference_split_restated(*state, np.array(keep), whole)
    restated = types.SimpleNamespace(means=m, scaling=s, transforms=t, u=v)
    fig_r = hold_chain(restated, fx, PIECES["float64"])
    print(f"[figure] {name}: checkers on recorded inputs, worst error / bar {worst(fig)}; reference_split_restated {worst(fig_r)}")


# ---- the bar discriminates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_the_bar_discriminates(mistake):
    """A mistake planted in the float64 chain misses CHAIN[float32] -- the loosest bar a GPU test uses -- on every fixture
    on which it can show.  children_mask_inherited cannot show on ANY correct chain: the product with boundary_mask
    leaves only free rows in the split, and a free parent's flag IS True.  It is planted on top of
    mask_without_boundary_product, where a boundary row is split, and must move the children's boundary_mask there."""
    factors = []
    for name in MISTAKES[mistake]:
        fx = fixture(name)
        if mistake == "children_mask_inherited":
            base = float64_chain(fx, ("mask_without_boundary_product",))
            wrong = float64_chain(fx, ("mask_without_boundary_product", mistake))
            assert not np.array_equal(base.boundary_mask, wrong.boundary_mask)
            assert np.array_equal(float64_chain(fx, (mistake,)).boundary_mask, fx["out/boundary_mask"].reshape(-1))
        else:
            wrong = float64_chain(fx, (mistake,))
        fig = chain_figures(wrong, fx, CHAIN["float32"])
        with pytest.raises(AssertionError):
            hold_chain(wrong, fx, CHAIN["float32"])
        finite = {k: v for k, v in fig.items() if np.isfinite(v)}
        print(f"[figure] {mistake} on {name}: misses the float32 bar by {worst(fig)}; largest finite factor "
              f"{worst(finite) if finite else 'none'}")
        factors.append(max(fig.values()))
    assert factors and min(factors) > 1.0
    print(f"[figure] {mistake}: smallest factor {min(factors):.3g}")


@pytest.mark.parametrize("name", FIXTURES)
def test_the_unmistaken_chain_passes_the_float32_bar(name):
    fx = fixture(name)
    hold_chain(float64_chain(fx), fx, CHAIN["float32"])
