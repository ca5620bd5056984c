"""CPU: state_loss_terms (pigs_amd/state_loss.py, csrc/state_loss.hip) -- the float64 torch recipe of its eight terms
against the reference's recorded ``Model.compute_loss`` of Problem.TEST (tests/golden/model_pn_state_loss/test.npz, from
tools/gen_state_loss.py), the numpy checker against the recipe's autograd, six planted mistakes, the column order, the
refusals, the C ABI.  No GPU call is made here.

Shared with tests/test_state_loss_gpu.py:
    state_loss_recipe()   the eight terms in torch without a host decision (``where`` and masked sums): the capturable
                          composition, and what the recorded scenes pin
    compose_losses()      pde_loss, bc_loss, conservation_loss from the terms, the penalty and the model's weights
    make_case()           synthetic inputs (float64 numpy holding values of the case's dtype)
    checker_terms()       the eight terms, every sum a math.fsum (exactly rounded: it adds no summation error of its own
                          to the 4-ulp bar of the GPU file)
    checker_grads()       the three input gradients in closed form
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_advance import MASKS, make_mask, scale_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("drift", "wall_low", "wall_high", "dmeans_x", "dmeans_spread", "height_spread", "unit_u", "du_mid")
INPUTS = ("means", "u", "deltas")
WALL, DRIFT = 0.8, 5.0
MISTAKES = ("nonstrict", "cond_by_F", "signs", "spread_by_F", "no_abs", "channel0")


# ---- the recipe: torch, no host decision --------------------------------------------------------------------
def state_loss_recipe(means, u, deltas, mask, wall=WALL, drift=DRIFT, mistake=None):
    """model_pn.py:851-861, 866-876 without ``if torch.any`` and without boolean indexing; ``mask`` torch.bool [N].
    ``mistake`` plants one of MISTAKES (the tests below show that each one is seen)."""
    c = u.shape[1]
    y, dx, dy, du, u0 = means[:, 1], deltas[:, 0], deltas[:, 1], deltas[:, 5:5 + c], u[:, 0]
    zero = torch.zeros((), dtype=means.dtype, device=means.device)

    def total(x, rows):
        return torch.where(rows.reshape((-1,) + (1,) * (x.dim() - 1)), x, zero).sum()
    F = mask.sum().to(means.dtype)
    if mistake == "nonstrict":
        low, high, mid = mask & (y <= -wall), mask & (y >= wall), mask & (y.abs() <= wall)
    else:
        low, high, mid = mask & (y < -wall), mask & (y > wall), mask & (y.abs() < wall)

    def conditional(x, rows, width):
        n = F if mistake == "cond_by_F" else rows.sum().to(means.dtype)
        return torch.where(rows.any(), total(x, rows) / (torch.clamp(n, min=1.0) * width), zero)
    up, down = (-1.0, 1.0) if mistake == "signs" else (1.0, -1.0)
    uu, dd, width = (u[:, :1], du[:, :1], 1) if mistake == "channel0" else (u, du, c)
    mean_dx, mean_dy, mean_y = total(dx, mask) / F, total(dy, mask) / F, total(y, mask) / F
    spread = total((dx - mean_dx) ** 2 + (dy - mean_dy) ** 2, mask) / ((1.0 if mistake == "spread_by_F" else 2.0) * F)
    unit = (u0 if mistake == "no_abs" else u0.abs()) - 1.0
    return torch.stack((total((dy - u0 / drift) ** 2, mask) / F,
                        conditional((uu - up) ** 2, low, width),
                        conditional((uu - down) ** 2, high, width),
                        total(dx ** 2, mask) / F,
                        spread,
                        total((y - mean_y) ** 2, mask) / F,
                        conditional(unit ** 2, mid, 1),
                        conditional(dd ** 2, mid, width)))


def masked_penalty(deltas, mask, c):
    """advance_gaussians' penalty (model_pn.py:878-882) in the same style: [dmeans, dscaling, dtransforms, du]"""
    F = mask.sum().to(deltas.dtype)
    zero = torch.zeros((), dtype=deltas.dtype, device=deltas.device)
    return torch.stack([torch.where(mask[:, None], deltas[:, a:b] ** 2, zero).sum() / (F * (b - a))
                        for a, b in ((0, 2), (2, 4), (4, 5), (5, 5 + c))])


def compose_losses(terms, penalty, w):
    """the three losses of compute_loss for TEST as it returns them; ``w`` maps the model's weight names to numbers"""
    pde = w["pde_weight"] * terms[0]
    bc = w["bc_weight"] * (terms[1] + terms[2])
    conservation = w["conservation_weight"] * (
        w["dmean_weight"] * (terms[3] + terms[4] + terms[5]) + w["du_weight"] * (terms[6] + terms[7])
        + w["dscale_weight"] * penalty[1] + w["dtransform_weight"] * penalty[2])
    return pde, bc, conservation


# ---- the recorded scenes ------------------------------------------------------------------------------------
def load_scenes():
    d = np.load(os.path.join(GOLDEN, "model_pn_state_loss", "test.npz"))
    weights = dict(zip((str(k) for k in d["weight_names"]), (float(v) for v in d["weights"])))
    scenes = []
    for k, kind in enumerate(d["kinds"]):
        prefix = f"s{k}/"
        scene = {name[len(prefix):]: d[name] for name in d.files if name.startswith(prefix)}
        scene["kind"] = str(kind)
        scenes.append(scene)
    return scenes, weights


SCENES, WEIGHTS = load_scenes()
RECORDED_GRADS = ("grad_means", "grad_u", "grad_dmeans", "grad_dscaling", "grad_dtransforms", "grad_du")


def scene_losses(scene, terms_of, device="cpu"):
    """the three losses and the six recorded gradients of one scene, composed behind ``prev + delta * mask``;
    ``terms_of(means, u, deltas, mask)`` is the recipe or the operator"""
    def leaf(a):
        return torch.tensor(a, dtype=torch.float64, device=device, requires_grad=True)
    prev_means, prev_u, deltas = leaf(scene["prev_means"]), leaf(scene["prev_u"]), leaf(scene["deltas"])
    mask = torch.tensor(scene["boundary_mask"], device=device)
    m = mask[:, None].to(torch.float64)
    means, u = prev_means + deltas[:, 0:2] * m, prev_u + deltas[:, 5:6] * m
    losses = compose_losses(terms_of(means, u, deltas, mask), masked_penalty(deltas, mask, 1), WEIGHTS)
    g_means, g_u, g_d = torch.autograd.grad(losses[0] + losses[1] + losses[2], (prev_means, prev_u, deltas))
    got = {"pde_loss": losses[0], "bc_loss": losses[1], "conservation_loss": losses[2], "grad_means": g_means,
           "grad_u": g_u, "grad_dmeans": g_d[:, 0:2], "grad_dscaling": g_d[:, 2:4], "grad_dtransforms": g_d[:, 4:5],
           "grad_du": g_d[:, 5:6], "means": means, "u": u}
    return {k: v.detach().cpu().numpy() for k, v in got.items()}


def test_fixture_covers_every_set():
    kinds = [s["kind"] for s in SCENES]
    assert {"mid", "low", "high", "mixed"} <= set(kinds)
    for s in SCENES:
        low, high, mid = (int(v) for v in s["counts"])
        free = int(s["boundary_mask"].sum())
        assert s["means"].shape == (56, 2) and free == 6 == low + high + mid and not s["boundary_mask"][:50].any()
        assert {"low": low == free, "high": high == free, "mid": mid == free,
                "mixed": max(low, high, mid) < free}[s["kind"]], s["kind"]
        assert s["means"].dtype == np.float64 and s["deltas"].shape == (56, 6)


@pytest.mark.parametrize("k", range(len(SCENES)), ids=[f"{k}-{s['kind']}" for k, s in enumerate(SCENES)])
def test_recipe_is_the_recorded_compute_loss(k):
    """the three losses and every recorded gradient, 1e-12 of each number's scale"""
    scene = SCENES[k]
    got = scene_losses(scene, state_loss_recipe)
    worst = 0.0
    for name in ("means", "u", "pde_loss", "bc_loss", "conservation_loss") + RECORDED_GRADS:
        err = float(np.abs(got[name] - scene[name]).max()) / scale_of(scene[name])
        worst = max(worst, err)
        assert err <= 1e-12, f"scene {k} ({scene['kind']}) {name}: {err:.3g} of its scale"
    print(f"scene {k} ({scene['kind']}, seed {int(scene['seed'])}): worst {worst:.3g} of a number's scale")


# ---- synthetic cases ----------------------------------------------------------------------------------------
def wall_targets(wall, dtype):
    """heights planted exactly on -wall and +wall (in no set) and one ulp either side of each, ``wall`` rounded to dtype"""
    w, inf = dtype(wall), dtype(np.inf)
    return np.array([-w, w, np.nextafter(-w, -inf), np.nextafter(-w, inf), np.nextafter(w, -inf), np.nextafter(w, inf)],
                    dtype=dtype)


def make_case(N, c, seed, mask="all", values="ordinary", heights="all", dtype=np.float64, wall=WALL, drift=DRIFT):
    """means: x U(-1, 1), y U(-1.1, 1.1) (all three sets filled); u N(0, 1) (both signs, some in MID); deltas N(0, sigma)
    with sigma 0.05 (dmeans), 0.3 (dscaling, dtransforms), 0.1 (du).  ``heights``: "all", or "nolow" / "nohigh" / "nomid"
    with that set left empty.  Value families:
        "walls"    the first free rows' heights on wall_targets()
        "naninf"   NaN / +Inf / -Inf in the state and the deltas of every boundary row
        "equal"    every height 0.37          "offset"   dmeans = 100 + 1e-3 N(0, 1)
    Every value is one of ``dtype``, held in float64."""
    rng = np.random.default_rng(seed)
    lo, hi = {"all": (-1.1, 1.1), "nolow": (-0.7, 1.1), "nohigh": (-1.1, 0.7), "nomid": (0.85, 1.1)}[heights]
    y = rng.uniform(lo, hi, N)
    if heights == "nomid":
        y *= rng.choice([-1.0, 1.0], N)
    a = {"means": np.stack((rng.uniform(-1.0, 1.0, N), y), -1), "u": rng.standard_normal((N, c))}
    sigma = np.concatenate(([0.05, 0.05, 0.3, 0.3, 0.3], np.full(c, 0.1)))
    a["deltas"] = rng.standard_normal((N, 5 + c)) * sigma
    m = make_mask(N, mask, rng)
    free, bound = np.flatnonzero(m), np.flatnonzero(~m)
    if values == "equal":
        a["means"][:, 1] = 0.37
    elif values == "offset":
        a["deltas"][:, 0:2] = 100.0 + 1e-3 * rng.standard_normal((N, 2))
    a = {k: v.astype(dtype) for k, v in a.items()}
    if values == "walls":
        t = wall_targets(wall, dtype)
        rows = free[:len(t)]
        a["means"][rows, 1] = t[:len(rows)]
        a["u"][rows, 0] = dtype(0.5) * np.where(np.arange(len(rows)) % 2, -1, 1)      # (|u0| - 1)^2 = 0.25: a row moves a term
    elif values == "naninf":
        bad = np.array([np.nan, np.inf, -np.inf], dtype=dtype)[np.arange(len(bound)) % 3]
        for k in INPUTS:
            a[k][bound] = bad[:, None]
    elif values not in ("ordinary", "equal", "offset"):
        raise ValueError(values)
    case = {k: v.astype(np.float64) for k, v in a.items()}
    case.update(mask=m, c=c, N=N, dtype=dtype, wall=float(wall), drift=float(drift))
    return case


def make_g(seed, dtype=np.float64):
    return np.random.default_rng(seed + 7919).standard_normal(8).astype(dtype).astype(np.float64)


# ---- the checker --------------------------------------------------------------------------------------------
def fsum_sq(x):
    return math.fsum(float(v) * float(v) for v in np.asarray(x).reshape(-1))


def statistics(case):
    """the free rows, the three sets among them (strict, against the wall rounded to the dtype), the three means and
    e = dy - u0 / drift with the division rounded to the dtype"""
    dtype, m = case["dtype"], case["mask"]
    wall = float(dtype(case["wall"]))
    y = case["means"][:, 1]
    with np.errstate(invalid="ignore"):
        low, high, mid = m & (y < -wall), m & (y > wall), m & (np.abs(y) < wall)
    F = int(m.sum())
    dx, dy = case["deltas"][:, 0], case["deltas"][:, 1]
    mean = [math.fsum(x[m]) / F if F else float("nan") for x in (dx, dy, y)]
    with np.errstate(all="ignore"):
        e = dy - (case["u"][:, 0].astype(dtype) / dtype(case["drift"])).astype(np.float64)
    return {"F": F, "low": low, "high": high, "mid": mid, "mean": mean, "e": e, "drift": float(dtype(case["drift"]))}


def checker_terms(case):
    s, c, m = statistics(case), case["c"], case["mask"]
    F, nan = s["F"], float("nan")
    u, du = case["u"], case["deltas"][:, 5:5 + c]
    dx, dy, y = case["deltas"][:, 0], case["deltas"][:, 1], case["means"][:, 1]

    def conditional(x, rows, width):
        n = int(rows.sum())
        return fsum_sq(x[rows]) / (n * width) if n else 0.0
    mdx, mdy, my = s["mean"]
    return np.array([
        fsum_sq(s["e"][m]) / F if F else nan,
        conditional(u - 1.0, s["low"], c),
        conditional(u + 1.0, s["high"], c),
        fsum_sq(dx[m]) / F if F else nan,
        math.fsum([fsum_sq(dx[m] - mdx), fsum_sq(dy[m] - mdy)]) / (2 * F) if F else nan,
        fsum_sq(y[m] - my) / F if F else nan,
        conditional(np.abs(u[:, 0]) - 1.0, s["mid"], 1),
        conditional(du, s["mid"], c)])


def checker_grads(case, g):
    """gradients of <g, terms> with respect to means, u, deltas: the sets, their counts and the means are constants"""
    s, c, m, N = statistics(case), case["c"], case["mask"], case["N"]
    F = s["F"]
    grads = {"means": np.zeros((N, 2)), "u": np.zeros((N, c)), "deltas": np.zeros((N, 5 + c))}
    if not F:
        return grads
    with np.errstate(all="ignore"):
        u, du = case["u"], case["deltas"][:, 5:5 + c]
        dx, dy, y, e = case["deltas"][:, 0], case["deltas"][:, 1], case["means"][:, 1], s["e"]
        mdx, mdy, my = s["mean"]
        n_low, n_high, n_mid = (int(s[k].sum()) for k in ("low", "high", "mid"))
        g_d = np.zeros((N, 5 + c))
        g_d[:, 0] = (2.0 * g[3] * dx + g[4] * (dx - mdx)) / F
        g_d[:, 1] = (2.0 * g[0] * e + g[4] * (dy - mdy)) / F
        if n_mid:
            g_d[:, 5:] = np.where(s["mid"][:, None], 2.0 * g[7] * du / (n_mid * c), 0.0)
        g_u = np.zeros((N, c))
        if n_low:
            g_u += np.where(s["low"][:, None], 2.0 * g[1] * (u - 1.0) / (n_low * c), 0.0)
        if n_high:
            g_u += np.where(s["high"][:, None], 2.0 * g[2] * (u + 1.0) / (n_high * c), 0.0)
        g_u[:, 0] -= 2.0 * g[0] * e / (s["drift"] * F)
        if n_mid:
            g_u[:, 0] += np.where(s["mid"], 2.0 * g[6] * (np.abs(u[:, 0]) - 1.0) * np.sign(u[:, 0]) / n_mid, 0.0)
        g_m = np.zeros((N, 2))
        g_m[:, 1] = 2.0 * g[5] * (y - my) / F
    for k, v in (("means", g_m), ("u", g_u), ("deltas", g_d)):
        grads[k] = np.where(m[:, None], v, 0.0)
    return grads


def recipe_on(case, g=None, mistake=None):
    """the recipe in float64 on the CPU at the case's values; with ``g`` also the gradients of <g, terms>"""
    leaves = [torch.tensor(case[k], dtype=torch.float64, requires_grad=g is not None) for k in INPUTS]
    terms = state_loss_recipe(*leaves, torch.tensor(case["mask"]), case["wall"], case["drift"], mistake)
    if g is None:
        return terms.numpy(), None
    grads = torch.autograd.grad((terms * torch.tensor(g)).sum(), leaves, allow_unused=True)
    return terms.detach().numpy(), {k: np.zeros_like(case[k]) if t is None else t.numpy() for k, t in zip(INPUTS, grads)}


def assert_checker_is_recipe(what, case, seed):
    g = make_g(seed)
    want, want_g = recipe_on(case, g)
    got, got_g = checker_terms(case), checker_grads(case, g)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    worst = float(np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300), initial=0.0))
    assert worst <= 1e-12, f"{what}: terms {worst:.3g}: {got} vs {want}"
    for k in INPUTS:
        err = float(np.abs(got_g[k] - want_g[k]).max()) / max(scale_of(want_g[k]), 1e-3)
        worst = max(worst, err)
        assert err <= 1e-12, f"{what}: d {k} {err:.3g} of its scale"
    return worst


@pytest.mark.parametrize("N", [1, 7, 64, 257])
@pytest.mark.parametrize("mask", MASKS)
def test_checker_agrees_with_the_recipes_autograd(mask, N):
    """float64, c running through 1..4: terms at 1e-12 of each, gradients at 1e-12 of each tensor's scale; with no free
    row the NaN pattern is torch.mean's of nothing and the checker's gradients are zero"""
    c = 1 + (N + MASKS.index(mask)) % 4
    case = make_case(N, c, seed=10 + N, mask=mask)
    if not case["mask"].any():
        got, (want, _) = checker_terms(case), recipe_on(case)
        assert np.array_equal(np.isnan(got), [True, False, False, True, True, True, False, False])
        assert np.array_equal(np.isnan(want), np.isnan(got)) and not got[~np.isnan(got)].any() and not want[~np.isnan(want)].any()
        assert torch.isnan(torch.mean(torch.zeros(3)[torch.zeros(3, dtype=torch.bool)]))
        assert not any(v.any() for v in checker_grads(case, make_g(1)).values())
        return
    worst = assert_checker_is_recipe(f"{mask} N={N} c={c}", case, seed=N)
    print(f"checker vs recipe, {mask}, N = {N}, c = {c}: worst {worst:.3g}")


@pytest.mark.parametrize("heights", ["nolow", "nohigh", "nomid"])
def test_checker_with_an_empty_set(heights):
    case = make_case(65, 2, seed=20, mask="half", heights=heights)
    s = statistics(case)
    assert [int(s[k].sum()) > 0 for k in ("low", "high", "mid")] == [heights != "nolow", heights != "nohigh", heights != "nomid"]
    assert_checker_is_recipe(heights, case, seed=21)
    terms = checker_terms(case)
    empty = {"nolow": [1], "nohigh": [2], "nomid": [6, 7]}[heights]
    assert not terms[empty].any() and np.isfinite(terms).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_checker_walls_are_strict_in_the_dtype(dtype):
    """rows at exactly +-wall are in no set, one ulp outside is LOW / HIGH, one ulp inside is MID; torch compares a
    tensor of the dtype with the Python scalar in the same way"""
    case = make_case(64, 2, seed=30, mask="all", values="walls", dtype=dtype)
    s = statistics(case)
    rows = np.arange(6)
    assert [(bool(s["low"][r]), bool(s["high"][r]), bool(s["mid"][r])) for r in rows] == [
        (False, False, False), (False, False, False), (True, False, False), (False, False, True), (False, False, True),
        (False, True, False)]
    y = torch.tensor(case["means"][rows, 1], dtype={np.float32: torch.float32, np.float64: torch.float64}[dtype])
    assert (y < -WALL).tolist() == [bool(s["low"][r]) for r in rows] and (y > WALL).tolist() == [bool(s["high"][r]) for r in rows]
    assert (y.abs() < WALL).tolist() == [bool(s["mid"][r]) for r in rows]
    if dtype is np.float64:
        assert_checker_is_recipe("walls", case, seed=31)


def test_checker_sign_of_zero_is_zero():
    case = make_case(7, 1, seed=32, mask="all")
    case["means"][:, 1] = 0.0
    case["u"][3, 0] = 0.0
    assert_checker_is_recipe("u0 = 0", case, seed=33)
    g = np.zeros(8)
    g[6] = 1.0
    assert checker_grads(case, g)["u"][3, 0] == 0.0


# ---- planted mistakes ---------------------------------------------------------------------------------------
def ulp_bar(want):
    """the GPU file's bar on a term in float64: 4 ulp"""
    return 4.0 * np.spacing(np.abs(want))


@pytest.mark.parametrize("mistake", MISTAKES)
def test_planted_mistake_is_seen(mistake):
    """each mistake moves a pinned number by more than 1e3 x the GPU file's bar on it (4 ulp of a loss in float64).  Four
    of them show on the recorded scenes.  The recorded scenes have c = 1 and no row on a wall, so "channel0" and
    "nonstrict" cannot show there: they are measured against the checker, on c = 3 and on heights planted at +-wall."""
    factor = 0.0
    if mistake in ("nonstrict", "channel0"):
        case = make_case(64, 3, seed=40, mask="all", values="walls" if mistake == "nonstrict" else "ordinary")
        want = checker_terms(case)
        got, _ = recipe_on(case, mistake=mistake)
        factor = float((np.abs(got - want) / ulp_bar(want)).max())
        right, _ = recipe_on(case)
        assert float((np.abs(right - want) / ulp_bar(want)).max()) <= 1.0
    else:
        for scene in SCENES:
            got = scene_losses(scene, lambda *a: state_loss_recipe(*a, mistake=mistake))
            for name in ("pde_loss", "bc_loss", "conservation_loss"):
                if scene[name] != 0.0:
                    factor = max(factor, float(abs(got[name] - scene[name]) / ulp_bar(scene[name])))
    print(f"planted mistake {mistake}: moves a pinned number by {factor:.3g} x the GPU bar")
    assert factor > 1e3, f"{mistake}: {factor:.3g} x the bar"


# ---- plumbing -----------------------------------------------------------------------------------------------
def test_column_order():
    import pigs_amd
    from pigs_amd import state_loss
    assert pigs_amd.STATE_LOSS_COLUMNS == state_loss.STATE_LOSS_COLUMNS == COLUMNS
    assert not any(name.startswith("test_") for name in dir(state_loss))
    # each term answers to its own inputs: a delta in one block moves that block's entries and nothing else
    base = make_case(17, 2, seed=50)
    base["deltas"][:] = 0.0
    still = checker_terms(base)
    moved_by = {0: {3, 4}, 1: {0, 4}, 5: {7}, 6: {7}}
    for col, want in moved_by.items():
        case = dict(base, deltas=base["deltas"].copy())
        case["deltas"][::2, col] = 0.125
        moved = set(np.flatnonzero(checker_terms(case) != still).tolist())
        assert moved == want, (col, moved)
    for col in (2, 3, 4):
        case = dict(base, deltas=base["deltas"].copy())
        case["deltas"][:, col] = 0.125
        assert np.array_equal(checker_terms(case), still)


def test_refusals_touch_no_gpu(hip_lib):
    import pigs_amd
    op = pigs_amd.state_loss_terms
    N, c = 4, 2
    means, u, deltas, mask = torch.zeros(N, 2), torch.ones(N, c), torch.zeros(N, 5 + c), torch.ones(N, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(means, u, deltas, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(means, u, deltas[None], mask[:, None], wall=0.5, drift=2.0)
    with pytest.raises(TypeError):
        op(means.numpy(), u, deltas, mask)
    with pytest.raises(NotImplementedError):
        op(torch.zeros(N, 3), u, deltas, mask)                                   # d = 3
    with pytest.raises(NotImplementedError):
        op(torch.zeros(N, 1), u, deltas, mask)                                   # d = 1
    with pytest.raises(NotImplementedError):
        op(means, torch.ones(N, 5), torch.zeros(N, 10), mask)                    # c = 5
    with pytest.raises(ValueError):
        op(torch.zeros(0, 2), torch.ones(0, c), torch.zeros(0, 5 + c), torch.ones(0, dtype=torch.bool))      # N = 0
    with pytest.raises(ValueError):
        op(means, torch.ones(N + 1, c), deltas, mask)                            # row counts differ
    with pytest.raises(ValueError):
        op(means, u, torch.zeros(N, 4 + c), mask)                                # deltas: not 5 + c columns
    with pytest.raises(ValueError):
        op(means, u, torch.zeros(2, N, 5 + c), mask)                             # a leading 2
    with pytest.raises(ValueError):
        op(means, u, deltas, torch.ones(N + 1, dtype=torch.bool))
    with pytest.raises(TypeError):
        op(means, u.double(), deltas, mask)                                      # dtypes differ
    with pytest.raises(TypeError):
        op(means.half(), u.half(), deltas.half(), mask)
    with pytest.raises(TypeError):
        op(means, u, deltas, mask.to(torch.uint8))                               # the mask is torch.bool
    for bad in ({"wall": -0.1}, {"wall": float("nan")}, {"wall": float("inf")}, {"drift": 0.0}, {"drift": float("nan")}):
        with pytest.raises(ValueError):
            op(means, u, deltas, mask, **bad)
    args = [means, u, deltas, mask[:, None]]
    for k, a in enumerate(args):                                                 # a strided view of the right shape
        bad = list(args)
        bad[k] = torch.cat((a, a), dim=0)[::2]
        assert bad[k].shape == a.shape and not bad[k].is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            op(*bad)


NAMES = ("pigs_state_loss_scratch_bytes", "pigs_state_loss_forward", "pigs_state_loss_backward")


def test_symbols_declared_exported_and_bound(hip_lib):
    from pigs_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name       # one ctypes type per parameter
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION
    assert _lib.SIGNATURES["pigs_state_loss_scratch_bytes"][0] is ctypes.c_size_t
    bound = int(re.search(r"#define\s+PIGS_STATE_LOSS_ONE_LAUNCH_ROWS\s+(\d+)", header).group(1))
    assert bound == 4096
    # the statistics record of 8 doubles; above the one-launch bound also a record of 20 doubles per 256 rows
    sizes = {n: hip_lib.pigs_state_loss_scratch_bytes(n) for n in (-1, 0, 1, 56, bound, bound + 1, 65536)}
    assert sizes == {-1: 0, 0: 0, 1: 64, 56: 64, bound: 64, bound + 1: 64 + 17 * 160, 65536: 64 + 256 * 160}


def test_abi_refusals_come_before_any_hip_call(hip_lib):
    """pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some, odd = ctypes.c_void_p(0), ctypes.c_void_p(1 << 12), ctypes.c_void_p((1 << 12) + 4)
    fwd, bwd = hip_lib.pigs_state_loss_forward, hip_lib.pigs_state_loss_backward

    def forward(dtype=0, c=1, N=4, wall=0.8, drift=5.0, ptrs=None, nbytes=1 << 20):
        p = list(ptrs or [some] * 6)                   # means, u, deltas, mask, scratch, terms
        return fwd(dtype, c, N, wall, drift, *p[:5], nbytes, p[5], null)
    assert forward(dtype=7) == 2
    assert forward(c=0) == 2 and forward(c=5) == 2
    assert forward(N=0) == 1 and forward(N=-3) == 1
    assert forward(wall=-1.0) == 1 and forward(wall=float("nan")) == 1 and forward(wall=float("inf")) == 1
    assert forward(drift=0.0) == 1 and forward(drift=float("nan")) == 1 and forward(drift=float("inf")) == 1
    for k in range(6):
        p = [some] * 6
        p[k] = null
        assert forward(ptrs=p) == 1, k                                            # a null array
    p = [some] * 6
    p[4] = odd
    assert forward(ptrs=p) == 1                                                   # the scratch holds doubles
    assert forward(N=4096, nbytes=63) == 4 and forward(N=4097, nbytes=64 + 17 * 160 - 1) == 4      # a short scratch

    def backward(dtype=0, c=1, N=4, wall=0.8, drift=5.0, ptrs=None):
        p = list(ptrs or [some] * 9)                   # means, u, deltas, mask, scratch, g_terms, three gradients
        return bwd(dtype, c, N, wall, drift, *p, null)
    assert backward(dtype=7) == 2 and backward(c=5) == 2 and backward(N=0) == 1
    assert backward(wall=float("nan")) == 1 and backward(drift=0.0) == 1
    for k in range(6):
        p = [some] * 9
        p[k] = null
        assert backward(ptrs=p) == 1, k                                           # a null input, scratch or g_terms
    p = [some] * 9
    p[4] = odd
    assert backward(ptrs=p) == 1
    p = [some] * 9
    p[6:] = [null] * 3
    assert backward(ptrs=p) == 1                                                  # no gradient wanted
