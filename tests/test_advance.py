"""CPU: advance_gaussians (pigs_amd/advance.py, csrc/advance.hip) -- its float64 checker against torch autograd through
a torch composition of the same semantics, the checker's covariance block against the reference's own builder
(tests/golden/ref_build_covariances.npz), the column order, the refusals, the C ABI.  No GPU call is made here.

The checker, shared with tests/test_advance_gpu.py:
    make_case()          inputs (float64 numpy holding values of the case's dtype), one mask family, one value family
    checker_forward()    the nine outputs
    make_gout()          random gradients on a chosen subset of the nine outputs
    checker_backward()   the five input gradients in closed form
The formulas are restated independently of the kernel: the covariance gradients go through the partials with respect to
(s0, s1, r, h, k) as tests/test_optim.py does, not through the kernel's collected expressions; the penalty is an exactly
rounded sum (math.fsum), so the checker adds no summation error of its own to the 4-ulp bar of the GPU file.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("means", "u", "scaling", "transforms", "covariances", "conics", "full_covariances", "full_conics", "penalty")
INPUTS = ("means", "u", "scaling", "transforms", "deltas")
MASKS = ("all", "prefix", "half", "single", "none")


def columns(c):
    """the column order of ``deltas``, the network's own (model_pn.py:269-272); its keys are the penalty's order"""
    return {"dmeans": slice(0, 2), "dscaling": slice(2, 4), "dtransforms": slice(4, 5), "du": slice(5, 5 + c)}


# ---- cases --------------------------------------------------------------------------------------------------
def make_mask(N, family, rng):
    """True = a free Gaussian.  "prefix": the first 50 rows are boundary rows (the TEST problem's shape) at N >= 256,
    the first N // 2 below; "single": one free row, the middle one"""
    if family == "all":
        return np.ones(N, bool)
    if family == "none":
        return np.zeros(N, bool)
    if family == "prefix":
        return np.arange(N) >= (50 if N >= 256 else N // 2)
    if family == "half":
        return rng.random(N) < 0.5
    if family == "single":
        m = np.zeros(N, bool)
        m[N // 2] = True
        return m
    raise ValueError(family)


def wrap_targets(lo, hi, dtype):
    """where means' is planted: exactly on lo and on hi (both stay), one ulp outside each (both shift), and 1.25 periods
    outside each (ONE shift leaves them a quarter period outside: a second shift would be wrong)"""
    lo, hi = dtype(lo), dtype(hi)
    period = hi - lo
    inf = dtype(np.inf)
    return np.array([lo, hi, np.nextafter(lo, -inf), np.nextafter(hi, inf), lo - dtype(1.25) * period,
                     hi + dtype(1.25) * period], dtype=dtype)


def make_case(N, c, seed, mask="all", values="ordinary", wrap=None, dtype=np.float64):
    """means U(-0.9, 0.9), u N(0, 1), scaling exp(U[-4, -1]), transforms U[-2, 2]; deltas N(0, sigma) with sigma = 0.05
    (dmeans), 0.3 (dscaling, dtransforms), 0.1 (du); with ``wrap`` the means are U(lo, hi) and dmeans scales with the box.  Every value is one of ``dtype``, held in float64.  Value families,
    planted in the first free (or boundary) rows:
        "t6"      transforms' reaches +-6 (5.5 + 0.5)          "ds10"    dscaling = +-10
        "naninf"  NaN / +Inf / -Inf in every delta of every boundary row
        "wrap"    means' lands on wrap_targets() in both coordinates, reached as (target - 0.25) + 0.25 (exact)"""
    rng = np.random.default_rng(seed)
    a = {"means": rng.uniform(-0.9, 0.9, (N, 2)), "u": rng.standard_normal((N, c)),
         "scaling": np.exp(rng.uniform(-4.0, -1.0, (N, 2))), "transforms": rng.uniform(-2.0, 2.0, (N, 1))}
    sigma = np.concatenate(([0.05, 0.05, 0.3, 0.3, 0.3], np.full(c, 0.1)))
    a["deltas"] = rng.standard_normal((N, 5 + c)) * sigma
    m = make_mask(N, mask, rng)
    free, bound = np.flatnonzero(m), np.flatnonzero(~m)
    if wrap is not None:
        lo, hi = wrap
        a["means"] = rng.uniform(lo, hi, (N, 2))                  # some rows cross an edge
        a["deltas"][:, 0:2] *= (hi - lo) / 2.0
    a = {k: v.astype(dtype) for k, v in a.items()}
    if values == "t6":
        rows = free[:4]
        sign = np.array([1.0, -1.0, 1.0, -1.0], dtype=dtype)[:len(rows)]
        a["transforms"][rows, 0] = 5.5 * sign
        a["deltas"][rows, 4] = 0.5 * sign
    elif values == "ds10":
        rows = free[:4]
        a["deltas"][rows, 2:4] = np.array([[10.0, -10.0], [-10.0, 10.0], [10.0, 10.0], [-10.0, -10.0]], dtype=dtype)[:len(rows)]
    elif values == "naninf":
        a["deltas"][bound] = np.array([np.nan, np.inf, -np.inf], dtype=dtype)[np.arange(len(bound)) % 3][:, None]
    elif values == "wrap":
        targets = wrap_targets(*wrap, dtype)
        rows = free[:len(targets)]
        t = targets[:len(rows)]
        for axis in (0, 1):
            a["deltas"][rows, axis] = dtype(0.25)
            a["means"][rows, axis] = t - dtype(0.25)
            assert np.array_equal(a["means"][rows, axis] + a["deltas"][rows, axis], t)      # lands exactly, in dtype
    elif values != "ordinary":
        raise ValueError(values)
    case = {k: v.astype(np.float64) for k, v in a.items()}
    case.update(mask=m, wrap=None if wrap is None else (float(wrap[0]), float(wrap[1])), c=c, N=N)
    return case


# ---- the checker --------------------------------------------------------------------------------------------
def masked_deltas(case):
    """the deltas with the boundary rows set to zero: m = 0 there, whatever they hold"""
    return np.where(case["mask"][:, None], case["deltas"], 0.0)


def cov_terms(s, t):
    e = np.exp(-2.0 * np.abs(t))
    k = (1.0 + e) ** 2 / (4.0 * e)                                # 1 / (1 - tanh(t)^2) = cosh(t)^2, no cancellation
    return s[:, 0], s[:, 1], np.tanh(t), np.sqrt(s[:, 0] * s[:, 1]), k


def penalty_of(case):
    d, m, out = case["deltas"], case["mask"], []
    n_free = int(m.sum())
    for name, cols in columns(case["c"]).items():
        x = d[m][:, cols].reshape(-1)
        out.append(math.fsum(float(v) * float(v) for v in x) / x.size if n_free else float("nan"))
    return np.array(out)


def checker_forward(case):
    d, col = masked_deltas(case), columns(case["c"])
    means = case["means"] + d[:, col["dmeans"]]
    if case["wrap"] is not None:
        lo, hi = case["wrap"]
        means = np.where(means > hi, means - (hi - lo), means)
        means = np.where(means < lo, means + (hi - lo), means)
    scaling = case["scaling"] * np.exp(d[:, col["dscaling"]])
    transforms = case["transforms"] + d[:, col["dtransforms"]]
    s0, s1, h, r, k = cov_terms(scaling, transforms[:, 0])
    cov = np.stack((s0, h * r, s1), -1)
    con = np.stack((k / s0, -h * k / r, k / s1), -1)
    return {"means": means, "u": case["u"] + d[:, col["du"]], "scaling": scaling, "transforms": transforms,
            "covariances": cov, "conics": con, "full_covariances": cov[:, [0, 1, 1, 2]].reshape(-1, 2, 2),
            "full_conics": con[:, [0, 1, 1, 2]].reshape(-1, 2, 2), "penalty": penalty_of(case)}


def make_gout(case, seed, present=OUTPUTS):
    """random gradients on the outputs named in ``present`` (the full matrices' are NOT symmetric); None elsewhere"""
    rng = np.random.default_rng(seed + 7919)
    N, c = case["N"], case["c"]
    shapes = {"means": (N, 2), "u": (N, c), "scaling": (N, 2), "transforms": (N, 1), "covariances": (N, 3),
              "conics": (N, 3), "full_covariances": (N, 2, 2), "full_conics": (N, 2, 2), "penalty": (4,)}
    return {k: rng.standard_normal(shapes[k]) if k in present else None for k in OUTPUTS}


def checker_backward(case, out, gout):
    """gradients of sum_k <gout[k], out[k]> with respect to means, u, scaling, transforms, deltas"""
    N, c, m = case["N"], case["c"], case["mask"]
    d, col = masked_deltas(case), columns(c)

    def g(name, shape):
        return np.zeros(shape) if gout[name] is None else gout[name]
    flat = {}
    for name, full in (("covariances", "full_covariances"), ("conics", "full_conics")):
        f = g(full, (N, 2, 2))
        flat[name] = g(name, (N, 3)) + np.stack((f[:, 0, 0], f[:, 0, 1] + f[:, 1, 0], f[:, 1, 1]), -1)
    gc, q = flat["covariances"], flat["conics"]
    s0, s1, h, r, k = cov_terms(out["scaling"], out["transforms"][:, 0])
    # covariance (s0, h r, s1), conic (k / s0, -h k / r, k / s1): partials with respect to s0, s1, r, h, k
    d_r = gc[:, 1] * h + q[:, 1] * h * k / r ** 2
    d_s0 = gc[:, 0] - q[:, 0] * k / s0 ** 2 + d_r * r / (2.0 * s0)
    d_s1 = gc[:, 2] - q[:, 2] * k / s1 ** 2 + d_r * r / (2.0 * s1)
    d_k = q[:, 0] / s0 + q[:, 2] / s1 - q[:, 1] * h / r
    d_h = gc[:, 1] * r - q[:, 1] * k / r + d_k * 2.0 * h * k ** 2            # dk/dh = 2 h k^2
    G_s = g("scaling", (N, 2)) + np.stack((d_s0, d_s1), -1)                     # with respect to scaling'
    G_t = g("transforms", (N, 1)) + (d_h / k)[:, None]                          # dh/dt = 1 / k
    G_m, G_u = g("means", (N, 2)), g("u", (N, c))                               # the wrap passes the gradient through
    grads = {"means": G_m.copy(), "u": G_u.copy(), "transforms": G_t.copy(),
             "scaling": G_s * np.exp(d[:, col["dscaling"]])}
    g_d = np.zeros((N, 5 + c))
    g_d[:, col["dmeans"]] = G_m
    g_d[:, col["dscaling"]] = G_s * out["scaling"]                              # d scaling' / d dscaling = scaling'
    g_d[:, col["dtransforms"]] = G_t
    g_d[:, col["du"]] = G_u
    n_free = int(m.sum())
    if gout["penalty"] is not None and n_free:
        for j, cols in enumerate(col.values()):
            width = cols.stop - cols.start
            g_d[:, cols] += 2.0 * d[:, cols] * gout["penalty"][j] / (n_free * width)
    grads["deltas"] = np.where(m[:, None], g_d, 0.0)
    return grads


def scale_of(a):
    a = np.asarray(a)
    return max(float(np.abs(a).max()), 1e-300) if a.size else 1e-300


# ---- the torch composition: the reference's lines -----------------------------------------------------------
def torch_forward(means, u, scaling, transforms, deltas, mask, wrap=None):
    """model_pn.py:270-273, 684-698, 878-882 in torch: sliced deltas, ``where`` for the wrap, tanh / inverse covariances.
    ``mask`` is torch.bool [N]; any device, any float dtype.  Returns the nine outputs in the order of OUTPUTS."""
    c = u.shape[1]
    dmeans, dscaling, dtransforms, du = deltas[:, 0:2], deltas[:, 2:4], deltas[:, 4:5], deltas[:, deltas.shape[1] - c:]
    m = mask[:, None].to(means.dtype)
    new_means = means + dmeans * m
    new_scaling = scaling * torch.exp(dscaling * m)
    new_transforms = transforms + dtransforms * m
    new_u = u + du * m
    if wrap is not None:
        lo, hi = wrap
        new_means = torch.where(new_means > hi, new_means - (hi - lo), new_means)
        new_means = torch.where(new_means < lo, new_means + (hi - lo), new_means)
    tau = torch.tanh(new_transforms[:, 0]) * torch.sqrt(new_scaling[:, 0] * new_scaling[:, 1])
    full_cov = torch.stack((new_scaling[:, 0], tau, tau, new_scaling[:, 1]), dim=-1).reshape(-1, 2, 2)
    full_con = torch.linalg.inv(full_cov)
    cov = torch.stack((full_cov[:, 0, 0], full_cov[:, 0, 1], full_cov[:, 1, 1]), dim=-1)
    con = torch.stack((full_con[:, 0, 0], full_con[:, 0, 1], full_con[:, 1, 1]), dim=-1)
    penalty = torch.stack([torch.mean(x[mask] ** 2) for x in (dmeans, dscaling, dtransforms, du)])
    return new_means, new_u, new_scaling, new_transforms, cov, con, full_cov, full_con, penalty


def torch_case(case, dtype=torch.float64, device="cpu"):
    leaves = [torch.tensor(case[k], dtype=dtype, device=device, requires_grad=True) for k in INPUTS]
    return leaves, torch.tensor(case["mask"], device=device)


def torch_grads(outs, leaves, gout):
    loss = None
    for o, name in zip(outs, OUTPUTS):
        if gout[name] is not None:
            term = (o * torch.as_tensor(gout[name], dtype=o.dtype, device=o.device)).sum()
            loss = term if loss is None else loss + term
    return torch.autograd.grad(loss, leaves, allow_unused=True)


@pytest.mark.parametrize("mask", ["all", "prefix", "half", "single"])
@pytest.mark.parametrize("wrap", [None, (-1.0, 1.0), (-0.5, 1.75)], ids=["nowrap", "wrap11", "wrapbox"])
def test_checker_agrees_with_torch_autograd(mask, wrap):
    """float64 on the CPU, N = 257, c = 2: the nine outputs and the five input gradients from random gradients on all
    nine outputs, 1e-12 of each tensor's scale"""
    case = make_case(257, 2, seed=1, mask=mask, wrap=wrap)
    out = checker_forward(case)
    gout = make_gout(case, seed=2)
    grads = checker_backward(case, out, gout)
    leaves, tmask = torch_case(case)
    touts = torch_forward(*leaves, tmask, wrap)
    worst = 0.0
    for name, t in zip(OUTPUTS, touts):
        err = np.abs(out[name] - t.detach().numpy()).max() / scale_of(t.detach().numpy())
        worst = max(worst, err)
        assert err <= 1e-12, f"{name}: {err:.3g} of its scale"
    for name, t in zip(INPUTS, torch_grads(touts, leaves, gout)):
        err = np.abs(grads[name] - t.numpy()).max() / scale_of(t.numpy())
        worst = max(worst, err)
        assert err <= 1e-12, f"d {name}: {err:.3g} of its scale"
    if wrap is not None and mask != "single":
        assert (np.abs(out["means"] - (case["means"] + masked_deltas(case)[:, :2])) > 1.0).any()      # some rows wrapped
    print(f"checker vs torch autograd, {mask}, wrap {wrap}: worst {worst:.3g} of a tensor's scale")


@pytest.mark.parametrize("present", [("penalty",), ("conics",), ("full_covariances",), ("means", "u"), ("scaling", "transforms")],
                         ids=lambda p: "+".join(p))
def test_checker_gradient_subsets_agree_with_torch(present):
    case = make_case(65, 3, seed=3, mask="half", wrap=(-1.0, 1.0))
    out, gout = checker_forward(case), make_gout(case, seed=4, present=present)
    grads = checker_backward(case, out, gout)
    leaves, tmask = torch_case(case)
    for name, t in zip(INPUTS, torch_grads(torch_forward(*leaves, tmask, (-1.0, 1.0)), leaves, gout)):
        t = np.zeros_like(case[name]) if t is None else t.numpy()
        assert np.abs(grads[name] - t).max() <= 1e-12 * max(scale_of(t), 1e-3), name


def test_checker_wrap_is_one_shift_with_strict_inequalities():
    for wrap in ((-1.0, 1.0), (-0.5, 1.75)):
        for dtype in (np.float32, np.float64):
            case = make_case(64, 1, seed=5, mask="all", values="wrap", wrap=wrap, dtype=dtype)
            lo, hi = wrap
            got = checker_forward(case)["means"][:6, 0]
            period = hi - lo
            t = wrap_targets(lo, hi, dtype).astype(np.float64)
            want = [lo, hi, t[2] + period, t[3] - period, lo - 0.25 * period, hi + 0.25 * period]
            assert np.array_equal(got, want), (wrap, dtype, got, want)


def test_checker_no_free_row_is_torch_mean_of_nothing():
    case = make_case(9, 2, seed=6, mask="none", values="naninf")
    out = checker_forward(case)
    assert np.isnan(out["penalty"]).all()
    assert torch.isnan(torch.mean(torch.zeros(9, 2)[torch.zeros(9, dtype=torch.bool)] ** 2))
    for k in ("means", "u", "scaling", "transforms"):
        assert np.array_equal(out[k], case[k])
    grads = checker_backward(case, out, make_gout(case, seed=7))
    assert not grads["deltas"].any() and all(np.isfinite(v).all() for v in grads.values())


def test_checker_covariance_block_is_the_reference_builder():
    """zero deltas: the covariance block alone, against the reference's own outputs and autograd gradients"""
    d = np.load(os.path.join(GOLDEN, "ref_build_covariances.npz"))
    N = d["scaling"].shape[0]
    case = {"means": np.zeros((N, 2)), "u": np.zeros((N, 1)), "scaling": d["scaling"], "transforms": d["transform"],
            "deltas": np.zeros((N, 6)), "mask": np.ones(N, bool), "wrap": None, "c": 1, "N": N}
    out = checker_forward(case)
    assert np.abs(out["covariances"] - d["cov"]).max() <= 1e-14 * scale_of(d["cov"])
    assert np.abs(out["conics"] / d["conic"] - 1).max() < 1e-12                  # element-wise: conics span 6 decades
    assert np.abs(out["full_covariances"] - d["full_cov"]).max() <= 1e-14 * scale_of(d["full_cov"])
    assert np.abs(out["full_conics"] / d["full_conic"] - 1).max() < 1e-12
    gout = dict.fromkeys(OUTPUTS)
    gout.update(covariances=d["r_cov"], conics=d["r_conic"])
    grads = checker_backward(case, out, gout)
    assert np.abs(grads["scaling"] - d["g_scaling"]).max() <= 1e-12 * scale_of(d["g_scaling"])
    assert np.abs(grads["transforms"] - d["g_transform"]).max() <= 1e-12 * scale_of(d["g_transform"])
    # the same gradients arriving at the full matrices, the xy entry split unevenly over the two off-diagonals
    full = {}
    for name, r in (("full_covariances", d["r_cov"]), ("full_conics", d["r_conic"])):
        full[name] = np.stack((r[:, 0], 0.25 * r[:, 1], 0.75 * r[:, 1], r[:, 2]), -1).reshape(-1, 2, 2)
    again = checker_backward(case, out, dict(dict.fromkeys(OUTPUTS), **full))
    assert np.abs(again["scaling"] - d["g_scaling"]).max() <= 1e-12 * scale_of(d["g_scaling"])


def test_column_order_is_the_networks():
    """ADVANCE_PENALTY_COLUMNS, the column order of ``deltas`` and the checker agree: a delta in one block moves that
    block's output and that block's penalty entry, nothing else"""
    import pigs_amd
    from pigs_amd import advance
    c = 3
    assert pigs_amd.ADVANCE_PENALTY_COLUMNS == advance.ADVANCE_PENALTY_COLUMNS == tuple(columns(c)) \
        == ("dmeans", "dscaling", "dtransforms", "du")
    assert advance.DELTA_COLUMNS == columns(c)["du"].start and advance.Advanced._fields == OUTPUTS
    moved_by = {"dmeans": {"means"}, "dscaling": {"scaling", "covariances", "conics", "full_covariances", "full_conics"},
                "dtransforms": {"transforms", "covariances", "conics", "full_covariances", "full_conics"}, "du": {"u"}}
    base = make_case(17, c, seed=8)
    base["deltas"][:] = 0.0
    still = checker_forward(base)
    for j, (name, cols) in enumerate(columns(c).items()):
        case = dict(base, deltas=base["deltas"].copy())
        case["deltas"][:, cols] = 0.125
        out = checker_forward(case)
        assert np.array_equal(out["penalty"] != 0, np.arange(4) == j) and out["penalty"][j] == 0.125 ** 2
        moved = {k for k in OUTPUTS[:-1] if not np.array_equal(out[k], still[k])}
        assert moved == moved_by[name], (name, moved)


# ---- the Python surface -------------------------------------------------------------------------------------
def test_refusals_touch_no_gpu(hip_lib):
    import pigs_amd
    adv = pigs_amd.advance_gaussians
    N, c = 4, 2
    means, u, scaling, transforms = torch.zeros(N, 2), torch.ones(N, c), torch.ones(N, 2), torch.zeros(N, 1)
    deltas, mask = torch.zeros(N, 5 + c), torch.ones(N, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        adv(means, u, scaling, transforms, deltas, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        adv(means, u, scaling, transforms[:, 0], deltas[None], mask[:, None], wrap=(-1.0, 1.0))
    with pytest.raises(TypeError):
        adv(means.numpy(), u, scaling, transforms, deltas, mask)
    with pytest.raises(NotImplementedError):
        adv(torch.zeros(N, 3), u, scaling, transforms, deltas, mask)             # d = 3
    with pytest.raises(NotImplementedError):
        adv(torch.zeros(N, 1), u, torch.ones(N, 1), transforms, deltas, mask)    # d = 1
    with pytest.raises(NotImplementedError):
        adv(means, u, scaling, torch.zeros(N, 3), deltas, mask)                  # d = 3 transforms
    with pytest.raises(NotImplementedError):
        adv(means, torch.ones(N, 5), scaling, transforms, torch.zeros(N, 10), mask)      # c = 5
    with pytest.raises(ValueError):
        adv(torch.zeros(0, 2), torch.ones(0, c), torch.ones(0, 2), torch.zeros(0, 1), torch.zeros(0, 5 + c),
            torch.ones(0, dtype=torch.bool))                                     # N = 0
    with pytest.raises(ValueError):
        adv(means, torch.ones(N + 1, c), scaling, transforms, deltas, mask)      # row counts differ
    with pytest.raises(ValueError):
        adv(means, u, scaling, transforms, torch.zeros(N, 4 + c), mask)          # deltas: not 5 + c columns
    with pytest.raises(ValueError):
        adv(means, u, scaling, transforms, torch.zeros(2, N, 5 + c), mask)       # a leading 2
    with pytest.raises(ValueError):
        adv(means, u, scaling, transforms, deltas, torch.ones(N + 1, dtype=torch.bool))
    with pytest.raises(TypeError):
        adv(means, u.double(), scaling, transforms, deltas, mask)                # dtypes differ
    with pytest.raises(TypeError):
        adv(means.half(), u.half(), scaling.half(), transforms.half(), deltas.half(), mask)
    with pytest.raises(TypeError):
        adv(means, u, scaling, transforms, deltas, mask.to(torch.uint8))         # the mask is torch.bool
    with pytest.raises(ValueError):
        adv(means, u, scaling, transforms, deltas, mask, wrap=(1.0, -1.0))


def test_non_contiguous_input_is_refused(hip_lib):
    """every argument in turn as a strided view of the right shape: ValueError, before the device is looked at"""
    import pigs_amd
    N, c = 4, 2
    args = [torch.zeros(N, 2), torch.ones(N, c), torch.ones(N, 2), torch.zeros(N, 1), torch.zeros(N, 5 + c),
            torch.ones(N, 1, dtype=torch.bool)]
    for k, a in enumerate(args):
        bad = list(args)
        bad[k] = torch.cat((a, a), dim=0)[::2]
        assert bad[k].shape == a.shape and not bad[k].is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            pigs_amd.advance_gaussians(*bad)


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_advance_scratch_bytes", "pigs_advance_forward", "pigs_advance_backward")


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
    assert _lib.SIGNATURES["pigs_advance_scratch_bytes"][0] is ctypes.c_size_t
    # one record of 5 doubles per workgroup of 256 rows, and one for the totals
    sizes = {n: hip_lib.pigs_advance_scratch_bytes(n) for n in (-1, 0, 1, 256, 257, 1600, 65536)}
    assert sizes == {-1: 0, 0: 0, 1: 80, 256: 80, 257: 120, 1600: 320, 65536: 257 * 40}


def test_abi_refusals_come_before_any_hip_call(hip_lib):
    """pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some, odd = ctypes.c_void_p(0), ctypes.c_void_p(1 << 12), ctypes.c_void_p((1 << 12) + 4)
    fwd, bwd = hip_lib.pigs_advance_forward, hip_lib.pigs_advance_backward

    def forward(dtype=0, c=1, N=4, wrap=0, lo=-1.0, hi=1.0, ptrs=None, nbytes=1 << 20):
        p = list(ptrs or [some] * 16)                  # 4 state, deltas, mask, scratch, 9 outputs
        return fwd(dtype, c, N, wrap, lo, hi, *p[:7], nbytes, *p[7:], null)
    assert forward(dtype=7) == 2
    assert forward(c=0) == 2 and forward(c=5) == 2
    assert forward(N=0) == 1 and forward(N=-3) == 1
    assert forward(wrap=1, lo=1.0, hi=1.0) == 1 and forward(wrap=1, lo=float("nan")) == 1
    for k in range(16):
        p = [some] * 16
        p[k] = null
        assert forward(ptrs=p) == 1, k                                            # a null array
    for k in (0, 2, 7, 9):                                                        # the rows of two: off their alignment
        p = [some] * 16
        p[k] = odd
        assert forward(ptrs=p) == 1, k
        assert forward(dtype=1, ptrs=[ctypes.c_void_p((1 << 12) + 8) if j == k else some for j in range(16)]) == 1, k
    p = [some] * 16
    p[6] = odd
    assert forward(ptrs=p) == 1                                                   # the scratch holds doubles
    assert forward(N=257, nbytes=119) == 4 and forward(N=256, nbytes=79) == 4     # a short scratch

    def backward(dtype=0, c=1, N=4, ptrs=None):
        p = list(ptrs or [some] * 19)                  # 3 saved, mask, scratch, 9 incoming, 5 gradients
        return bwd(dtype, c, N, *p, null)
    assert backward(dtype=7) == 2 and backward(c=5) == 2 and backward(N=0) == 1
    for k in range(4):
        p = [some] * 19
        p[k] = null
        assert backward(ptrs=p) == 1, k                                           # a null saved array or mask
    p = [some] * 19
    p[4] = null
    assert backward(ptrs=p) == 1                                                  # a penalty gradient needs the scratch
    p = [some] * 19
    p[14:] = [null] * 5
    assert backward(ptrs=p) == 1                                                  # no gradient wanted
    for k in (0, 5, 7, 14, 16):                                                   # the rows of two
        p = [some] * 19
        p[k] = odd
        assert backward(ptrs=p) == 1, k
