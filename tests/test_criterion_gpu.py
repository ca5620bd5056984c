"""GPU: the split criteria (pigs_amd/refine.py: split_mask, threshold_mask, split_criterion; csrc/criterion.hip).

Kernel level, exact and without exclusions: the metric against the same composition in torch on the CPU (2 ulp; bit
equality expected), x_lo / x_hi equal to np.sort of the kernel's OWN metric at lo / hi, the quantile within 1 ulp of
the double formula on those two, the mask torch.equal to the compare of the kernel's own metric with its own quantile,
the two variants bitwise alike.  End to end: split_criterion on the scenes of tests/test_criterion.py against the float64
oracle, with that file's band and cap.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_criterion import (BAND_ROWS, LDS_VALUES, SCENE_CHANNELS, SCENE_GRIDS, SCENE_SEEDS, compare_with_scene_oracle,
                            criterion_oracle, meanstd_oracle, quantile_of_pair, quantile_position, scene_oracle)

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
QS = [0.98, 0.0, 1.0, 0.5, "integer"]


def integer_q(L):
    """a q near 1/4 whose position q (L - 1) is an integer in double arithmetic"""
    for lo in range((L - 1) // 4, L):
        q = lo / (L - 1)
        if q * (L - 1) == lo:
            return q


@pytest.fixture(scope="module")
def refine(hip_lib):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from pigs_amd import refine
    return refine


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


# ---- sizes ----------------------------------------------------------------------------------------------------
BASE_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025]
LARGE = 50001
SWEEP = 70001                  # with c = 4 more values than 256 workgroups of 1 024 threads take in one sweep


def sizes_for(c):
    """the base sizes, the n that put L = n c just below / at / above the one-workgroup limit, and one large size"""
    return BASE_SIZES + [(LDS_VALUES - 1) // c, LDS_VALUES // c, LDS_VALUES // c + 1] + [LARGE] + ([SWEEP] if c == 4 else [])


def variants_for(L):
    return ("one", "many") if L <= LDS_VALUES else ("many",)


def test_sizes_cover_the_mechanisms(refine):
    assert refine.CRITERION_LDS_VALUES == LDS_VALUES
    for c in (1, 2, 3, 4):
        Ls = [n * c for n in sizes_for(c)]
        assert LDS_VALUES - 1 in Ls or LDS_VALUES in Ls         # the largest one-workgroup size
        assert any(L <= LDS_VALUES for L in Ls) and any(LDS_VALUES < L <= LDS_VALUES + c for L in Ls)
        assert max(Ls) > 1024 * (256 if c == 4 else 1)          # more than one workgroup; c = 4: more than one sweep
    assert LDS_VALUES in [n * c for c in (1, 2, 4) for n in sizes_for(c)]
    assert variants_for(LDS_VALUES) == ("one", "many") and variants_for(LDS_VALUES + 1) == ("many",)


# ---- the kernel-level check -----------------------------------------------------------------------------------
worst = {"metric_ulp": 0.0}


def ulps(got, want):
    """largest distance in units of the spacing at `want`; NaN and inf must match exactly"""
    special = ~np.isfinite(want)
    assert np.array_equal(got[special], want[special], equal_nan=True)
    if special.all():
        return 0.0
    return float((np.abs(got[~special] - want[~special]) / np.spacing(np.abs(want[~special]))).max())


def check_case(refine, su, pu, D, bm, q, dtype, expect_nan=False):
    """su, pu [n, c], D [n] numpy (any float dtype); bm bool [n] or None.  Runs every variant the size admits."""
    npd = NP[dtype]
    su, pu, D = (np.asarray(a, npd) for a in (su, pu, D))
    n, c = su.shape
    t_su, t_pu, t_D = torch.as_tensor(su), torch.as_tensor(pu), torch.as_tensor(D).reshape(n, 1)
    want_metric = (((t_su - t_pu) ** 2) * (1.0 - (t_D - t_D.min()) / t_D.max())).numpy()      # :733, :745, :750 on the CPU
    assert want_metric.dtype == npd
    g_bm = dev(bm)
    results = []
    for variant in variants_for(n * c):
        mask, metric, stats = refine.split_mask(dev(su), dev(pu), dev(D), g_bm, q=q, variant=variant, return_stats=True)
        assert mask.dtype == torch.bool and mask.shape == (n,) and metric.shape == (n, c) and metric.dtype == dtype
        plain = refine.split_mask(dev(su), dev(pu), dev(D).reshape(n, 1), None if g_bm is None else g_bm.reshape(n, 1),
                                  q=q, variant=variant)
        assert torch.equal(plain, mask)
        m, s = metric.cpu().numpy(), stats.cpu().numpy()
        worst["metric_ulp"] = max(worst["metric_ulp"], ulps(m, want_metric))
        assert ulps(m, want_metric) <= 2
        quantile, x_lo, x_hi, nan = s
        assert (nan == 1.0) == expect_nan == bool(np.isnan(m).any()) and nan in (0.0, 1.0)
        if expect_nan:
            assert np.isnan(quantile) and np.isnan(x_lo) and np.isnan(x_hi) and not mask.any()
        else:
            x = np.sort(m.ravel())
            lo, hi, t = quantile_position(x.size, q)
            assert np.array_equal(x_lo, x[lo]) and np.array_equal(x_hi, x[hi]), (variant, n, c, q, x_lo, x[lo], x_hi, x[hi])
            want_q = quantile_of_pair(x[lo], x[hi], t, npd)
            if np.isfinite(want_q):
                assert abs(quantile - want_q) <= np.spacing(abs(want_q)), (variant, quantile, want_q)
            else:
                assert np.array_equal(quantile, want_q, equal_nan=True)
        want_mask = (metric > stats[0]).any(-1)
        if g_bm is not None:
            want_mask = want_mask & g_bm
        assert torch.equal(mask, want_mask), (variant, n, c, q)
        results.append((m, s, mask.cpu().numpy()))
    for other in results[1:]:                                   # the variants agree bit for bit
        for a, b in zip(results[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return results[0]


def random_inputs(n, c, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, c)), rng.standard_normal((n, c)), rng.uniform(0.5, 3.0, n), rng.random(n) < 0.7


@DTYPES
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_sizes_random(refine, dtype, c):
    for n in sizes_for(c):
        su, pu, D, bm = random_inputs(n, c, 100 * c + n)
        _, s, mask = check_case(refine, su, pu, D, bm if n % 2 else None, 0.98, dtype)
        if n * c == 1:
            assert not mask.any()                               # L = 1: quantile = x[0], the compare is strict
    print(f"[figure] metric vs the CPU composition, worst so far: {worst['metric_ulp']:.3g} ulp")


# ---- value families -------------------------------------------------------------------------------------------
FAMILY_SIZES = [(65, 1), (1025, 2), (8193, 2)]                  # the last above the one-workgroup limit
FAMILIES = ["random", "eight_values", "all_equal", "zeros", "denormals", "magnitudes", "one_inf", "one_nan",
            "constant_density", "mask_none", "mask_all_false"]


def family(kind, n, c, dtype, seed):
    """(su, pu, D, bm, expect_nan); unless the kind says otherwise pu = 0 and D is constant, so m = su * su exactly"""
    rng = np.random.default_rng(seed)
    su, pu, D, bm = rng.standard_normal((n, c)), np.zeros((n, c)), np.full(n, 1.5), rng.random(n) < 0.7
    tiny = 1e-20 if dtype == torch.float32 else 1e-160          # its square is a denormal
    if kind == "random":
        pu, D = rng.standard_normal((n, c)), rng.uniform(0.5, 3.0, n)
    elif kind == "eight_values":
        su = rng.integers(1, 9, (n, c)).astype(np.float64)      # x[lo] == x[hi], many entries equal the quantile
    elif kind == "all_equal":
        su = np.full((n, c), 0.75)
    elif kind == "zeros":                                       # D < 0 in places: w < 0 there, and 0 * w = -0.0
        D = rng.uniform(0.5, 3.0, n) * np.where(rng.random(n) < 0.3, -1.0, 1.0)
        su = np.where(rng.random((n, c)) < 0.6, 0.0, su)
    elif kind == "denormals":
        su = su * tiny
    elif kind == "magnitudes":                                  # m from 1e-30 to 1e30: every digit decides somewhere
        su = 10.0 ** rng.uniform(-15, 15, (n, c))
    elif kind == "one_inf":
        su[n // 3, c - 1] = np.inf
    elif kind == "one_nan":
        su[n // 2, 0] = np.nan
    elif kind == "constant_density":
        pu = rng.standard_normal((n, c))
    elif kind == "mask_none":
        bm = None
    elif kind == "mask_all_false":
        bm = np.zeros(n, bool)
    return su, pu, D, bm, kind == "one_nan"


@DTYPES
@pytest.mark.parametrize("kind", FAMILIES)
def test_value_families(refine, kind, dtype):
    for n, c in FAMILY_SIZES:
        for q in QS:
            exact = q == "integer"
            q = integer_q(n * c) if exact else q
            assert not exact or quantile_position(n * c, q)[2] == 0.0
            su, pu, D, bm, expect_nan = family(kind, n, c, dtype, seed=n + c)
            m, s, mask = check_case(refine, su, pu, D, bm, q, dtype, expect_nan)
            if kind == "all_equal" or kind == "mask_all_false":
                assert not mask.any()
            if kind == "eight_values" and (q == 0.5 or exact):
                assert s[1] == s[2] == s[0] and (m == s[0]).sum() > n * c // 16
            if kind == "zeros":
                assert np.signbit(m[m == 0]).any() and not np.signbit(m[m == 0]).all()
            if kind == "denormals":
                assert (np.abs(m[m != 0]) < np.finfo(NP[dtype]).tiny).all()
            if kind == "one_inf" and q == 0.98:
                assert np.isinf(m).sum() == 1 and np.isfinite(s[0]) and (m > s[0]).sum() >= 1
            if kind == "mask_none" and q == 0.98:
                assert mask.sum() > 0


def test_inputs_that_require_grad_views_and_empty(refine):
    su, pu, D, bm = random_inputs(300, 2, 5)
    a, b, d = dev(su, torch.float32), dev(pu, torch.float32), dev(D, torch.float32)
    want = refine.split_mask(a, b, d, dev(bm))
    wide = torch.cat((a, a), -1).requires_grad_(True)
    got = refine.split_mask(wide[:, 2:], b.clone().requires_grad_(True), d, dev(bm))           # a view that wants a gradient
    assert torch.equal(got, want) and not got.requires_grad
    empty = refine.split_mask(a[:0], b[:0], d[:0])
    assert empty.shape == (0,) and empty.dtype == torch.bool
    with pytest.raises(NotImplementedError):
        refine.split_mask(dev(np.zeros((LDS_VALUES + 1, 1)), torch.float32), dev(np.zeros((LDS_VALUES + 1, 1)), torch.float32),
                          dev(np.ones(LDS_VALUES + 1), torch.float32), variant="one")
    with pytest.raises(TypeError):
        refine.split_mask(a, b.double(), d)
    with pytest.raises(ValueError):
        refine.split_mask(a, b, d, q=1.5)


# ---- threshold_mask -------------------------------------------------------------------------------------------
def check_threshold(refine, score, keep, k, dtype):
    npd = NP[dtype]
    score = np.asarray(score, npd)
    n = score.size
    want_t = meanstd_oracle(score, k)[0]
    out = []
    for variant in variants_for(n):
        mask, stats = refine.threshold_mask(dev(score), dev(keep), k=k, variant=variant, return_stats=True)
        threshold, mean, std = stats.cpu().numpy()
        if np.isnan(want_t):
            assert np.isnan(threshold) and not mask.any()
        else:
            assert abs(np.float64(threshold) - want_t) <= 4 * np.spacing(npd(abs(want_t))), (variant, n, threshold, want_t)
        want_mask = dev(score) > stats[0]
        if keep is not None:
            want_mask = want_mask & dev(keep)
        assert torch.equal(mask, want_mask) and mask.dtype == torch.bool
        assert torch.equal(refine.threshold_mask(dev(score), dev(keep), k=k, variant=variant), mask)
        out.append(mask.cpu().numpy())
    return out[0]


@DTYPES
def test_threshold_sizes_random(refine, dtype):
    for n in sizes_for(1):
        rng = np.random.default_rng(n)
        mask = check_threshold(refine, rng.gamma(2.0, size=n), rng.random(n) < 0.7 if n % 2 else None, 1.6, dtype)
        if n == 1:
            assert not mask.any()                               # std of one value is NaN
        if n >= 1023:
            assert 0 < mask.sum() < n


@DTYPES
def test_threshold_constant_scores_nan_and_negative_k(refine, dtype):
    for n in (64, 1025, LDS_VALUES + 1):
        const = np.full(n, 0.75)                                # 0.75 sums exactly: std = 0, threshold = the score
        assert not check_threshold(refine, const, None, 1.6, dtype).any()
        assert not check_threshold(refine, const, None, -1.6, dtype).any()      # k * 0 = -0: still not above itself
        rng = np.random.default_rng(n)
        score = rng.standard_normal(n)
        low = check_threshold(refine, score, None, -1.0, dtype)
        high = check_threshold(refine, score, None, 1.0, dtype)
        assert low.sum() > n // 2 > high.sum() > 0
        score[n // 2] = np.nan
        assert not check_threshold(refine, score, None, 1.6, dtype).any()


# ---- the C ABI ------------------------------------------------------------------------------------------------
def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_c_abi_canaries_null_outputs_short_workspace_and_variant_limit(refine, hip_lib):
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, c in ((1025, 2), (LDS_VALUES // 2 + 7, 2)):
        su, pu, D, bm = random_inputs(n, c, 9)
        a, b, d, m = dev(su, torch.float32), dev(pu, torch.float32), dev(D, torch.float32), dev(bm)
        want_mask, want_metric, want_stats = refine.split_mask(a, b, d, m, return_stats=True)
        need = hip_lib.pigs_criterion_workspace_bytes(0, n, c)
        ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
        for variant in (0, 2) + ((1,) if n * c <= LDS_VALUES else ()):
            mask = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
            metric = torch.full((n * c + 64,), -5.0, dtype=torch.float32, device="cuda")
            stats = torch.full((4 + 4,), -5.0, dtype=torch.float32, device="cuda")
            rc = hip_lib.pigs_criterion_quantile_mask(0, variant, c, n, 0.98, ptr(a), ptr(b), ptr(d), ptr(m), ptr(ws), need,
                                                      ptr(metric), ptr(stats), ptr(mask), stream)
            assert rc == 0
            assert torch.equal(mask[:n].bool(), want_mask) and (mask[n:] == 7).all() and (mask[:n] <= 1).all()
            assert torch.equal(metric[:n * c].reshape(n, c), want_metric) and (metric[n * c:] == -5.0).all()
            assert torch.equal(stats[:4], want_stats) and (stats[4:] == -5.0).all()
            mask.fill_(7)
            rc = hip_lib.pigs_criterion_quantile_mask(0, variant, c, n, 0.98, ptr(a), ptr(b), ptr(d), None, ptr(ws), need,
                                                      None, None, ptr(mask), stream)             # metric, stats, boundary NULL
            assert rc == 0 and torch.equal(mask[:n].bool(), refine.split_mask(a, b, d)) and (mask[n:] == 7).all()
        assert hip_lib.pigs_criterion_quantile_mask(0, 2, c, n, 0.98, ptr(a), ptr(b), ptr(d), None, ptr(ws), need - 1, None, None,
                                                    ptr(mask), stream) == 4
        rc = hip_lib.pigs_criterion_quantile_mask(0, 1, c, n, 0.98, ptr(a), ptr(b), ptr(d), None, None, 0, None, None, ptr(mask), stream)
        assert rc == (0 if n * c <= LDS_VALUES else 2)          # one workgroup: no workspace; above its limit: refused
    # mean/std: a canary behind the mask, stats NULL, the short workspace
    n = LDS_VALUES + 5
    score = dev(np.random.default_rng(1).gamma(2.0, size=n), torch.float64)
    need = hip_lib.pigs_criterion_workspace_bytes(1, n, 1)
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    mask = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
    assert hip_lib.pigs_criterion_meanstd_mask(1, 0, n, 1.6, ptr(score), None, ptr(ws), need, None, ptr(mask), stream) == 0
    assert torch.equal(mask[:n].bool(), refine.threshold_mask(score)) and (mask[n:] == 7).all()
    assert hip_lib.pigs_criterion_meanstd_mask(1, 2, n, 1.6, ptr(score), None, ptr(ws), need - 1, None, ptr(mask), stream) == 4
    assert hip_lib.pigs_criterion_meanstd_mask(1, 1, n, 1.6, ptr(score), None, None, 0, None, ptr(mask), stream) == 2


# ---- no host wait: capture and replay -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["one", "many"])
def test_capture_and_replay(refine, variant):
    n, c = 1601, 2
    su, pu, D, bm = random_inputs(n, c, 21)
    a, b, d, m = dev(su, torch.float32), dev(pu, torch.float32), dev(D, torch.float32), dev(bm)
    score, keep = dev(np.random.default_rng(2).gamma(2.0, size=n), torch.float32), dev(bm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        refine.split_mask(a, b, d, m, variant=variant)                        # the warm-up: the library is loaded
        refine.threshold_mask(score, keep, variant=variant)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mask = refine.split_mask(a, b, d, m, variant=variant)
        chosen = refine.threshold_mask(score, keep, variant=variant)
    torch.cuda.current_stream().wait_stream(side)
    for seed in (31, 32):
        su, pu, D, bm = random_inputs(n, c, seed)
        for t, new in ((a, su), (b, pu), (d, D), (m, bm)):
            t.copy_(dev(new, t.dtype))
        score.copy_(dev(np.random.default_rng(seed).gamma(2.0, size=n), torch.float32))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask, refine.split_mask(a, b, d, m, variant=variant)) and 0 < int(mask.sum()) < n
        assert torch.equal(chosen, refine.threshold_mask(score, keep, variant=variant)) and 0 < int(chosen.sum()) < n


# ---- end to end: split_criterion ------------------------------------------------------------------------------
worst_e2e = {"quantile": 0.0, "metric": 0.0, "rows": 0}


def run_scene(refine, s, sampler):
    """split_criterion on the scene through `sampler`; returns (mask, metric, quantile) as numpy"""
    from pigs_amd.covariances import build_covariances
    f32 = torch.float32
    cov, con = build_covariances(dev(s.scaling, f32), dev(s.transforms, f32))
    means, prev_means = dev(s.means, f32), dev(s.prev_means, f32)
    args = (sampler, means, dev(s.values, f32), cov, con, prev_means, dev(s.prev_values, f32), cov, con)
    mask = refine.split_criterion(*args, dev(s.boundary_mask))
    assert mask.dtype == torch.bool and mask.shape == (s.n,)
    # the sampler is left bound to the last pass (the previous Gaussians at the current means): its field once more,
    # then the first pass again for the metric and the quantile behind the mask
    prev = sampler.sample_gaussians()
    ones = torch.ones((s.n, 1), device="cuda")
    if refine._one_pass(sampler, s.n, s.c):
        sampler.preprocess(means, torch.cat((dev(s.values, f32), ones), -1), cov, con, means)
        out = sampler.sample_gaussians()
        sample_u, density = out[:, :s.c], out[:, s.c]
    else:
        sampler.preprocess(means, dev(s.values, f32), cov, con, means)
        sample_u = sampler.sample_gaussians()
        sampler.preprocess(means, ones, cov, con, means)
        density = sampler.sample_gaussians()
    again, metric, stats = refine.split_mask(sample_u, prev, density, dev(s.boundary_mask), return_stats=True)
    assert torch.equal(again, mask)
    return mask.cpu().numpy(), metric.cpu().numpy(), float(stats[0])


def check_scene(refine, grid, c, seed, sampler):
    s, o = scene_oracle(grid, c, seed)
    assert int(o.band.sum()) <= BAND_ROWS
    mask, metric, quantile = run_scene(refine, s, sampler)
    q_err, m_err = compare_with_scene_oracle(o, metric, quantile, mask)
    worst_e2e["quantile"] = max(worst_e2e["quantile"], q_err)
    worst_e2e["metric"] = max(worst_e2e["metric"], m_err)
    worst_e2e["rows"] = max(worst_e2e["rows"], int((mask != o.mask).sum()))
    return mask


@pytest.mark.parametrize("host", ["ctypes", "native"])
@pytest.mark.parametrize("c", SCENE_CHANNELS)
@pytest.mark.parametrize("grid", SCENE_GRIDS)
def test_split_criterion_scenes(refine, grid, c, host):
    from diff_gaussian_sampling import GaussianSampler
    sampler = GaussianSampler(True, host=host)
    for seed in SCENE_SEEDS:
        check_scene(refine, grid, c, seed, sampler)
    print(f"[figure] end to end, worst so far in units of the quantile: quantile {worst_e2e['quantile']:.3g}, metric "
          f"{worst_e2e['metric']:.3g} (bar 2e-4); most mask rows that differ in a scene {worst_e2e['rows']}")


def test_split_criterion_binned_backend(refine):
    """a 40^2 scene with the binned path forced (c <= 2 there): with c = 1 the density rides as the second channel, with
    c = 2 it is a pass of its own"""
    from diff_gaussian_sampling import GaussianSampler
    for c in (1, 2):
        check_scene(refine, 40, c, 0, GaussianSampler(True, backend="binned"))
    print(f"[figure] binned: quantile {worst_e2e['quantile']:.3g}, metric {worst_e2e['metric']:.3g}")


def test_split_criterion_periodic(refine):
    """periodic=(-1, 1): the oracle sums the nine images"""
    from diff_gaussian_sampling import GaussianSampler
    from test_criterion import BAND
    s, _ = scene_oracle(40, 2, 1)
    total = [0.0, 0.0, 0.0]
    for shift in [(2.0 * i, 2.0 * j) for i in (-1, 0, 1) for j in (-1, 0, 1)]:
        total = [t + f for t, f in zip(total, shifted_fields(s, np.array(shift)))]
    o = criterion_oracle(*total, s.boundary_mask)
    o.band = (np.abs(o.metric - o.quantile) <= BAND * o.quantile).any(-1)
    assert int(o.band.sum()) <= BAND_ROWS
    mask, metric, quantile = run_scene(refine, s, GaussianSampler(True, periodic=(-1.0, 1.0)))
    q_err, m_err = compare_with_scene_oracle(o, metric, quantile, mask)
    print(f"[figure] periodic: quantile {q_err:.3g}, metric {m_err:.3g} of the quantile")


def shifted_fields(s, shift):
    """the three fields of the scene's Gaussians moved by `shift`, at the unmoved current means (float64)"""
    from oracle import covariances_numpy, dense_numpy
    _, conics = covariances_numpy.build_covariances(s.scaling, s.transforms)
    full = np.stack((conics[:, 0], conics[:, 1], conics[:, 1], conics[:, 2]), -1).reshape(-1, 2, 2)
    at = s.means.astype(np.float64)
    both = np.concatenate((s.values, np.ones((s.n, 1), np.float32)), -1).astype(np.float64)
    out = dense_numpy.forward(at + shift, full, both, at, orders=(0,))[0]
    prev = dense_numpy.forward(s.prev_means.astype(np.float64) + shift, full, s.prev_values.astype(np.float64), at, orders=(0,))[0]
    return out[:, :s.c], prev, out[:, s.c]


def test_model_forward_split_recipe_with_the_criterion(refine):
    """INTEGRATION.md, 'Model.forward(split=True)': prune, split_criterion, split_gaussians -- against the same steps
    composed in numpy from the float64 oracle"""
    import types
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.covariances import build_covariances
    from test_criterion import BAND, fields
    s, _ = scene_oracle(20, 2, 2)
    f32 = torch.float32
    rng = np.random.default_rng(8)
    values = s.values * (rng.random((s.n, 1)) > 0.1)            # a tenth of the rows is empty: the prune drops them
    means, scaling, transforms, u = dev(s.means, f32), dev(s.scaling, f32), dev(s.transforms, f32), dev(values, f32)
    boundary_mask = dev(s.boundary_mask).reshape(-1, 1)
    keep = (torch.norm(torch.abs(u), dim=-1) > 0.01) | ~boundary_mask.squeeze(-1)              # :703-704
    p = refine.split_gaussians(means, scaling, transforms, u, None, keep)
    boundary_mask = boundary_mask.index_select(0, p.source)
    cov, con = build_covariances(p.scaling, p.transforms)
    kept = keep.cpu().numpy()
    prev_cov, prev_con = build_covariances(scaling, transforms)
    sampler = GaussianSampler(True)
    indices = refine.split_criterion(sampler, p.means, p.values, cov, con, dev(s.prev_means, f32), dev(s.prev_values, f32),
                                     prev_cov, prev_con, boundary_mask)
    r = refine.split_gaussians(p.means, p.scaling, p.transforms, p.values, indices)
    n_kept, n_split = int(kept.sum()), int(indices.sum())
    assert 0 < n_kept < s.n and n_split > 0
    assert r.means.shape[0] == n_kept + n_split
    # the oracle: the current Gaussians are the kept rows, the previous ones all rows
    cur = types.SimpleNamespace(n=n_kept, c=s.c, scaling=s.scaling[kept], transforms=s.transforms[kept], means=s.means[kept],
                                values=values[kept].astype(np.float32), prev_means=s.means[kept], prev_values=values[kept])
    su, _, density = fields(cur)
    old = types.SimpleNamespace(n=s.n, c=s.c, scaling=s.scaling, transforms=s.transforms, means=s.prev_means,
                                values=s.prev_values, prev_means=s.prev_means, prev_values=s.prev_values)
    prev_su = fields_at(old, s.means[kept])
    o = criterion_oracle(su, prev_su, density, s.boundary_mask[kept])
    band = (np.abs(o.metric - o.quantile) <= BAND * o.quantile).any(-1)
    assert int(band.sum()) <= BAND_ROWS
    differ = indices.cpu().numpy() != o.mask
    assert not (differ & ~band).any()
    assert torch.equal(r.source[r.child < 0], torch.nonzero(~indices).squeeze(-1))


def fields_at(s, points):
    """the field of the Gaussians (s.means, s.values) at `points`, float64"""
    from oracle import covariances_numpy, dense_numpy
    _, conics = covariances_numpy.build_covariances(s.scaling, s.transforms)
    full = np.stack((conics[:, 0], conics[:, 1], conics[:, 1], conics[:, 2]), -1).reshape(-1, 2, 2)
    return dense_numpy.forward(s.means.astype(np.float64), full, s.values.astype(np.float64), points.astype(np.float64),
                               orders=(0,))[0]
