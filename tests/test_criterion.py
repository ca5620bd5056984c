"""CPU: the split criteria (pigs_amd/refine.py: split_mask, threshold_mask, split_criterion; csrc/criterion.hip) --
their float64 checker against torch.quantile / torch.std and the reference's lines restated, the C ABI's refusals, and
the end-to-end scenes' exclusion cap on the checker alone.  No GPU call is made here.

The checker, shared with tests/test_criterion_gpu.py:
    criterion_oracle()   the quantile rule of include/pigs_amd.h (pigs_criterion_quantile_mask) in numpy, float64 by
                         default; with dtype=np.float32 every operation of the metric is in float32, as on the device
    meanstd_oracle()     the mean/std rule (pigs_criterion_meanstd_mask), sums in float64
    scene() / fields()   the end-to-end scenes and their three sampled fields through oracle.dense_numpy
"""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_VALUES = 16384             # PIGS_CRITERION_LDS_VALUES
MAX_VALUES = 1 << 24


# ---- the checkers -------------------------------------------------------------------------------------------
def quantile_position(L, q):
    """(lo, hi, t) of torch.quantile's linear rule"""
    pos = q * (L - 1)
    lo = int(np.floor(pos))
    return lo, min(lo + 1, L - 1), pos - lo


def quantile_of_pair(x_lo, x_hi, t, dtype):
    """x[lo] + (x[hi] - x[lo]) t in double, rounded once to dtype (inf - inf = NaN is the formula's)"""
    with np.errstate(invalid="ignore"):
        return dtype(np.float64(x_lo) + (np.float64(x_hi) - np.float64(x_lo)) * np.float64(t))


def criterion_oracle(sample_u, prev_sample_u, density, boundary_mask=None, q=0.98, dtype=np.float64):
    """Returns a namespace: metric [n, c], quantile, x_lo, x_hi, nan, mask [n] (bool)."""
    su, pu = np.asarray(sample_u, dtype), np.asarray(prev_sample_u, dtype)
    D = np.asarray(density, dtype).reshape(-1)
    n = su.shape[0]
    o = types.SimpleNamespace()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = dtype(1) - (D - D.min()) / D.max()
        d = su - pu
        o.metric = (d * d) * w[:, None]
    assert o.metric.dtype == dtype
    x = np.sort(o.metric.ravel())
    lo, hi, t = quantile_position(x.size, q)
    o.nan = bool(np.isnan(x).any())
    if o.nan:
        o.x_lo = o.x_hi = o.quantile = dtype(np.nan)
    else:
        o.x_lo, o.x_hi = x[lo], x[hi]
        o.quantile = quantile_of_pair(o.x_lo, o.x_hi, t, dtype)
    with np.errstate(invalid="ignore"):
        o.mask = (o.metric > o.quantile).any(-1)
    if boundary_mask is not None:
        o.mask = o.mask & np.asarray(boundary_mask, bool).reshape(n)
    return o


def meanstd_oracle(score, k=1.6, keep=None):
    """threshold = mean + k * std (unbiased) in float64; returns (threshold, mean, std, mask)"""
    s = np.asarray(score, np.float64)
    n = s.size
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(math.fsum(s)) / n                      # fsum: the sums carry no error of their own
        std = np.sqrt(np.float64(math.fsum((s - mean) ** 2)) / np.float64(n - 1))
        threshold = mean + k * std
        mask = s > threshold
    if keep is not None:
        mask = mask & np.asarray(keep, bool)
    return threshold, mean, std, mask


# ---- the end-to-end scenes ----------------------------------------------------------------------------------
SCENE_GRIDS, SCENE_CHANNELS, SCENE_SEEDS = (8, 20, 40), (1, 2), (0, 1, 2, 3, 4)
BAND = 2e-4                    # of the quantile: the bar of the quantile and of the metric, and the band of the mask
BAND_ROWS = 2                  # the most rows of a scene that may lie in the band


def scene(grid, c, seed):
    """A jittered lattice of grid^2 Gaussians on (-1, 1)^2 and its previous state, held in float32.  Widths about 1.3
    spacings with log-normal scatter (sigma 0.3), rotation parameter tanh(N(0, 0.5)); the previous means moved by
    N(0, 0.1 spacing), the previous values by N(0, 0.05)."""
    rng = np.random.default_rng(1000 * grid + 10 * c + seed)
    n, h = grid * grid, 2.0 / grid
    centre = -1.0 + h * (np.arange(grid) + 0.5)
    means = np.stack(np.meshgrid(centre, centre, indexing="ij"), -1).reshape(n, 2) + rng.uniform(-0.25, 0.25, (n, 2)) * h
    sigma = 1.3 * h * np.exp(0.3 * rng.standard_normal((n, 2)))
    s = types.SimpleNamespace(n=n, c=c, spacing=h)
    s.means = means.astype(np.float32)
    s.scaling = (sigma * sigma).astype(np.float32)
    s.transforms = (0.5 * rng.standard_normal((n, 1))).astype(np.float32)
    s.values = rng.standard_normal((n, c)).astype(np.float32)
    s.prev_means = (means + 0.1 * h * rng.standard_normal((n, 2))).astype(np.float32)
    s.prev_values = (s.values + 0.05 * rng.standard_normal((n, c))).astype(np.float32)
    s.boundary_mask = rng.random(n) < 0.9
    return s


def fields(s, dtype=np.float64):
    """(sample_u, prev_sample_u, density) of a scene through oracle.dense_numpy, every array in `dtype`"""
    from oracle import covariances_numpy, dense_numpy
    _, conics = covariances_numpy.build_covariances(s.scaling, s.transforms)
    full = np.stack((conics[:, 0], conics[:, 1], conics[:, 1], conics[:, 2]), -1).reshape(-1, 2, 2).astype(dtype)
    means, prev_means = s.means.astype(dtype), s.prev_means.astype(dtype)
    both = np.concatenate((s.values, np.ones((s.n, 1), np.float32)), -1).astype(dtype)
    out = dense_numpy.forward(means, full, both, means, orders=(0,))[0]
    prev = dense_numpy.forward(prev_means, full, s.prev_values.astype(dtype), means, orders=(0,))[0]
    assert out.dtype == dtype and prev.dtype == dtype
    return out[:, :s.c], prev, out[:, s.c]


_scene_oracles = {}


def scene_oracle(grid, c, seed):
    """the scene, its float64 criterion and the rows inside the band; computed once per session"""
    key = (grid, c, seed)
    if key not in _scene_oracles:
        s = scene(grid, c, seed)
        o = criterion_oracle(*fields(s), s.boundary_mask)
        o.band = (np.abs(o.metric - o.quantile) <= BAND * o.quantile).any(-1)
        _scene_oracles[key] = (s, o)
    return _scene_oracles[key]


def compare_with_scene_oracle(o, metric, quantile, mask):
    """the end-to-end bars: returns (quantile error, worst metric error) in units of the quantile"""
    q_err = abs(float(quantile) - o.quantile) / o.quantile
    m_err = np.abs(np.asarray(metric, np.float64) - o.metric).max() / o.quantile
    assert q_err <= BAND and m_err <= BAND, (q_err, m_err)
    differ = np.asarray(mask, bool) != o.mask
    assert not (differ & ~o.band).any(), f"{int((differ & ~o.band).sum())} mask rows differ outside the band"
    return q_err, m_err


@pytest.mark.parametrize("c", SCENE_CHANNELS)
@pytest.mark.parametrize("grid", SCENE_GRIDS)
def test_scenes_stay_inside_the_exclusion_cap(grid, c):
    """On the oracle alone at most BAND_ROWS rows of a scene have an entry within BAND * quantile of the quantile; a
    float32 numpy restatement of the whole criterion (standing in for the GPU) meets the end-to-end bars."""
    for seed in SCENE_SEEDS:
        s, o = scene_oracle(grid, c, seed)
        assert o.quantile > 0 and not o.nan
        assert int(o.band.sum()) <= BAND_ROWS, (grid, c, seed, int(o.band.sum()))
        assert 0 < int(o.mask.sum()) < s.n
        r = criterion_oracle(*fields(s, np.float32), s.boundary_mask, dtype=np.float32)
        q_err, m_err = compare_with_scene_oracle(o, r.metric, r.quantile, r.mask)
        print(f"grid {grid} c {c} seed {seed}: band rows {int(o.band.sum())}, float32 quantile {q_err:.2g}, metric {m_err:.2g}, "
              f"mask rows that differ {int((r.mask != o.mask).sum())}")


# ---- the checker against torch ------------------------------------------------------------------------------
def random_fields(n, c, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, c)).astype(dtype), rng.standard_normal((n, c)).astype(dtype),
            rng.uniform(0.5, 3.0, n).astype(dtype))


def t_of(L, q):
    return quantile_position(L, q)[2]


@pytest.mark.parametrize("q", [0.0, 0.5, 0.98, 1.0])
@pytest.mark.parametrize("L", [1, 2, 64, 801, 3200])
def test_quantile_formula_is_torch_quantile(L, q):
    su, pu, D = random_fields(L, 1, L)
    o = criterion_oracle(su, pu, D, q=q)
    want = torch.quantile(torch.as_tensor(o.metric), q).item()
    # torch's lerp evaluates x[hi] - (x[hi] - x[lo]) (1 - t) where t >= 0.5: the same real number through three
    # roundings of its own, each at most half an ulp of a term that does not exceed the result (the metric is >= 0)
    ulps = abs(o.quantile - want) / np.spacing(abs(want))
    print(f"L {L} q {q}: {ulps:.0f} ulp from torch.quantile")
    assert ulps <= (3 if t_of(L, q) >= 0.5 else 0), (o.quantile, want)


def test_quantile_formula_at_an_integer_position():
    L, q = 801, 0.25                                     # pos = 200 exactly
    lo, hi, t = quantile_position(L, q)
    assert (lo, hi, t) == (200, 201, 0.0)
    o = criterion_oracle(*random_fields(L, 1, 5), q=q)
    assert o.quantile == o.x_lo == torch.quantile(torch.as_tensor(o.metric), q).item()


@pytest.mark.parametrize("c", [1, 2])
def test_oracle_is_the_reference_lines_restated(c):
    """model_pn.py:733, :745, :750-754 with torch on the CPU, float64 (the oracle is held to the three fields and the split
    of a recorded forward of the reference in tests/test_model_split.py)"""
    n = 1600
    su, pu, D = random_fields(n, c, 11 + c)
    boundary = np.random.default_rng(3).random((n, 1)) < 0.8
    density = torch.as_tensor(D).reshape(n, 1)
    density = 1.0 - (density - density.min()) / density.max()
    ut = (torch.as_tensor(su) - torch.as_tensor(pu)) ** 2
    metric = ut * density
    quantile = torch.quantile(metric, 0.98)
    indices = ((metric > quantile).any(-1, keepdim=True) * torch.as_tensor(boundary)).squeeze(-1)
    o = criterion_oracle(su, pu, D, boundary, 0.98)
    assert np.array_equal(o.metric, metric.numpy()) and o.quantile == quantile.item()
    assert np.array_equal(o.mask, indices.numpy().astype(bool)) and 0 < o.mask.sum() < n


def test_oracle_conventions():
    su, pu, D = random_fields(50, 2, 7)
    bad = su.copy()
    bad[17, 1] = np.nan
    o = criterion_oracle(bad, pu, D)
    assert o.nan and np.isnan(o.quantile) and not o.mask.any()
    assert np.isnan(torch.quantile(torch.as_tensor(o.metric), 0.98).item())
    one = criterion_oracle(su[:1, :1], pu[:1, :1], D[:1])
    assert one.quantile == one.metric[0, 0] and not one.mask.any()


@pytest.mark.parametrize("k", [1.6, -0.5])
def test_meanstd_oracle_is_torch(k):
    score = np.random.default_rng(2).gamma(2.0, size=2000)
    keep = np.random.default_rng(3).random(2000) < 0.7
    threshold, mean, std, mask = meanstd_oracle(score, k, keep)
    t = torch.as_tensor(score)
    want = torch.mean(t) + k * torch.std(t)                                  # test_no_mlp.py:204
    assert abs(threshold - want.item()) <= 4 * np.spacing(abs(want.item()))
    assert np.array_equal(mask, torch.logical_and(t > want, torch.as_tensor(keep)).numpy())
    assert np.isnan(meanstd_oracle(score[:1])[0]) and not meanstd_oracle(score[:1])[3].any()


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_criterion_lds_values", "pigs_criterion_workspace_bytes", "pigs_criterion_quantile_mask",
         "pigs_criterion_meanstd_mask")


def test_symbols_declared_exported_and_bound(hip_lib):
    from pigs_amd import _lib, refine
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION
    # the header's constant, the library's and the module's mirror
    assert re.search(r"#define PIGS_CRITERION_LDS_VALUES %d\b" % LDS_VALUES, header)
    assert hip_lib.pigs_criterion_lds_values() == LDS_VALUES == refine.CRITERION_LDS_VALUES
    assert LDS_VALUES * 8 < 160 * 1024                  # the float64 keys fit the LDS of a CU


def test_workspace_bytes_is_a_pure_monotone_function_of_the_value_count(hip_lib):
    f = hip_lib.pigs_criterion_workspace_bytes
    for dtype, key in ((0, 4), (1, 8)):
        last = 0
        for n, c in ((1, 1), (63, 1), (64, 2), (LDS_VALUES, 1), (LDS_VALUES // 2 + 1, 2), (50001, 4), (MAX_VALUES // 4, 4),
                     (MAX_VALUES, 1)):
            b = f(dtype, n, c)
            assert b >= last and b >= key * n * c and b == f(dtype, n, c)
            last = b
        assert f(dtype, 1000, 2) == f(dtype, 2000, 1)
        assert f(dtype, 0, 1) == 0 and f(dtype, -5, 1) == 0 and f(dtype, 5, 0) == 0 and f(dtype, 5, -1) == 0
        assert f(dtype, MAX_VALUES + 1, 1) == 0 and f(dtype, MAX_VALUES // 2 + 1, 2) == 0 and f(dtype, 1 << 40, 4) == 0
    assert f(7, 5, 1) == 0


def test_refusals_come_before_any_hip_call(hip_lib):
    """null pointers everywhere: a call that got as far as a launch would fault; none does"""
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(1 << 12)                               # never dereferenced: the call is refused first
    quantile, meanstd = hip_lib.pigs_criterion_quantile_mask, hip_lib.pigs_criterion_meanstd_mask

    def qm(dtype=0, variant=0, c=1, n=4, q=0.98, arrays=(null,) * 4, ws=null, ws_bytes=0, outs=(null,) * 3):
        return quantile(dtype, variant, c, n, q, *arrays, ws, ws_bytes, *outs, null)

    assert qm(dtype=7) == 2 and qm(variant=3) == 2 and qm(variant=-1) == 2
    assert qm(n=MAX_VALUES + 1) == 2 and qm(n=MAX_VALUES // 2 + 1, c=2) == 2           # n * c > 2^24
    assert qm(n=-1) == 1 and qm(c=0) == 1
    assert qm(q=-0.01) == 1 and qm(q=1.01) == 1 and qm(q=float("nan")) == 1
    assert qm() == 1                                                                    # null required arrays
    assert qm(arrays=(some, some, some, null)) == 1                                     # null mask
    assert qm(arrays=(some, null, some, null), outs=(null, null, some)) == 1
    assert qm(n=0) == 0 and qm(n=0, dtype=1, c=3, variant=2) == 0                       # n = 0: ok, no launch
    assert qm(variant=1, n=LDS_VALUES + 1) == 2 and qm(variant=1, n=LDS_VALUES // 2 + 1, c=2) == 2
    need = hip_lib.pigs_criterion_workspace_bytes(0, 5000, 2)
    full = dict(n=5000, c=2, variant=2, arrays=(some, some, some, null), outs=(null, null, some))
    assert qm(ws=some, ws_bytes=need - 1, **full) == 4                                  # workspace one byte short
    assert qm(ws=null, ws_bytes=need, **full) == 1                                      # many workgroups need one

    def ms(dtype=0, variant=0, n=4, k=1.6, score=null, ws=null, ws_bytes=0, mask=null):
        return meanstd(dtype, variant, n, k, score, null, ws, ws_bytes, null, mask, null)

    assert ms(dtype=7) == 2 and ms(variant=3) == 2 and ms(n=MAX_VALUES + 1) == 2
    assert ms(n=-1) == 1 and ms(k=float("nan")) == 1 and ms() == 1 and ms(score=some) == 1
    assert ms(n=0) == 0
    assert ms(variant=1, n=LDS_VALUES + 1) == 2
    need = hip_lib.pigs_criterion_workspace_bytes(1, 50001, 1)
    assert ms(dtype=1, variant=2, n=50001, score=some, mask=some, ws=some, ws_bytes=need - 1) == 4


# ---- the Python surface -------------------------------------------------------------------------------------
def test_criteria_refuse_cpu_tensors_and_bad_arguments(hip_lib):
    import pigs_amd
    from pigs_amd import refine
    for name in ("split_mask", "threshold_mask", "split_criterion"):
        assert getattr(pigs_amd, name) is getattr(refine, name)
    su, pu, D = torch.zeros(4, 2), torch.zeros(4, 2), torch.ones(4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.split_mask(su, pu, D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.threshold_mask(torch.zeros(4))
    with pytest.raises(ValueError):
        refine.split_mask(su, torch.zeros(4, 1), D)
    with pytest.raises(ValueError):
        refine.split_mask(su, pu, torch.ones(5))
    with pytest.raises(ValueError):
        refine.split_mask(torch.zeros(4), torch.zeros(4), D)
    with pytest.raises(TypeError):
        refine.split_mask(su.numpy(), pu, D)
    with pytest.raises(ValueError):
        refine.threshold_mask(torch.zeros(4, 1))
    assert refine.VARIANTS == {"auto": 0, "one": 1, "many": 2}
