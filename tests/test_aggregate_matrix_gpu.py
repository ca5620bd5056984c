"""GPU: the neighbour lists of pigs_amd/csrc/aggregate.hip against an all-pairs statement of the neighbour relation, and
the three sampling kernels at every launch variant against the sparse float64 checker (oracle/aggregate_sparse.py).

What tests/test_aggregate_gpu.py and tests/test_periodic_aggregate_gpu.py leave open is N > 2048 -- the grid walk that
builds the lists, two and one waves per Gaussian, the split sums over N -- and the second component per lane of the
three kernels; tests/test_aggregate_matrix.py asks the launchers' own choice functions and asserts, without a GPU, that
the case lists below reach all of it.

The cut-off band.  With u the unit roundoff of the kernel's dtype and S = |a dx^2| + |2 b dx dy| + |c dy^2|, a pair is
sure in if q <= q_max - 8 u S, sure out if q > q_max + 8 u S and in the band otherwise (8 u S: a first-order bound of
the roundings behind a dx^2 + 2 b dx dy + c dy^2; the periodic lists add the rounding of mu'_j - mu'_i before the shift,
oracle/aggregate_sparse.py).  Band pairs are taken as the kernel decided them; a case may have at most 1e-4 of its pairs
there in float32 and none in float64, which every test asserts.

(a) lists of the grid build against the brute force: every row list holds every sure-in pair, no sure-out pair and no
    entry twice; the counts are the list lengths; the column lists are the transpose; overflow == 0; cap is the longest
    list rounded up to 64.
(b) ``cap`` given: one pass gives the same sets; half the longest list (and half the longest row) sets overflow,
    clamps the counts, stores true neighbours only and makes check() raise.
(c) the periodic grid build against the brute force over the 9N images, with the row walk's ``reach`` cull active (top
    grid level unoccupied) and unbounded (one Gaussian just under the period).
(d) output and six gradients at N = 2049 / 4097 / 8193 (4 / 2 / 1 waves per Gaussian, 2 / 3 / 5 splits of the sums);
    rows and columns from under 64 entries to more than 64 (2 waves - 1): a second round of 64 in every wave.
(e) output and six gradients at N = 300 in the shapes that take the second component per lane, the most LDS, F = 0 and
    both paths of for_row.
(f) bars: those of tests/test_aggregate_gpu.py -- float64 1e-10, float32 5e-5, frequencies x 10, relative to the
    largest entry.  No case needed another.

Measured on an MI355X (all 50 tests, 14 s): band pairs 0 in every case but one (rank_one, float32: 1 of 254 077); worst
error over (d) and (e), float32 / float64: output 7.9e-7 / 1.9e-15, features 1.3e-6 / 2.3e-15, transform 5.0e-7 / 7.9e-15,
queries 2.9e-5 (L = K = 1, F = 0; 4.8e-6 elsewhere) / 2.3e-13, keys 1.5e-6 / 4.2e-15, frequencies 3.5e-6 / 1.1e-13,
distance_transform 3.4e-7 / 2.6e-15.  The list tests catch what they are for: with the grid's cut-off shrunk to
0.9 q_max (a scratch build, ``grid_cutoff`` of aggregate.hip), all 23 tests of (a), (b), (c) that go through the grid
fail on missed neighbours -- 172 to 3 493 pairs a case -- and the two all-pairs cases of (c) pass.
"""
import functools
import math

import pytest
import torch

from oracle import aggregate_sparse as sparse

pytestmark = pytest.mark.gpu

Q_MAX = 36.0
LO, PERIOD = -1.0, 2.0
DTYPES = {"float32": torch.float32, "float64": torch.float64}
NAMES = ("features", "transform", "queries", "keys", "frequencies", "distance_transform")
TOL = {"float32": 5e-5, "float64": 1e-10}
BAND_CAP = {"float32": 1e-4, "float64": 0.0}

# ---- the case lists: plain data (tests/test_aggregate_matrix.py reads them without a GPU)
# (a) (dtype, generator, N)
LIST_CASES = [(t, "spread", N) for t in DTYPES for N in (2049, 4097, 8193)] + \
             [(t, g, 2049) for t in DTYPES for g in ("scales", "anisotropic", "clusters", "rank_one")] + \
             [("float64", "offset", 2049)]
# (c) (dtype, generator, N): periodic lists
PERIODIC_CASES = [(t, g, 2500) for t in DTYPES for g in ("torus", "torus_small", "torus_wide")] + \
                 [(t, "torus", 400) for t in DTYPES]                # the all-pairs build's four shifts, for comparison
# (d) (dtype, N, L, K, F)
VARIANT_CASES = [(t, N, 16, 16, 2) for t in DTYPES for N in (2049, 4097, 8193)]
# (e) (name, L, K, F, dtypes); N = SHAPE_N, all-pairs build, four waves per Gaussian
SHAPE_N = 300
SHAPES = [("forward_cols_second", 40, 30, 5, ("float32", "float64")),
          ("rows_cols_second", 8, 66, 2, ("float32", "float64")),
          ("float32_widest", 78, 50, 6, ("float32",)),              # W = 128 and L + K = 128
          ("float32_largest", 1, 126, 2, ("float32",)),             # K + F = 128: 134 272 B in the backward by rows
          ("float64_largest", 13, 66, 11, ("float64",)),
          ("no_frequencies", 1, 1, 0, ("float32", "float64")),
          ("scalar_rows", 5, 3, 1, ("float32", "float64")),
          ("vector_rows", 6, 16, 1, ("float32", "float64"))]
SHAPE_CASES = [(t, name, L, K, F) for name, L, K, F, ts in SHAPES for t in ts]
# the periodic instantiations of the sampling kernels on lists of (c): (dtype, generator, N, L, K, F)
PERIODIC_NUMERIC = [(t, "torus", N, 4, 1, 3) for t in DTYPES for N in (400, 2500)]


# ---- inputs: float64 on the CPU, deterministic
def conics_of(sdx, sdy, rho):
    sxx, syy, sxy = sdx * sdx, sdy * sdy, rho * sdx * sdy
    det = sxx * syy - sxy * sxy
    return torch.stack((syy / det, -sxy / det, sxx / det), dim=-1)


def conics_of_axes(s1, s2, theta):
    """Principal standard deviations s1, s2, the first axis at angle theta."""
    c, s = torch.cos(theta), torch.sin(theta)
    i1, i2 = 1 / (s1 * s1), 1 / (s2 * s2)
    return torch.stack((c * c * i1 + s * s * i2, c * s * (i1 - i2), s * s * i1 + c * c * i2), dim=-1)


def rand(g, *shape):
    return torch.rand(shape, generator=g, dtype=torch.float64)


def randn(g, *shape):
    return torch.randn(shape, generator=g, dtype=torch.float64)


SPREAD = {2049: 0.5, 4097: 0.9, 8193: 0.7}      # log-normal spread of the standard deviations


CROWD = 400


def gen_spread(g, N):
    """Centres over [-1, 1)^2, standard deviations log-normal with mean 1.15 * 2 / sqrt(N) and spread SPREAD[N]; CROWD
    of the centres lie in one patch of side 3 / sqrt(N).  A row's length is a sum over many independent Gaussians and
    stays near its mean (on the CPU 124 / 121 / 131 at N = 2049 / 4097 / 8193 without the crowd, 29 to 180 over all
    rows: the short ones at the domain's border), so a uniform spread gives no row beyond 192.  The crowd's Gaussians
    all reach one another: their rows hold more than CROWD entries, enough for a second round of 64 in every wave of
    a Gaussian at four waves each (more than 448).  The columns range from a few entries to thousands without help."""
    means = rand(g, N, 2) * 2 - 1
    sd = 1.15 * 2 / math.sqrt(N) * torch.exp(randn(g, N, 2) * SPREAD[N] - SPREAD[N] ** 2 / 2)
    rho = torch.tanh(randn(g, N) * 0.5) * 0.5
    means[:CROWD] = torch.tensor([0.3, -0.2], dtype=torch.float64) + (rand(g, CROWD, 2) - 0.5) * 3 / math.sqrt(N)
    return means, conics_of(sd[:, 0], sd[:, 1], rho)


def gen_scales(g, N):
    """Standard deviations log-uniform over 2.4 decades (several grid levels), three Gaussians wider than the domain
    and 40 far below the finest cell."""
    means = rand(g, N, 2) * 2 - 1
    sd = 10 ** (-3.3 + 2.4 * rand(g, N, 1)) * torch.exp(randn(g, N, 2) * 0.2)
    sd[:3] = torch.tensor([[2.5, 3.0], [4.0, 4.0], [9.0, 6.0]], dtype=torch.float64)
    sd[3:43] = 10 ** (-6.5 + rand(g, 40, 2))
    perm = torch.randperm(N, generator=g)
    return means, conics_of(sd[:, 0], sd[:, 1], rand(g, N) - 0.5)[perm]


def gen_anisotropic(g, N):
    """Half: axis ratios up to 14:1 at any angle (|rho| up to 0.99); half: 14:1 to 30:1 within 0.1 rad of an axis."""
    means = rand(g, N, 2) * 2 - 1
    h = N // 2
    ratio = torch.cat((14 ** rand(g, h), 14 * (30 / 14) ** rand(g, N - h)))
    ratio[0], ratio[h] = 14.0, 30.0
    theta = torch.cat((rand(g, h) * math.pi, (rand(g, N - h) - 0.5) * 0.2 + math.pi / 2 * torch.randint(0, 2, (N - h,), generator=g)))
    theta[0] = math.pi / 4
    s2 = 0.3 * 2 / math.sqrt(N) * torch.exp(randn(g, N) * 0.3)
    return means, conics_of_axes(s2 * ratio, s2, theta)


def gen_clusters(g, N):
    """Half of the centres in three tight clusters, 24 exact copies of one centre and 8 duplicated pairs."""
    means = rand(g, N, 2) * 2 - 1
    h = N // 2
    centre = torch.tensor([[-0.4, 0.3], [0.5, 0.55], [0.1, -0.6]], dtype=torch.float64)
    means[:h] = centre[torch.arange(h) % 3] + randn(g, h, 2) * torch.tensor([0.004, 0.02, 0.0005], dtype=torch.float64)[torch.arange(h) % 3, None]
    means[h:h + 24] = means[0]
    means[h + 24:h + 32] = means[h + 32:h + 40]
    sd = 1.15 * 2 / math.sqrt(N) * torch.exp(randn(g, N, 2) * 0.5)
    perm = torch.randperm(N, generator=g)
    return means[perm], conics_of(sd[:, 0], sd[:, 1], torch.tanh(randn(g, N) * 0.5) * 0.5)[perm]


def gen_rank_one(g, N):
    """Two rank-one conics among ordinary Gaussians: a = b = c = 1 (q = (dx + dy)^2 <= 36 everywhere: it reaches
    everybody) and a = b = c = 400 (a strip |dx + dy| <= 0.3 across the domain)."""
    means, conics = gen_spread(g, N)
    conics[N // 3] = 1.0
    conics[2 * N // 3] = 400.0
    return means, conics


def gen_offset(g, N):
    """Centres at (300, -700) + U(-1, 1)^2, every standard deviation along any axis at least 6e-3: the float64 grid is
    built on float32 copies of these centres (spacing 6e-5) under a cut-off inflated by 5 %."""
    means = rand(g, N, 2) * 2 - 1 + torch.tensor([300.0, -700.0], dtype=torch.float64)
    sd = (1.15 * 2 / math.sqrt(N) * torch.exp(randn(g, N, 2) * 0.6)).clamp_min(0.0085)
    sd[:20] = 0.0085
    return means, conics_of(sd[:, 0], sd[:, 1], rand(g, N) - 0.5)       # smallest axis >= 0.0085 sqrt(1 - 0.5) = 6.0e-3


def to_box(means, conics, box):
    """x -> lo + (x + 1) a, a = (hi - lo) / 2, applied to a problem stated on (-1, 1): means (or points) mapped,
    conics / a^2 (None for points); torch tensors or numpy arrays.  ``box`` = (lo, hi); None leaves the problem as it is.  The one
    statement of the map: every box test goes through it."""
    if box is None:
        return means, conics
    a = (float(box[1]) - float(box[0])) / 2.0
    return float(box[0]) + (means + 1.0) * a, None if conics is None else conics / (a * a)


def lo_period_as_held(box, dtype):
    """(lo, period) of ``box`` = (lo, hi) as a kernel of ``dtype`` holds them (both are cast to T); None: (-1, 1)."""
    if box is None:
        return LO, PERIOD
    lo, period = float(box[0]), float(box[1]) - float(box[0])
    if DTYPES[dtype] == torch.float32:
        lo, period = float(torch.tensor(lo, dtype=torch.float32)), float(torch.tensor(period, dtype=torch.float32))
    return lo, period


def gen_torus(g, N, box=None):
    """A jittered lattice that fills the box; part of the means start outside it (the caller wraps)."""
    n = math.isqrt(N)
    cell = PERIOD / n
    t = LO + (torch.arange(n, dtype=torch.float64) + 0.5) * cell
    gx, gy = torch.meshgrid((t, t), indexing="ij")
    means = torch.stack((gx, gy), dim=-1).reshape(N, 2) + (rand(g, N, 2) - 0.5) * 0.7 * cell + 0.31
    sd = (0.06 + 0.04 * rand(g, N, 2)) * (8.0 / n)
    return to_box(means, conics_of(sd[:, 0], sd[:, 1], torch.tanh(randn(g, N) * 0.5) * 0.5), box)


def gen_torus_small(g, N, box=None):
    """Every half extent small (at most 6 * 0.004): the top grid level stays empty and the row walk culls by reach
    (asserted from the grid's level mask by the test)."""
    means = rand(g, N, 2) * 2 - 1
    sd = 0.002 + 0.002 * rand(g, N, 2)
    means[:64, 0] = LO + rand(g, 64) * 0.004                    # a crowd on either side of the seam
    means[64:128, 0] = LO + PERIOD - rand(g, 64) * 0.004
    means[:128, 1] = means[0, 1] + (rand(g, 128) - 0.5) * 0.01
    means[128:160, 1] = LO + rand(g, 32) * 0.004
    means[160:192, 1] = LO + PERIOD - rand(g, 32) * 0.004
    means[128:192, 0] = means[128, 0] + (rand(g, 64) - 0.5) * 0.01
    return to_box(means, conics_of(sd[:, 0], sd[:, 1], rand(g, N) - 0.5), box)


def gen_torus_wide(g, N, box=None):
    """gen_torus with one Gaussian whose q <= q_max half extents are just under the period (0.98 and 0.9 of it): the
    top grid level is occupied and the row walk's reach unbounded (asserted from the grid's level mask by the test)."""
    means, conics = gen_torus(g, N)
    conics[N // 2] = conics_of(torch.tensor(0.98 * PERIOD / 6), torch.tensor(0.9 * PERIOD / 6), torch.tensor(0.3))
    return to_box(means, conics, box)


def gen_shapes(g, N):
    """N = 300: wide enough that a central row is reached by more than 256 Gaussians (five rounds of 64), and one
    Gaussian that reaches everybody (a column of N entries)."""
    means = rand(g, N, 2) * 2 - 1
    sd = 0.3 * torch.exp(randn(g, N, 2) * 0.4)
    sd[7] = 3.0
    return means, conics_of(sd[:, 0], sd[:, 1], torch.tanh(randn(g, N) * 0.5) * 0.5)


GENERATORS = {"spread": gen_spread, "scales": gen_scales, "anisotropic": gen_anisotropic, "clusters": gen_clusters,
              "rank_one": gen_rank_one, "offset": gen_offset, "torus": gen_torus, "torus_small": gen_torus_small,
              "torus_wide": gen_torus_wide, "shapes": gen_shapes}
PERIODIC_GENERATORS = ("torus", "torus_small", "torus_wide")


@functools.lru_cache(maxsize=None)
def inputs(dtype, gen, N, box=None):
    """means [N, 2] and conics [N, 3] rounded to ``dtype`` (float64 on the CPU).  The periodic generators' means are
    wrapped into the box after the rounding, as the sampler hands them to the lists.  ``box`` = (lo, hi), periodic
    generators only: the problem moved onto that box, wrapped on the box as ``dtype`` holds it."""
    g = torch.Generator().manual_seed(1000 * sorted(GENERATORS).index(gen) + N)
    means, conics = GENERATORS[gen](g, N) if box is None else GENERATORS[gen](g, N, box=box)
    means, conics = means.to(DTYPES[dtype]), conics.to(DTYPES[dtype])
    if gen in PERIODIC_GENERATORS:
        lo, period = lo_period_as_held(box, dtype)
        means = lo + torch.remainder(means - lo, period)
        means = torch.where(means >= lo + period, torch.full_like(means, lo), means)
    return means, conics


class Relation:
    """The brute-force relation of one case: sorted keys i * M + column of the sure-in pairs and of the band pairs
    (M = N columns, or 9N with column = k * N + j on the torus)."""

    def __init__(self, dtype, gen, N, box=None):
        means, conics = inputs(dtype, gen, N, box)
        self.N, self.periodic = N, gen in PERIODIC_GENERATORS
        if self.periodic:
            lo, period = lo_period_as_held(box, dtype)
            i, j, k, q, S = sparse.brute_pairs_periodic(means, conics, Q_MAX, lo, period)
            self.M = 9 * N
            key = i * self.M + k * N + j
        else:
            i, j, q, S = sparse.brute_pairs(means, conics, Q_MAX)
            self.M = N
            key = i * self.M + j
        sure, band = sparse.classify(q, S, Q_MAX, DTYPES[dtype])
        self.sure, self.band = key[sure].sort().values, key[band].sort().values
        self.band_fraction = self.band.numel() / max(1, self.sure.numel())
        self.images_used = bool((k[sure] != 0).any()) if self.periodic else False
        self.images_seen = set(k[sure].unique().tolist()) if self.periodic else set()
        self.row_counts = torch.bincount(key[sure] // self.M, minlength=N)


@functools.lru_cache(maxsize=None)
def relation(dtype, gen, N, box=None):
    return Relation(dtype, gen, N, box)


def contains(sorted_keys, keys):
    """Mask of ``keys`` that occur in ``sorted_keys``."""
    if sorted_keys.numel() == 0:
        return torch.zeros_like(keys, dtype=torch.bool)
    pos = torch.searchsorted(sorted_keys, keys).clamp_max(sorted_keys.numel() - 1)
    return sorted_keys[pos] == keys


def list_keys(counts, lists, M, N, periodic, transpose):
    """Keys i * M + column of the valid entries of [N, cap] lists; ``transpose``: the lists are by columns."""
    counts, lists = counts.cpu().long(), lists.cpu().long()
    cap = lists.shape[1]
    valid = torch.arange(cap)[None, :] < counts[:, None]
    own = torch.arange(N)[:, None].expand(N, cap)[valid]
    e = lists[valid] & 0xFFFFFFFF
    other, k = (e & ((1 << 28) - 1), e >> 28) if periodic else (e, torch.zeros_like(e))
    assert int(other.max()) < N and int(k.max()) <= 8
    i, j = (other, own) if transpose else (own, other)
    return i * M + k * N + j


def check_lists(nb, rel, dtype, clamped=False):
    """The set assertions of (a); returns the rows' keys (sorted).  ``clamped``: a truncated build -- only what is
    stored is checked."""
    N, M = rel.N, rel.M
    assert rel.band_fraction <= BAND_CAP[dtype], (rel.band.numel(), rel.sure.numel())
    rows = list_keys(nb.row_counts, nb.row_lists, M, N, rel.periodic, False)
    cols = list_keys(nb.col_counts, nb.col_lists, M, N, rel.periodic, True)
    for keys in (rows, cols):
        assert torch.unique(keys).numel() == keys.numel()                            # no entry twice
        extra = keys[~contains(rel.sure, keys)]
        assert bool(contains(rel.band, extra).all()), int((~contains(rel.band, extra)).sum())      # no sure-out pair
    if clamped:
        return rows.sort().values
    rows = rows.sort().values
    missed = rel.sure[~contains(rows, rel.sure)]
    assert missed.numel() == 0, (missed.numel(), (missed[:5] // M).tolist(), (missed[:5] % M).tolist())
    assert torch.equal(rows, cols.sort().values)                                     # the transpose
    assert int(nb.overflow.item()) == 0
    longest = int(max(nb.row_counts.max(), nb.col_counts.max()))
    assert longest <= nb.cap
    return rows


def build_lists(dtype, gen, N, cap=None, box=None):
    """``box`` = (lo, hi): the lists get (lo, hi - lo) as doubles, the way the sampler hands them over."""
    from pigs_amd.aggregate import NeighborLists
    means, conics = inputs(dtype, gen, N, box)
    per = (LO, PERIOD) if box is None else (float(box[0]), float(box[1]) - float(box[0]))
    return NeighborLists(means.cuda(), conics.cuda(), Q_MAX, cap=cap, periodic=per if gen in PERIODIC_GENERATORS else None)


# ---- (a)
@pytest.mark.parametrize("dtype,gen,N", LIST_CASES)
def test_grid_lists_match_the_brute_force(hip_lib, dtype, gen, N):
    rel = relation(dtype, gen, N)
    nb = build_lists(dtype, gen, N)
    check_lists(nb, rel, dtype)
    longest = int(max(nb.row_counts.max(), nb.col_counts.max()))
    assert nb.cap == max(64, (longest + 63) // 64 * 64)
    print(f"lists {gen} N={N} {dtype}: pairs {rel.sure.numel()}, band {rel.band.numel()}, cap {nb.cap}, "
          f"rows {float(nb.row_counts.float().mean()):.0f} mean / {int(nb.row_counts.max())} max")


# ---- (b)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_given_cap_on_the_grid_build(hip_lib, dtype):
    from pigs_amd._lib import PigsError
    gen, N = "spread", 2049
    rel = relation(dtype, gen, N)
    counted = build_lists(dtype, gen, N)
    rows = check_lists(counted, rel, dtype)
    longest = int(max(counted.row_counts.max(), counted.col_counts.max()))
    one_pass = build_lists(dtype, gen, N, cap=longest)             # not rounded: a slab that fits exactly
    assert one_pass.cap == longest
    assert torch.equal(check_lists(one_pass, rel, dtype), rows)
    one_pass.check()
    # half the longest list (a column) truncates columns only; half the longest row truncates rows as well
    for cap in (longest // 2, int(counted.row_counts.max()) // 2):
        half = build_lists(dtype, gen, N, cap=cap)
        assert half.cap == cap and int(half.overflow.item()) != 0
        for got, full in ((half.row_counts, counted.row_counts), (half.col_counts, counted.col_counts)):
            assert torch.equal(got.cpu(), full.cpu().clamp_max(cap))
        stored = check_lists(half, rel, dtype, clamped=True)       # every stored entry is a true neighbour
        assert stored.numel() == int(half.row_counts.sum()) and int(half.col_counts.sum()) < rows.numel()
        with pytest.raises(PigsError, match="truncated"):
            half.check()
    assert int(half.row_counts.sum()) < rows.numel()


# ---- (c)
def occupied_levels(hip_lib, nb, dtype, N):
    """(mask of the grid levels that hold a Gaussian, levels of the grid) of a grid build."""
    import ctypes
    info = (ctypes.c_int64 * 2)()
    assert hip_lib.pigs_aggregate_grid_info(list(DTYPES).index(dtype), N, info) == 0
    return int(nb.workspace[info[0]:info[0] + 4].view(torch.int32).item()) & 0xFFFFFFFF, int(info[1])


@pytest.mark.parametrize("dtype,gen,N", PERIODIC_CASES)
def test_periodic_lists_match_the_brute_force_on_the_images(hip_lib, dtype, gen, N):
    rel = relation(dtype, gen, N)
    assert rel.images_used
    nb = build_lists(dtype, gen, N)
    rows = check_lists(nb, rel, dtype)
    assert bool(((rows % rel.M) // N != 0).any())                  # some k != 0 in the lists
    if N > 2048:            # aggregate_lists_kernel: the row walk culls a shift by reach unless the top level is occupied
        mask, levels = occupied_levels(hip_lib, nb, dtype, N)
        assert 0 < mask < 1 << levels
        if gen == "torus_small":
            assert mask == 1                                        # the finest level alone: the smallest reach
        if gen == "torus_wide":
            assert mask >> (levels - 1) == 1
        if gen == "torus":
            assert mask >> (levels - 1) == 0
    longest = int(max(nb.row_counts.max(), nb.col_counts.max()))
    assert nb.cap == max(64, (longest + 63) // 64 * 64)
    print(f"periodic lists {gen} N={N} {dtype}: pairs {rel.sure.numel()}, band {rel.band.numel()}, cap {nb.cap}")


# ---- (d), (e)
def arguments(N, L, K, F, seed=1):
    g = torch.Generator().manual_seed(seed)
    E = 4 * F + 1
    args = [rand(g, *s) for s in [(N, L), (L, L), (N, K), (N, K), (F,), (L, 2 * E)]]
    args[4] = randn(g, F) * 10
    return args


def rel_err(got, want):
    want = want.detach().double().cpu()
    if want.numel() == 0:
        return 0.0
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def check_numerics(dtype, gen, N, L, K, F):
    from pigs_amd import aggregate as A
    rel = relation(dtype, gen, N)
    nb = build_lists(dtype, gen, N)
    rows = check_lists(nb, rel, dtype)          # the checker's pairs: the sure-in ones plus the kernel's band decisions
    dt = DTYPES[dtype]
    a64 = [a.to(dt).double() for a in arguments(N, L, K, F)]
    args = [a.to(dt).cuda().requires_grad_(True) for a in a64]
    r64 = randn(torch.Generator().manual_seed(5), N, L).to(dt).double()
    out = A.aggregate(nb, *args)
    assert out.shape == (N, L) and out.dtype == dt
    grads = torch.autograd.grad((out * r64.to(dt).cuda()).sum(), args)

    means, conics = (x.double() for x in inputs(dtype, gen, N))
    for a in a64:
        a.requires_grad_(True)
    I, col = rows // rel.M, rows % rel.M
    f, tr, q, k, fr, dist = a64
    if rel.periodic:
        m9, c9 = sparse.periodic_images(means, conics, LO, PERIOD)
        want = sparse.aggregate(N, I, col, m9, c9, f.repeat(9, 1), tr, q, k.repeat(9, 1), fr, dist)
    else:
        want = sparse.aggregate(N, I, col, means, conics, f, tr, q, k, fr, dist)
    wgrads = torch.autograd.grad((want * r64).sum(), a64)
    err = {"out": rel_err(out, want)}
    for name, got, w in zip(NAMES, grads, wgrads):
        assert got.shape == w.shape and got.dtype == dt
        err[name] = rel_err(got, w)
    print(f"aggregate {gen} N={N} L={L} K={K} F={F} {dtype}: cap {nb.cap}, pairs {rows.numel()}, errors "
          + ", ".join(f"{n} {e:.2g}" for n, e in err.items()))
    for name, e in err.items():
        assert e < TOL[dtype] * (10 if name == "frequencies" else 1), (name, e, err)
    return nb


@pytest.mark.parametrize("dtype,N,L,K,F", VARIANT_CASES)
def test_launch_variants_match_the_sparse_checker(hip_lib, dtype, N, L, K, F):
    nb = check_numerics(dtype, "spread", N, L, K, F)
    # wave g of a Gaussian's wpg takes the entries from 64 g, 64 (g + wpg), ...: beyond 64 (2 wpg - 1) entries every wave
    # runs a second round (the running maximum rescales acc / l across rounds, then the waves merge), under 64 all but
    # the first are left without one -- in the kernels by rows and in the one by columns
    wpg = 4 if N <= 4096 else 2 if N <= 8192 else 1
    for counts in (nb.row_counts.cpu(), nb.col_counts.cpu()):
        assert int(counts.max()) > 64 * (2 * wpg - 1) and int(counts.min()) < 64, (int(counts.min()), int(counts.max()))


@pytest.mark.parametrize("dtype,name,L,K,F", SHAPE_CASES)
def test_shapes_match_the_sparse_checker(hip_lib, dtype, name, L, K, F):
    nb = check_numerics(dtype, "shapes", SHAPE_N, L, K, F)
    assert int(nb.row_counts.max()) > 256 and int(nb.col_counts.max()) == SHAPE_N      # five rounds of 64


@pytest.mark.parametrize("dtype,gen,N,L,K,F", PERIODIC_NUMERIC)
def test_periodic_lists_through_the_sampling_kernels(hip_lib, dtype, gen, N, L, K, F):
    check_numerics(dtype, gen, N, L, K, F)


# ---- the LDS limit: what the C API admits fits a CU, and what does not is refused by both hosts before any launch
def small_sampler(host, dtype):
    from diff_gaussian_sampling import GaussianSampler
    means, conics = (x.cuda() for x in inputs(dtype, "shapes", SHAPE_N))
    s = GaussianSampler(True, unpinned_aggregate=True, host=host, backend="dense")
    s.preprocess(means, torch.ones((SHAPE_N, 1), dtype=means.dtype, device="cuda"), None, conics, means[:16])
    s.preprocess_aggregate()
    return s


@pytest.mark.parametrize("host", ["native", "ctypes"])
def test_float64_shapes_beyond_the_lds_of_a_cu_are_refused(hip_lib, host):
    s = small_sampler(host, "float64")
    for L, K, F in ((126, 1, 0),            # the forward alone would need 260 096 B
                    (16, 100, 2)):          # the forward fits; the backward by columns would need 239 616 B
        args = [a.cuda().requires_grad_(True) for a in arguments(SHAPE_N, L, K, F)]
        with pytest.raises(NotImplementedError, match=r"float64.*163840"):
            s.aggregate_neighbors(*args)
    # the same sizes in float32 are admitted (132 096 B at most) -- and the largest float64 shapes of the matrix run
    s32 = small_sampler(host, "float32")
    args = [a.float().cuda().requires_grad_(True) for a in arguments(SHAPE_N, 16, 100, 2)]
    out = s32.aggregate_neighbors(*args)
    out.sum().backward()
    assert all(bool(torch.isfinite(a.grad).all()) for a in args)
    for L, K, F in ((8, 66, 2), (13, 66, 11)):
        args = [a.cuda().requires_grad_(True) for a in arguments(SHAPE_N, L, K, F)]
        ref = check_reference(L, K, F)
        out = s.aggregate_neighbors(*args)
        assert rel_err(out, ref) < TOL["float64"]
        out.sum().backward()
        assert all(bool(torch.isfinite(a.grad).all()) for a in args)


@functools.lru_cache(maxsize=None)
def check_reference(L, K, F):
    """The sparse checker's output at N = SHAPE_N in float64 (no pair of the case lies in the float64 band)."""
    rel = relation("float64", "shapes", SHAPE_N)
    assert rel.band.numel() == 0
    means, conics = inputs("float64", "shapes", SHAPE_N)
    return sparse.aggregate(SHAPE_N, rel.sure // rel.M, rel.sure % rel.M, means, conics, *arguments(SHAPE_N, L, K, F))
