"""CPU: the periodic domain on boxes other than (-1, 1), as far as it goes without a device (DESIGN.md section 11,
"Boxes").  tests/test_periodic_boxes_gpu.py and tests/test_periodic_aggregate_boxes_gpu.py move the suite's (-1, 1)
problems onto the boxes below by x -> lo + (x + 1) a, a = (hi - lo) / 2: means and points mapped, covariances times
a^2, conics divided by a^2, aggregation frequencies divided by a, values and features unchanged.  Here:

(1) the map applied to the checkers alone -- the image sum of the float64 C oracle on a box is the (-1, 1) sum times
    a^-k for order k, and oracle/aggregate_torch.py on the mapped 9N images gives the unmapped output, both to 1e-12:
    the GPU files' inputs mean what they say before any kernel is involved;
(2) the cut-off band of every list case of tests/test_periodic_aggregate_boxes_gpu.py from the brute-force relation
    alone: at most BAND_CAP of the pairs may be decided either way by rounding, and every case has sure pairs that
    are met through an image;
(3) the C entry points and both hosts refuse a box that is none.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import aggregate_torch, c_oracle

# name -> (lo, hi); what each separates from (-1, 1) is in DESIGN.md section 11
BOXES = {"A": (0.0, 1.0), "B": (0.0, 2 * math.pi), "C": (0.25, 3.75), "D": (-5.5, -1.5), "E": (64.0, 66.0)}
HOSTS = ("native", "ctypes")
# the list cases of tests/test_periodic_aggregate_boxes_gpu.py, (box, dtype, generator, N): 2 500 takes the grid build,
# 400 the all-pairs build
LIST_CASES = [(b, t, g, 2500) for b in "ABCD" for t in ("float32", "float64") for g in ("torus", "torus_small", "torus_wide")] + \
             [(b, t, "torus", 400) for b in "ABCD" for t in ("float32", "float64")]
SHIFTS = np.array([(kx, ky) for ky in (-1, 0, 1) for kx in (-1, 0, 1)], dtype=np.float64)
PIGS_ERR_INVALID = 1


def stacked_images(means, lo, period):
    m = lo + np.mod(means - lo, period)
    return np.concatenate([m + s * period for s in SHIFTS])


def base_problem(N=48, res=17, seed=3):
    """Gaussians in (-1, 1)^2, half of them next to a seam, a few handed over unwrapped; means and points are rounded
    to float32, so that the dyadic maps below are exact in float64."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1, 1, (N, 2))
    means[:N // 4, 0] = rng.choice([-0.97, 0.97], N // 4) + rng.uniform(-0.03, 0.03, N // 4)
    means[N // 4:N // 2, 1] = rng.choice([-0.97, 0.97], N // 4) + rng.uniform(-0.03, 0.03, N // 4)
    means[-4:] += np.array([[2.0, 0.0], [-2.0, 2.0], [0.0, -4.0], [4.0, 2.0]])
    s = np.exp(rng.uniform(-4.5, -3.0, (N, 2)))
    tau = np.tanh(rng.normal(0, 0.5, N)) * np.sqrt(s[:, 0] * s[:, 1])
    det = s[:, 0] * s[:, 1] - tau ** 2
    con = np.stack((s[:, 1] / det, -tau / det, s[:, 0] / det), -1)
    g = np.linspace(-1.0, 1.0, res)
    pts = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    return np.float32(means).astype(np.float64), con, rng.uniform(-1, 1, (N, 2)), np.float32(pts).astype(np.float64)


@pytest.mark.parametrize("name", list(BOXES))
def test_image_sum_of_the_oracle_follows_the_scale_law(name):
    lo, hi = BOXES[name]
    a = (hi - lo) / 2
    means, con, values, pts = base_problem()
    base = c_oracle.forward(stacked_images(means, -1.0, 2.0), np.tile(con, (9, 1)), np.tile(values, (9, 1)), pts,
                            orders=(0, 1, 2, 3))
    moved = c_oracle.forward(stacked_images(lo + (means + 1) * a, lo, hi - lo), np.tile(con / a ** 2, (9, 1)),
                             np.tile(values, (9, 1)), lo + (pts + 1) * a, orders=(0, 1, 2, 3))
    for k in range(4):
        want = base[k] * a ** -k
        err = np.abs(moved[k] - want).max() / np.abs(want).max()
        assert err < 1e-12, (name, k, err)
    # the sum really has its mass across the seams: without the images the field on the box's edge is another one
    alone = c_oracle.forward(lo + np.mod(lo + (means + 1) * a - lo, hi - lo), con / a ** 2, values, lo + (pts + 1) * a,
                             orders=(0,))
    assert np.abs(alone[0] - moved[0]).max() > 0.1 * np.abs(moved[0]).max()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_aggregation_checker_does_not_see_the_map(name):
    from test_periodic_aggregate_gpu import arguments, images64, lattice
    lo, hi = BOXES[name]
    a = (hi - lo) / 2
    n_side, L, K, F = 6, 3, 4, 2
    N = n_side * n_side
    args = [x.detach() for x in arguments(N, L, K, F, torch.float64, device="cpu")]
    outs, pairs = [], []
    for box in (None, (lo, hi)):
        m, c = lattice(n_side, seed=3, box=box)
        m9, c9 = images64(m, c) if box is None else images64(m, c, lo, hi - lo)
        mask, delta, g = aggregate_torch.neighbor_structure(m9, c9, 36.0)
        f, tr, q, k, fr, dist = args
        if box is not None:
            fr = fr / a
        outs.append(aggregate_torch.aggregate(mask, delta, g, f.repeat(9, 1), tr, q.repeat(9, 1), k.repeat(9, 1), fr, dist)[:N])
        pairs.append(mask[:N])
    assert torch.equal(pairs[0], pairs[1]) and bool(pairs[0].reshape(N, 9, N)[:, 1:].any())
    err = float((outs[1] - outs[0]).abs().max() / outs[0].abs().max())
    assert err < 1e-12, (name, err)


@pytest.mark.parametrize("list_case", LIST_CASES, ids=["-".join(map(str, c)) for c in LIST_CASES])
def test_band_shares_and_images_of_every_list_case(list_case):
    """No case leaves the decision of more than BAND_CAP of its pairs to rounding (none at all in float64), so the
    list tests hold the kernel to the brute-force relation; and the relation has pairs through an image."""
    import test_aggregate_matrix_gpu as G
    name, dtype, gen, N = list_case
    rel = G.relation(dtype, gen, N, BOXES[name])
    print(f"box {name} {gen} N={N} {dtype}: sure {rel.sure.numel()}, band {rel.band.numel()}, "
          f"longest row {int(rel.row_counts.max())}, images {sorted(rel.images_seen)}")
    assert rel.band_fraction <= G.BAND_CAP[dtype], (rel.band.numel(), rel.sure.numel())
    assert rel.images_used
    if gen == "torus_small" and name in ("A", "D"):          # a crowd on either side of the x seam and of the y seam
        assert rel.images_seen & {4, 5} and rel.images_seen & {2, 7}, rel.images_seen


# ---- (3)
def test_entry_points_refuse_a_box_that_is_none(hip_lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)          # p is never dereferenced: every call fails its checks

    def images(lo, period, dtype=0):
        return hip_lib.pigs_periodic_images(dtype, 1, 4, lo, period, 44.0, *([p] * 6), null, null)

    def lists(lo, period, dtype=0):
        return hip_lib.pigs_aggregate_lists_periodic(dtype, 4, 4, p, p, 36.0, lo, period, null, 0, 1, p, p, p, p, p, null)

    for call in (images, lists):
        for dtype in (0, 1):
            for lo, period in ((0.25, 0.0), (0.25, -3.5), (0.0, -2 * math.pi), (0.0, math.nan), (0.0, math.inf),
                               (math.nan, 3.5), (math.inf, 3.5), (-math.inf, 3.5), (1e308, 1e308), (-1.7e308, math.inf)):
                assert call(lo, period, dtype) == PIGS_ERR_INVALID, (call.__name__, dtype, lo, period)


@pytest.mark.parametrize("host", HOSTS)
def test_hosts_refuse_a_box_that_is_none(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    for bad in ((3.75, 0.25), (0, math.inf), (-1.5, -5.5), (2 * math.pi, 0.0)):
        with pytest.raises(ValueError):
            GaussianSampler(False, periodic=bad, host=host)
        s = GaussianSampler(False, periodic=BOXES["C"], host=host)
        with pytest.raises(ValueError):
            s.periodic = bad
        assert s.periodic == BOXES["C"]
    for name, box in BOXES.items():
        s = GaussianSampler(False, periodic=box, host=host)
        assert s.periodic == box
        assert s._core.periodic == box
