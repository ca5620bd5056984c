"""GPU: pigs_amd.grid_lookup (csrc/grid_lookup.hip, pigs_grid_lookup) -- the pixel of an image under every sample point.

The expectation is a numpy statement of the formula with one rounding per operation in the samples' dtype (numpy's
float32 / float64 subtraction, division and multiplication are correctly rounded, as the kernel's must be):

    tx = (x - lo) / (hi - lo) * W ;  ix = clamp(trunc(tx), 0, W - 1) ;  a non-finite x reads pixel 0

Indices (read from an image that holds its own flat indices) and values are EQUAL to it: random points, points planted
exactly on pixel borders, one ulp to either side of them, on the box's edges, outside the box, huge, infinite and NaN.
For box = (-1, 1) and a square image they are also equal to the reference's three torch lines (main_pn.py:206-207, 210)
run on the GPU, on the points where those lines are defined (finite, of moderate size: ``.to(torch.long)`` of a huge or
non-finite float is not)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
M_RANDOM = 4099
SHAPES = [(64, 64), (48, 80)]
BOXES = [(-1.0, 1.0), (-2.5, 2.5)]
NP = {torch.float32: np.float32, torch.float64: np.float64}


def expected_pixels(samples, H, W, box):
    """(iy, ix) by the formula, every operation rounded once in the samples' dtype"""
    T = samples.dtype.type
    lo, span = T(box[0]), T(box[1]) - T(box[0])
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for x, n in ((samples[:, 1], H), (samples[:, 0], W)):
            t = np.trunc((x - lo) / span * T(n))
            i = np.clip(np.where(np.isnan(t), T(0), t), T(0), T(n - 1)).astype(np.int64)
            out.append(np.where(np.isfinite(x), i, 0))
    return out


def points(dtype, H, W, box, seed):
    """M_RANDOM random points over the box and a margin, then the planted ones"""
    T = NP[dtype]
    rng = np.random.default_rng(seed)
    lo, hi = box
    span = hi - lo
    rand = rng.uniform(lo - 0.1 * span, hi + 0.1 * span, (M_RANDOM, 2))
    bx = (lo + np.arange(W + 1) * span / W).astype(T)                       # the pixel borders, rounded to the dtype
    by = (lo + np.arange(H + 1) * span / H).astype(T)
    planted = []                                                            # on a border, and one ulp to either side
    for v in (bx, np.nextafter(bx, T(-np.inf)), np.nextafter(bx, T(np.inf))):
        planted.append(np.stack((v, np.resize(by[::-1], len(v))), -1))      # x on the borders of x (y on some border of y)
    for v in (by, np.nextafter(by, T(-np.inf)), np.nextafter(by, T(np.inf))):
        planted.append(np.stack((np.resize(bx[::-1], len(v)), v), -1))      # y on the borders of y
    special = np.array([[lo, lo], [hi, hi], [lo, hi], [hi, lo], [lo - 0.3, 0.1], [0.1, hi + 0.5], [-1e30, 1e30], [1e30, -1e30],
                        [np.inf, 0.0], [0.0, -np.inf], [np.nan, 0.2], [0.2, np.nan], [np.nan, np.inf], [-0.0, 0.0]])
    return np.concatenate([rand] + planted + [special]).astype(T)


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("image_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_indices_and_values_equal_the_formula(hip_lib, dtype, image_dtype, H, W, box):
    import pigs_amd
    pts = points(dtype, H, W, box, seed=H + W)
    iy, ix = expected_pixels(pts, H, W, box)
    assert len(pts) > M_RANDOM + 6 * 49 and {0, W - 1} <= set(ix.tolist()) and {0, H - 1} <= set(iy.tolist())
    samples = torch.as_tensor(pts, device="cuda")
    index_image = torch.arange(H * W, dtype=image_dtype, device="cuda").reshape(H, W)
    got = pigs_amd.grid_lookup(index_image, samples, box=box)
    assert tuple(got.shape) == (len(pts),) and got.dtype == image_dtype and not got.requires_grad
    want = iy * W + ix
    wrong = np.flatnonzero(got.cpu().numpy().astype(np.int64) != want)
    print(f"{dtype} samples, {image_dtype} image {H} x {W}, box {box}: {len(wrong)} of {len(pts)} indices differ")
    assert len(wrong) == 0, (wrong[:8], pts[wrong[:8]], got[wrong[:8]], want[wrong[:8]])
    image = torch.as_tensor(np.random.default_rng(5).normal(size=(H, W)), dtype=image_dtype, device="cuda")
    got = pigs_amd.grid_lookup(image, samples, box=box)
    assert torch.equal(got, image.reshape(-1)[torch.as_tensor(want, device="cuda")])


@pytest.mark.parametrize("res", [64, 48])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_equals_the_references_lines_on_the_gpu(hip_lib, dtype, res):
    import pigs_amd
    pts = points(dtype, res, res, (-1.0, 1.0), seed=res)
    pts = pts[np.isfinite(pts).all(1) & (np.abs(pts) < 1e6).all(1)]
    assert len(pts) > M_RANDOM + 6 * 49
    samples = torch.as_tensor(pts, device="cuda")
    desired = torch.as_tensor(np.random.default_rng(6).normal(size=(res, res)), dtype=torch.float32, device="cuda")
    coords = ((samples + 1.0) / 2.0 * res).to(torch.long).clamp(0, res - 1)            # main_pn.py:206
    coords = coords[:, 1] * res + coords[:, 0]                                           # :207
    want = torch.take(desired, coords)                                                   # :210
    got = pigs_amd.grid_lookup(desired, samples)
    assert torch.equal(got, want)
    index_image = torch.arange(res * res, dtype=torch.float32, device="cuda").reshape(res, res)
    assert torch.equal(pigs_amd.grid_lookup(index_image, samples).long(), coords)


def test_views_empty_inputs_and_refusals(hip_lib):
    import pigs_amd
    image = torch.arange(48 * 80, dtype=torch.float32, device="cuda").reshape(48, 80)
    samples = torch.as_tensor(points(torch.float32, 48, 80, (-1.0, 1.0), 3), device="cuda")
    want = pigs_amd.grid_lookup(image, samples)
    wide = torch.zeros((len(samples), 3), device="cuda")
    wide[:, :2] = samples
    assert torch.equal(pigs_amd.grid_lookup(image, wide[:, :2]), want)                   # a strided view is made contiguous
    assert torch.equal(pigs_amd.grid_lookup(image.t().contiguous().t(), samples), want)
    assert torch.equal(pigs_amd.grid_lookup(image, samples[1:])[:], want[1:])            # an offset of 8 bytes
    empty = pigs_amd.grid_lookup(image, samples[:0])
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.float32
    assert not pigs_amd.grid_lookup(image, samples.clone().requires_grad_(True)).requires_grad      # no gradient
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pigs_amd.grid_lookup(image, samples.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pigs_amd.grid_lookup(image.cpu(), samples)
    with pytest.raises(ValueError, match="lo < hi"):
        pigs_amd.grid_lookup(image, samples, box=(1.0, -1.0))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        pigs_amd.grid_lookup(image.reshape(-1), samples)


def test_replay_inside_a_graphed_step(hip_lib):
    """Capturable: nothing synchronises and only the output is allocated; a replay follows samples rewritten in place."""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    H, W, box = 48, 80, (-2.5, 2.5)
    image = torch.arange(H * W, dtype=torch.float32, device="cuda").reshape(H, W)
    rng = np.random.default_rng(9)
    first = rng.uniform(-2.5, 2.5, (M_RANDOM, 2)).astype(np.float32)
    step = GraphedStep(lambda s: pigs_amd.grid_lookup(image, s, box=box), lambda: (torch.as_tensor(first, device="cuda"),))
    for trial in range(2):
        pts = rng.uniform(-2.6, 2.6, (M_RANDOM, 2)).astype(np.float32)
        step.inputs[0].copy_(torch.as_tensor(pts, device="cuda"))
        got = step().clone()
        torch.cuda.synchronize()
        iy, ix = expected_pixels(pts, H, W, box)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), iy * W + ix), trial
