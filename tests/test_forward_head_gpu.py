"""GPU: the head of a forward wave.  The forward asks for the order of the points with one scalar load
and requests the tile header, the row's list length and the first 2 x 16 list entries beside it, before it knows the
tile's mode or where its point is; the point and the records follow together.  None of it may change an output: point
sets in either order (a lattice read through the caller's array, points sorted into cells), a shape that changes under
the library's memory of the size, ragged last tiles, and the first forward of a plan with deferred lists (the same
head inside the launch that builds the lists) -- against the dense kernels."""
import numpy as np
import pytest
import torch

from pigs_amd import synthetic
from test_binned_gpu import random_gaussians, rel, dev32, TOL

pytestmark = pytest.mark.gpu
HOSTS = ["native", "ctypes"]


def settled_forward_only(host, t, pts, rounds=4, **kw):
    """A sampler whose last build ran on the library's memory of the sizes (index-tiled points, strips)."""
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(False, fuse="all", backend="binned", host=host, reuse_samples=False, **kw)
    outs = None
    with torch.no_grad():
        for _ in range(rounds):
            s.preprocess(t["means"], t["values"], None, t["conics"], pts)
            outs = [o.clone() for o in s.sample((0, 1, 2))]
            torch.cuda.synchronize()
    return s, outs


def dense_outputs(t, pts):
    from diff_gaussian_sampling import GaussianSampler
    d = GaussianSampler(False, backend="dense")
    with torch.no_grad():
        d.preprocess(t["means"], t["values"], None, t["conics"], pts)
        return d.sample((0, 1, 2))


@pytest.mark.parametrize("host", HOSTS)
def test_a_lattice_that_changes_shape_then_loses_its_order(hip_lib, host):
    """The library remembers a 512 x 128 lattice; then come 128 x 512 points (the same M, another row length), then the
    same points in no order (sorted into cells: the order words are zero and the points come from the sorted copy).
    Against the dense kernels on a slice of the points."""
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(64, 64, 0.7, seed=2)
    t = {k: gs[k].float().to(dev) for k in ("means", "values", "conics")}
    shape_a = synthetic.grid_samples(512, 128).float().to(dev)
    shape_b = synthetic.grid_samples(128, 512).float().to(dev)
    assert shape_a.shape == shape_b.shape
    perm = torch.randperm(shape_b.shape[0], generator=torch.Generator().manual_seed(7)).to(dev)
    settled_forward_only(host, t, shape_a)
    from diff_gaussian_sampling import GaussianSampler
    sub = torch.arange(0, shape_b.shape[0], 13, device=dev)
    for name, pts in (("another shape", shape_b), ("no order", shape_b[perm].contiguous())):
        s = GaussianSampler(False, fuse="all", backend="binned", host=host, reuse_samples=False)
        with torch.no_grad():
            s.preprocess(t["means"], t["values"], None, t["conics"], pts)
            outs = s.sample((0, 1, 2))
        want = dense_outputs(t, pts[sub].contiguous())
        for o, (a, b) in enumerate(zip(outs, want)):
            assert rel(a[sub], b.cpu().double().numpy()) < TOL, (name, o, rel(a[sub], b.cpu().double().numpy()))


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("M", [70 * 64 + 37, 3000, 4096 + 8])
def test_ragged_and_small_point_sets(hip_lib, host, M):
    """M not a multiple of 64 (positions behind the last point), M < 4 096 (never a lattice) and a row of a grid cut
    short: the dense kernels' numbers."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(M)
    means, con, values = random_gaussians(rng, 1500, 1, log_sigma_mean=-3.2, log_sigma_std=0.4)
    t = {"means": dev32(means), "values": dev32(values), "conics": dev32(con)}
    g = np.linspace(-1, 1, 8 * int(np.ceil(np.sqrt(M) / 8)))
    gx, gy = np.meshgrid(g, g, indexing="xy")
    pts = dev32(np.stack((gx, gy), -1).reshape(-1, 2)[:M])
    s, outs = settled_forward_only(host, t, pts, rounds=3)
    want = dense_outputs(t, pts)
    for o, (a, b) in enumerate(zip(outs, want)):
        assert rel(a, b.cpu().double().numpy()) < TOL, (o, rel(a, b.cpu().double().numpy()))


@pytest.mark.parametrize("host", HOSTS)
def test_first_forward_of_a_plan_with_deferred_lists(hip_lib, host):
    """PIGS_BUILD_DEFER_LISTS: the first forward runs inside the launch that builds the lists (plan_lists_forward_kernel)
    and reads headers and entries its own wave has just written -- through the same head."""
    dev = torch.device("cuda")
    gs = synthetic.lattice_gaussians(64, 64, 0.7, seed=3)
    t = {k: gs[k].float().to(dev) for k in ("means", "values", "conics")}
    for pts in (synthetic.grid_samples(256, 256).float().to(dev),
                (torch.rand((20000 + 37, 2), generator=torch.Generator().manual_seed(5)) * 2 - 1).float().to(dev)):
        s, outs = settled_forward_only(host, t, pts, rounds=3, defer_lists=True)
        want = dense_outputs(t, pts)
        for o, (a, b) in enumerate(zip(outs, want)):
            assert rel(a, b.cpu().double().numpy()) < TOL, (o, rel(a, b.cpu().double().numpy()))
