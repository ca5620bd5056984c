"""CPU: the periodic domain (GaussianSampler(..., periodic=(lo, hi)), C ABI 10) as far as it goes without a device --
constructor validation on both hosts, and the two new C entry points rejecting bad arguments before any HIP call."""
import ctypes
import math

import pytest

HOSTS = ("native", "ctypes")


@pytest.mark.parametrize("host", HOSTS)
def test_constructor_validates_the_box(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(False, periodic=(-1, 1), host=host)
    assert s.periodic == (-1.0, 1.0)
    assert s.q_cut == max(s.q_max, s.q_max_backward, s.q_max_order3) == 44.0
    assert s._core.periodic == (-1.0, 1.0)
    assert GaussianSampler(False, host=host).periodic is None
    for bad in ((1, -1), (0.5, 0.5), (float("nan"), 1), (-1, float("inf")), (-1, 0, 1), (1,), 2.0, "ab", (None, 1)):
        with pytest.raises(ValueError):
            GaussianSampler(False, periodic=bad, host=host)


@pytest.mark.parametrize("host", HOSTS)
def test_periodic_preprocess_keeps_the_cpu_checks(hip_lib, host):
    """The images are built after the usual validation: CPU tensors and bad shapes fail as without periodic."""
    import torch
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(True, periodic=(-1, 1), host=host)
    means = torch.zeros(4, 2); values = torch.ones(4, 1); con = torch.ones(4, 3); pts = torch.zeros(8, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.preprocess(means, values, con, con, pts)
    with pytest.raises(ValueError):
        s.preprocess(torch.zeros(4), values, con, con, pts)
    assert s._inputs is None


def test_images_entry_point_rejects_bad_arguments_without_a_gpu(hip_lib):
    null = ctypes.c_void_p(0)
    f = hip_lib.pigs_periodic_images
    p = ctypes.c_void_p(16)           # never dereferenced: every call below fails its checks first
    ok = [p] * 6
    assert f(7, 1, 4, -1.0, 2.0, 44.0, *ok, null, null) == 2          # dtype
    assert f(0, 0, 4, -1.0, 2.0, 44.0, *ok, null, null) == 2          # c = 0
    assert f(1, 5, 4, -1.0, 2.0, 44.0, *ok, null, null) == 2          # c = 5
    assert f(0, 1, -1, -1.0, 2.0, 44.0, *ok, null, null) == 1         # negative N
    assert f(0, 1, 4, -1.0, 0.0, 44.0, *ok, null, null) == 1          # period 0
    assert f(0, 1, 4, -1.0, -2.0, 44.0, *ok, null, null) == 1         # negative period
    assert f(0, 1, 4, -1.0, math.nan, 44.0, *ok, null, null) == 1     # NaN period
    assert f(0, 1, 4, -1.0, math.inf, 44.0, *ok, null, null) == 1     # infinite period
    assert f(0, 1, 4, math.nan, 2.0, 44.0, *ok, null, null) == 1      # NaN lo
    assert f(0, 1, 4, -1.0, 2.0, 0.0, *ok, null, null) == 1           # q_cut
    for k in range(6):                                                # a null array with N > 0
        args = list(ok)
        args[k] = null
        assert f(0, 1, 4, -1.0, 2.0, 44.0, *args, null, null) == 1
    assert f(0, 1, 0, -1.0, 2.0, 44.0, *([null] * 6), null, null) == 0   # N = 0: nothing to launch


def test_fold_entry_point_rejects_bad_arguments_without_a_gpu(hip_lib):
    null = ctypes.c_void_p(0)
    f = hip_lib.pigs_periodic_images_backward
    p = ctypes.c_void_p(16)
    assert f(7, 1, 4, *([p] * 6), null) == 2                          # dtype
    assert f(0, 9, 4, *([p] * 6), null) == 2                          # c
    assert f(0, 1, -3, *([p] * 6), null) == 1                         # negative N
    for k in range(3, 6):                                             # a null output with N > 0
        args = [p] * 6
        args[k] = null
        assert f(0, 1, 4, *args, null) == 1
    assert f(0, 1, 0, *([null] * 6), null) == 0                       # N = 0


def test_abi_10_declares_the_periodic_entry_points(hip_lib):
    from pigs_amd import _lib
    assert _lib.ABI_VERSION == hip_lib.pigs_abi_version() == 10
    for name in ("pigs_periodic_images", "pigs_periodic_images_backward"):
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)


@pytest.mark.parametrize("host", HOSTS)
def test_periodic_is_settable_and_reaches_both_hosts(hip_lib, host):
    """Assigning ``sampler.periodic`` after construction validates the box and reaches the native core as well (the
    next preprocess uses it on either host)."""
    from diff_gaussian_sampling import GaussianSampler
    s = GaussianSampler(False, host=host)
    s.periodic = (0, 3)
    assert s.periodic == (0.0, 3.0)
    assert s._core.periodic == (0.0, 3.0)
    with pytest.raises(ValueError):
        s.periodic = (2, 1)
    assert s.periodic == (0.0, 3.0)
    s.periodic = None
    assert s.periodic is None
    assert s._core.periodic is None
    assert GaussianSampler(False, host=host, q_max_order3=50.0).q_cut == 50.0
