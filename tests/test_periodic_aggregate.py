"""CPU: the periodic neighbour-list entry points (pigs_aggregate_*_periodic, additive to ABI 10) are exported and
reject bad arguments before any HIP call; the sampler option validates without a GPU."""
import ctypes
import math

import pytest

PIGS_ERR_INVALID, PIGS_ERR_UNSUPPORTED = 1, 2
NEW = ("pigs_aggregate_lists_periodic", "pigs_aggregate_forward_periodic", "pigs_aggregate_backward_periodic")
P = ctypes.c_void_p(16)               # never dereferenced: every call below fails its checks first
NULL = ctypes.c_void_p(0)


def lists(lib, dtype=0, N=4, cap=4, q_max=36.0, lo=-1.0, period=2.0):
    return lib.pigs_aggregate_lists_periodic(dtype, N, cap, P, P, q_max, lo, period, NULL, 0, 1, P, P, P, P, P, NULL)


def forward(lib, dtype=0, N=4, cap=4, period=2.0):
    return lib.pigs_aggregate_forward_periodic(dtype, N, cap, 4, 4, 2, period, *([P] * 13), NULL)


def backward(lib, dtype=0, N=4, cap=4, period=2.0):
    return lib.pigs_aggregate_backward_periodic(dtype, N, cap, 4, 4, 2, period, *([P] * 15), P, 1 << 20, *([P] * 6), NULL)


def test_the_three_symbols_are_exported_and_the_abi_number_stays(hip_lib):
    from pigs_amd import _lib
    assert _lib.ABI_VERSION == hip_lib.pigs_abi_version() == 10
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    header = open(_lib.HERE + "/../include/pigs_amd.h").read()
    for name in NEW:
        assert name + "(" in header


@pytest.mark.parametrize("call", [lists, forward, backward])
def test_period_must_be_finite_and_positive(hip_lib, call):
    for period in (0.0, -2.0, math.nan, math.inf):
        assert call(hip_lib, period=period) == PIGS_ERR_INVALID


def test_lo_must_be_finite(hip_lib):
    for lo in (math.nan, math.inf, -math.inf):
        assert lists(hip_lib, lo=lo) == PIGS_ERR_INVALID
    assert lists(hip_lib, lo=1e308, period=1e308) == PIGS_ERR_INVALID      # lo + period overflows


@pytest.mark.parametrize("call", [lists, forward, backward])
def test_index_range_and_dtype(hip_lib, call):
    assert call(hip_lib, N=1 << 28, cap=4) == PIGS_ERR_UNSUPPORTED          # an entry is j | k << 28
    assert call(hip_lib, dtype=7) == PIGS_ERR_UNSUPPORTED


def test_the_plain_checks_still_apply(hip_lib):
    assert lists(hip_lib, cap=0) == PIGS_ERR_INVALID
    assert lists(hip_lib, q_max=0.0) == PIGS_ERR_INVALID
    assert forward(hip_lib, N=-1) == PIGS_ERR_INVALID
    assert backward(hip_lib, cap=0) == PIGS_ERR_INVALID


def test_a_library_without_the_symbols_asks_for_a_rebuild(hip_lib, monkeypatch):
    from pigs_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "pigs_aggregate_lists_periodic_missing", (ctypes.c_int, []))
    with pytest.raises(ImportError, match="rebuild"):
        _lib.load()


@pytest.mark.parametrize("host", ["native", "ctypes"])
def test_periodic_aggregate_needs_periodic(hip_lib, host):
    from diff_gaussian_sampling import GaussianSampler
    with pytest.raises(ValueError, match="periodic"):
        GaussianSampler(False, host=host, periodic_aggregate=True)
    s = GaussianSampler(False, host=host, periodic=(-1.0, 1.0), periodic_aggregate=True)
    assert s.periodic_aggregate is True
    with pytest.raises(ValueError, match="periodic"):
        s.periodic = None
    s.periodic_aggregate = False
    s.periodic = None
    assert s.periodic is None and s.periodic_aggregate is False
    with pytest.raises(ValueError, match="periodic"):
        s.periodic_aggregate = True
    assert GaussianSampler(False, host=host).periodic_aggregate is False
