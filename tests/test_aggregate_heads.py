"""CPU: the C ABI of aggregate_neighbors_heads (all heads of a layer in one launch; pigs_amd/csrc/aggregate.hip,
include/pigs_amd.h) -- the four symbols, the size rule and the argument checks, none of which needs a GPU.

The size rule is restated here from the header's text: at most 128 components per kernel (L + 2E, H K + F,
H (L + K)) and, with PART = 136 values of a wave's partial result, four wave regions of
    forward            max(64 ((L + 4F) | 1), H PART)
    backward by rows   H PART + max(64 ((H K + F) | 1), PART)
    backward by cols   max(64 ((H (L + K)) | 1), PART)
values within PIGS_AGGREGATE_LDS_MAX bytes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pigs_aggregate_heads_forward", "pigs_aggregate_heads_backward", "pigs_aggregate_heads_lds_bytes",
           "pigs_aggregate_heads_backward_scratch_bytes")
LDS_MAX = 163840
OK, INVALID, UNSUPPORTED = 0, 1, 2
F32, F64 = 0, 1

# (dtype, H, L, K, F, admitted)
SHAPES = [
    (F32, 2, 16, 16, 6, True), (F64, 2, 16, 16, 6, True),              # the model's shape
    (F32, 2, 2, 4, 5, True), (F32, 3, 2, 4, 5, True), (F32, 4, 2, 4, 5, True),      # the reference test's shape
    (F64, 2, 2, 4, 5, True), (F64, 3, 2, 4, 5, True), (F64, 4, 2, 4, 5, True),
    (F32, 4, 16, 16, 6, True),                                          # 128 components by columns: 132 096 B
    (F64, 4, 16, 16, 6, False),                                         # the same in float64: 264 192 B
    (F64, 3, 16, 16, 6, False),                                         # stride 97 by columns: 198 656 B
    (F32, 3, 16, 16, 6, True),
    (F32, 4, 20, 16, 2, False),                                         # H (L + K) = 144 components
    (F32, 2, 8, 64, 6, False),                                          # H K + F = 134 components
    (F32, 2, 80, 4, 6, False),                                          # L + 2E = 130 components
    (F32, 2, 1, 1, 0, True), (F64, 4, 1, 1, 0, True),                   # the merge region (H PART) is the forward's largest
    (F64, 2, 30, 9, 3, True), (F64, 2, 30, 10, 3, False),               # stride 79 / 81 by columns: 161 792 / 165 888 B
]


def lds_bytes(dtype, H, L, K, F):
    """What pigs_aggregate_heads_lds_bytes returns for 2 <= H <= 4: 0 beyond 128 components, else the bytes."""
    if L + 2 * (4 * F + 1) > 128 or H * K + F > 128 or H * (L + K) > 128:
        return 0
    part = 136
    forward = max(64 * ((L + 4 * F) | 1), H * part)
    by_rows = H * part + max(64 * ((H * K + F) | 1), part)
    by_cols = max(64 * ((H * (L + K)) | 1), part)
    return (8 if dtype == F64 else 4) * 4 * max(forward, by_rows, by_cols)


def admitted(dtype, H, L, K, F):
    return 2 <= H <= 4 and 0 < lds_bytes(dtype, H, L, K, F) <= LDS_MAX


def test_header_exports_and_signatures(hip_lib):
    from pigs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/pigs_amd.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert hip_lib.pigs_abi_version() == _lib.ABI_VERSION == 10          # additive: the number stays
    i, i64, vp, sz, dbl = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    head = [i, i64, i64, i, i, i, i, dbl]                 # dtype, N, cap, H, L, K, F, period
    assert _lib.SIGNATURES["pigs_aggregate_heads_lds_bytes"] == (sz, [i] * 5)
    assert _lib.SIGNATURES["pigs_aggregate_heads_backward_scratch_bytes"] == (sz, [i, i64, i, i, i])
    assert _lib.SIGNATURES["pigs_aggregate_heads_forward"] == (i, head + [vp] * 14)
    assert _lib.SIGNATURES["pigs_aggregate_heads_backward"] == (i, head + [vp] * 16 + [sz] + [vp] * 7)

    def params(name):         # the header's parameter list, as ctypes kinds
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = []
        for p in decl.split(","):
            p = p.strip()
            kinds.append(vp if "*" in p else {"int": i, "int64_t": i64, "size_t": sz, "double": dbl}[p.split()[0]])
        return kinds
    for name in SYMBOLS:
        assert params(name) == _lib.SIGNATURES[name][1], name


def test_size_rule_matches_its_python_mirror(hip_lib):
    from pigs_amd import aggregate as A
    import torch
    assert A.LDS_MAX == LDS_MAX
    header = open(os.path.join(ROOT, "include", "pigs_amd.h")).read()
    assert int(re.search(r"#define PIGS_AGGREGATE_HEADS_MAX (\d+)", header).group(1)) == A.MAX_HEADS == 4
    seen = set()
    for dtype, H, L, K, F, want in SHAPES:
        assert admitted(dtype, H, L, K, F) == want, (dtype, H, L, K, F)
        assert hip_lib.pigs_aggregate_heads_lds_bytes(dtype, H, L, K, F) == lds_bytes(dtype, H, L, K, F), (dtype, H, L, K, F)
        dt = torch.float64 if dtype == F64 else torch.float32
        assert (A.heads_refusal(dt, H, L, K, F) is None) == want
        seen.add(want)
    assert seen == {True, False}
    # the figures the design table quotes for the model's shape
    assert lds_bytes(F32, 2, 16, 16, 6) == 66560 and lds_bytes(F64, 2, 16, 16, 6) == 133120
    # H = 1 is the single-head rule; arguments out of range give 0
    for dtype, L, K, F in ((F32, 16, 16, 6), (F64, 2, 4, 5), (F64, 16, 100, 2)):
        assert hip_lib.pigs_aggregate_heads_lds_bytes(dtype, 1, L, K, F) == hip_lib.pigs_aggregate_lds_bytes(dtype, L, K, F)
    for bad in ((7, 2, 16, 16, 6), (F32, 0, 16, 16, 6), (F32, 5, 16, 16, 6), (F32, 2, 0, 16, 6), (F32, 2, 16, 129, 6)):
        assert hip_lib.pigs_aggregate_heads_lds_bytes(*bad) == 0, bad
    # scratch: dacc [N][H][W], D [N][H], per-row d frequencies [N][F], rounded up to 256 bytes
    for dtype, N, H, L, F in ((F32, 1600, 2, 16, 6), (F64, 25, 3, 2, 5), (F32, 0, 2, 16, 6)):
        W = L + 2 * (4 * F + 1)
        want = -(-(8 if dtype == F64 else 4) * N * (H * (W + 1) + F) // 256) * 256
        assert hip_lib.pigs_aggregate_heads_backward_scratch_bytes(dtype, N, H, L, F) == want
    assert hip_lib.pigs_aggregate_heads_backward_scratch_bytes(F32, 100, 1, 16, 6) == \
        hip_lib.pigs_aggregate_backward_scratch_bytes(F32, 100, 16, 6)


def calls(hip_lib):
    dummy = ctypes.c_void_p(16)           # never dereferenced: N = 0 returns after the checks, before any HIP call

    def forward(dtype, H, L, K, F, N=0, period=0.0, p=dummy):
        return hip_lib.pigs_aggregate_heads_forward(dtype, N, 1, H, L, K, F, period, *([p] * 14))

    def backward(dtype, H, L, K, F, N=0, period=0.0, p=dummy):
        return hip_lib.pigs_aggregate_heads_backward(dtype, N, 1, H, L, K, F, period, *([p] * 16), 0, *([p] * 7))
    return forward, backward


def test_entries_check_sizes_before_any_hip_call(hip_lib):
    for call in calls(hip_lib):
        for dtype, H, L, K, F, want in SHAPES:
            assert call(dtype, H, L, K, F) == (OK if want else UNSUPPORTED), (call.__name__, dtype, H, L, K, F)
        assert call(F32, 0, 16, 16, 6) == UNSUPPORTED
        assert call(F32, 5, 16, 16, 6) == UNSUPPORTED
        assert call(F32, -1, 16, 16, 6) == UNSUPPORTED
        assert call(7, 2, 16, 16, 6) == UNSUPPORTED
        assert call(F32, 1, 16, 16, 6) == OK                      # H = 1: the single-head kernels and their rule
        assert call(F64, 1, 16, 100, 2) == UNSUPPORTED            # ... which refuses this one (239 616 B by columns)
        assert call(F32, 2, 0, 16, 6) == INVALID and call(F32, 2, 16, 16, -1) == INVALID
        assert call(F32, 2, 16, 16, 6, N=-1) == INVALID
        assert call(F32, 2, 16, 16, 6, period=2.0) == OK          # lists of the torus
        assert call(F32, 2, 16, 16, 6, period=-2.0) == INVALID
        assert call(F32, 2, 16, 16, 6, period=float("nan")) == INVALID
        # null pointers with N > 0: refused before any HIP call, after the size rule
        assert call(F32, 2, 16, 16, 6, N=4, p=ctypes.c_void_p(0)) == INVALID
        assert call(F64, 4, 16, 16, 6, N=4, p=ctypes.c_void_p(0)) == UNSUPPORTED
    # a scratch block that is too small
    _, backward = calls(hip_lib)
    assert backward(F32, 2, 16, 16, 6, N=4) == 4                  # PIGS_ERR_WORKSPACE


def test_sampler_method_exists_on_both_hosts(hip_lib):
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd import _pigs_host
    assert callable(getattr(GaussianSampler, "aggregate_neighbors_heads"))
    assert hasattr(_pigs_host.SamplerCore, "aggregate_neighbors_heads")
