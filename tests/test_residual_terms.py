"""CPU: the C ABI of the general residual (pigs_residual_terms_forward / _backward: per-point coefficients and an
advection term, include/pigs_amd.h) -- the symbols are there, the ABI number stays, and bad arguments are refused
before any HIP call (null device pointers, no GPU)."""
import ctypes
import os
import re

from pigs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIGS_ERR_INVALID, PIGS_ERR_UNSUPPORTED = 1, 2
NAMES = ("pigs_residual_terms_forward", "pigs_residual_terms_backward")
null = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # "a plan workspace": never dereferenced by a call that is refused


def terms(**kw):
    t = _lib.PigsResidualTerms()
    for k, v in kw.items():
        setattr(t, k, v)
    return ctypes.byref(t)


def forward(lib, dtype=0, d=2, c=1, N=4, M=4, tz=None, plan=null, out=FAKE):
    return lib.pigs_residual_terms_forward(dtype, d, c, N, M, null, null, null, null, tz, null, out, null,
                                           plan, 1 << 20, plan, 1 << 20, null)


def backward(lib, dtype=0, d=2, c=1, N=4, M=4, tz=None, plan=null, aux=null, gout=FAKE, grads=FAKE):
    return lib.pigs_residual_terms_backward(dtype, d, c, N, M, null, null, null, null, tz, gout, aux, grads, grads, grads,
                                            plan, 1 << 20, plan, 1 << 20, null)


def test_both_symbols_are_exported_declared_and_bound(hip_lib):
    header = open(os.path.join(ROOT, "include", "pigs_amd.h")).read()
    assert "typedef struct PigsResidualTerms" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/pigs_amd.h"
        assert name in _lib.SIGNATURES and hasattr(raw, name) and hasattr(hip_lib, name)


def test_the_abi_number_stays(hip_lib):
    assert _lib.ABI_VERSION == hip_lib.pigs_abi_version() == 10


def test_the_struct_has_the_header_layout():
    """double a0, a1[2], aL, adv; double advect_by[2][4]; four pointers."""
    t = _lib.PigsResidualTerms
    assert ctypes.sizeof(t) == 5 * 8 + 8 * 8 + 4 * ctypes.sizeof(ctypes.c_void_p)
    assert t.a1.offset == 8 and t.aL.offset == 24 and t.adv.offset == 32 and t.advect_by.offset == 40
    assert t.a0_pt.offset == 104 and t.adv_pt.offset == 104 + 3 * ctypes.sizeof(ctypes.c_void_p)


def test_null_terms_are_invalid(hip_lib):
    assert forward(hip_lib, tz=None) == PIGS_ERR_INVALID
    assert backward(hip_lib, tz=None) == PIGS_ERR_INVALID
    assert forward(hip_lib, tz=None, plan=FAKE) == PIGS_ERR_INVALID
    assert backward(hip_lib, tz=None, plan=FAKE) == PIGS_ERR_INVALID


def test_backward_with_advection_needs_aux(hip_lib):
    for plan in (null, FAKE):
        assert backward(hip_lib, tz=terms(adv=0.5), plan=plan) == PIGS_ERR_INVALID
        assert backward(hip_lib, tz=terms(adv_pt=4096), plan=plan) == PIGS_ERR_INVALID
    # without advection a null aux is fine: the call gets as far as the null inputs
    assert backward(hip_lib, tz=terms(a0=1.0)) == PIGS_ERR_INVALID
    assert backward(hip_lib, tz=terms(a0=1.0), gout=null) == PIGS_ERR_INVALID
    assert backward(hip_lib, tz=terms(a0=1.0), grads=null) == PIGS_ERR_INVALID
    assert forward(hip_lib, tz=terms(a0=1.0), out=null) == PIGS_ERR_INVALID


def test_a_plan_takes_float32_in_two_dimensions_with_up_to_two_channels(hip_lib):
    tz = terms(a0=1.0)
    for call in (forward, backward):
        assert call(hip_lib, dtype=1, tz=tz, plan=FAKE) == PIGS_ERR_UNSUPPORTED      # f64
        assert call(hip_lib, d=1, tz=tz, plan=FAKE) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, c=3, tz=tz, plan=FAKE) == PIGS_ERR_UNSUPPORTED


def test_the_dense_checks_still_apply(hip_lib):
    tz = terms(a0=1.0)
    for call in (forward, backward):
        assert call(hip_lib, d=3, tz=tz) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, c=5, tz=tz) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, dtype=7, tz=tz) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, N=-1, tz=tz) == PIGS_ERR_INVALID
        assert call(hip_lib, tz=tz) == PIGS_ERR_INVALID          # null inputs with N, M > 0
