"""CPU: the C ABI of the coupled residual (pigs_residual_coupled_forward / _backward: two constant c x c matrices mix
the channels under a per-point weight, include/pigs_amd.h) -- the symbols are there, the ABI number stays, the ctypes
struct has the header's layout, and bad arguments are refused before any HIP call (null device pointers, no GPU)."""
import ctypes
import os
import re

from pigs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIGS_ERR_INVALID, PIGS_ERR_UNSUPPORTED = 1, 2
NAMES = ("pigs_residual_coupled_forward", "pigs_residual_coupled_backward")
null = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # "a plan workspace": never dereferenced by a call that is refused


def coupling(**kw):
    t = _lib.PigsResidualCoupling()
    for k, v in kw.items():
        setattr(t, k, v)
    return ctypes.byref(t)


def forward(lib, dtype=0, d=2, c=2, N=4, M=4, cz=None, plan=null, out=FAKE):
    return lib.pigs_residual_coupled_forward(dtype, d, c, N, M, null, null, null, null, cz, null, out,
                                             plan, 1 << 20, plan, 1 << 20, null)


def backward(lib, dtype=0, d=2, c=2, N=4, M=4, cz=None, plan=null, gout=FAKE, grads=FAKE):
    return lib.pigs_residual_coupled_backward(dtype, d, c, N, M, null, null, null, null, cz, gout, grads, grads, grads,
                                              plan, 1 << 20, plan, 1 << 20, null)


def test_both_symbols_are_exported_declared_and_bound(hip_lib):
    header = open(os.path.join(ROOT, "include", "pigs_amd.h")).read()
    assert "typedef struct PigsResidualCoupling" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/pigs_amd.h"
        assert name in _lib.SIGNATURES and hasattr(raw, name) and hasattr(hip_lib, name)


def test_the_abi_number_stays(hip_lib):
    assert _lib.ABI_VERSION == hip_lib.pigs_abi_version() == 10


def test_the_struct_has_the_header_layout():
    """double a0, aL, cw; double couple0[4][4], couple_lap[4][4]; three pointers -- and the header says so."""
    t = _lib.PigsResidualCoupling
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(t) == 3 * 8 + 2 * 16 * 8 + 3 * ptr
    assert t.a0.offset == 0 and t.aL.offset == 8 and t.cw.offset == 16
    assert t.couple0.offset == 24 and t.couple_lap.offset == 24 + 128
    assert t.a0_pt.offset == 280 and t.aL_pt.offset == 280 + ptr and t.cw_pt.offset == 280 + 2 * ptr
    header = open(os.path.join(ROOT, "include", "pigs_amd.h")).read()
    body = re.search(r"typedef struct PigsResidualCoupling \{(.*?)\} PigsResidualCoupling;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [" ".join(x.split()) for x in body.split(";") if x.strip()]
    assert decls == ["double a0, aL, cw", "double couple0[4][4], couple_lap[4][4]", "const void *a0_pt, *aL_pt, *cw_pt"]
    # [ch][c']: the row is the output channel
    z = t()
    z.couple0[1][0] = 3.0
    assert (ctypes.c_double * 16).from_buffer(z, t.couple0.offset)[4] == 3.0


def test_a_null_struct_is_invalid(hip_lib):
    for plan in (null, FAKE):
        assert forward(hip_lib, cz=None, plan=plan) == PIGS_ERR_INVALID
        assert backward(hip_lib, cz=None, plan=plan) == PIGS_ERR_INVALID


def test_null_outputs_and_inputs_are_invalid(hip_lib):
    cz = coupling(a0=1.0)
    assert forward(hip_lib, cz=cz, out=null) == PIGS_ERR_INVALID
    assert backward(hip_lib, cz=cz, gout=null) == PIGS_ERR_INVALID
    assert backward(hip_lib, cz=cz, grads=null) == PIGS_ERR_INVALID
    for call in (forward, backward):
        assert call(hip_lib, cz=cz) == PIGS_ERR_INVALID          # null inputs with N, M > 0
        assert call(hip_lib, N=-1, cz=cz) == PIGS_ERR_INVALID


def test_a_plan_takes_float32_in_two_dimensions_with_two_channels(hip_lib):
    cz = coupling(a0=1.0, cw=1.0)
    for call in (forward, backward):
        assert call(hip_lib, dtype=1, cz=cz, plan=FAKE) == PIGS_ERR_UNSUPPORTED      # f64
        assert call(hip_lib, d=1, cz=cz, plan=FAKE) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, c=3, cz=cz, plan=FAKE) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, c=1, cz=cz, plan=FAKE) == PIGS_ERR_UNSUPPORTED


def test_dense_takes_one_or_two_dimensions_and_two_to_four_channels(hip_lib):
    cz = coupling(a0=1.0, cw=1.0)
    for call in (forward, backward):
        assert call(hip_lib, d=3, cz=cz) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, c=5, cz=cz) == PIGS_ERR_UNSUPPORTED
        assert call(hip_lib, c=1, cz=cz) == PIGS_ERR_UNSUPPORTED      # nothing to couple
        assert call(hip_lib, dtype=7, cz=cz) == PIGS_ERR_UNSUPPORTED
        for c in (2, 3, 4):                                            # compiled: as far as the null inputs
            assert call(hip_lib, c=c, cz=cz) == PIGS_ERR_INVALID
