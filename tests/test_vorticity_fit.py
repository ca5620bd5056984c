"""CPU: the surface of GaussianSampler.vorticity_residual(data=...) and pigs_amd.grid_lookup() that needs no GPU -- the
three C ABI symbols, their ctypes signatures and argument checks, the exported names -- and the two numpy helpers that
the GPU tests (tests/test_vorticity_fit_gpu.py) take their expectations from, extensions of ``compose`` / ``adjoint`` of
tests/test_vorticity_residual.py:

  compose3(now7, prev7, tau, nu, dt, time_term, data, data_weight)   [M, 3] = compose's two columns and
                                                                     data_weight (w_now - data)
  adjoint3(gout3, now7, prev7, tau, nu, dt, time_term, data_weight)  the gradient [M, 7] that arrives at ``now7``

``adjoint3`` is pinned as the derivative of ``compose3`` by central differences (compose3 is quadratic in ``now7``: the
quotient is exact up to rounding), and column 2 against the reference's data lines (main_pn.py:209-210,
test_initialize.py:135-136) written in numpy with their own index expressions.
"""
import ctypes

import numpy as np
import pytest

from test_vorticity import combine
from test_vorticity_residual import CONSTANTS, adjoint, compose


def compose3(now7, prev7, tau, nu, dt, time_term=1.0, data=None, data_weight=1.0):
    now7 = np.asarray(now7, dtype=np.float64)
    fit = data_weight * (now7[:, 3] - np.asarray(data, dtype=np.float64).reshape(-1))
    return np.concatenate((compose(now7, prev7, tau, nu, dt, time_term), fit[:, None]), -1)


def adjoint3(gout3, now7, prev7, tau, nu, dt, time_term=1.0, data_weight=1.0):
    """The gradient with respect to ``now7`` of sum(gout3 * compose3(now7, ...)); ``data`` does not enter."""
    gout3 = np.asarray(gout3, dtype=np.float64)
    g = adjoint(gout3[:, :2], now7, prev7, tau, nu, dt, time_term)
    g[:, 3] += gout3[:, 2] * data_weight
    return g


def reference_pixels(samples, res):
    """main_pn.py:206-207 / test_initialize.py:132-133 in numpy, in the samples' dtype: the flat pixel index."""
    coords = np.clip(((samples + samples.dtype.type(1.0)) / samples.dtype.type(2.0) * samples.dtype.type(res)).astype(np.int64), 0, res - 1)
    return coords[:, 1] * res + coords[:, 0]


@pytest.mark.parametrize("k", CONSTANTS)
@pytest.mark.parametrize("with_prev", [True, False])
@pytest.mark.parametrize("data_weight", [np.sqrt(5.0), -0.7])
def test_adjoint3_is_the_derivative_of_compose3(k, with_prev, data_weight):
    rng = np.random.default_rng(0)
    M, h = 41, 1e-3
    now, gout, tau, data = rng.normal(size=(M, 7)), rng.normal(size=(M, 3)), rng.uniform(0, 1, M), rng.normal(size=M)
    prev = rng.normal(size=(M, 7)) if with_prev else None
    g = adjoint3(gout, now, prev, tau, data_weight=data_weight, **k)
    f = lambda x: (gout * compose3(x, prev, tau, data=data, data_weight=data_weight, **k)).sum()      # noqa: E731
    for _ in range(8):      # random directions
        dn = rng.normal(size=(M, 7))
        fd = (f(now + h * dn) - f(now - h * dn)) / (2 * h)
        assert abs(fd - (g * dn).sum()) <= 1e-9 * max(abs(fd), 1.0), (fd, (g * dn).sum())
    for col in range(7):      # column by column, so that no two columns can trade places
        dn = np.zeros((M, 7))
        dn[:, col] = rng.normal(size=M)
        fd = (f(now + h * dn) - f(now - h * dn)) / (2 * h)
        assert abs(fd - (g * dn).sum()) <= 1e-9 * max(abs(fd), 1.0), (col, fd, (g * dn).sum())
    for out_col in range(3):      # and each of the three outputs alone
        go = np.zeros((M, 3))
        go[:, out_col] = gout[:, out_col]
        dn = rng.normal(size=(M, 7))
        fo = lambda x: (go * compose3(x, prev, tau, data=data, data_weight=data_weight, **k)).sum()      # noqa: E731
        fd = (fo(now + h * dn) - fo(now - h * dn)) / (2 * h)
        assert abs(fd - (adjoint3(go, now, prev, tau, data_weight=data_weight, **k) * dn).sum()) <= 1e-9 * max(abs(fd), 1.0)


def test_compose3_keeps_the_two_columns_of_compose():
    rng = np.random.default_rng(1)
    M = 37
    now, prev, tau, data = rng.normal(size=(M, 7)), rng.normal(size=(M, 7)), rng.uniform(0, 1, M), rng.normal(size=M)
    got = compose3(now, prev, tau, 0.05, 0.01, 1.0, data, 2.0)
    assert got.shape == (M, 3) and np.array_equal(got[:, :2], compose(now, prev, tau, 0.05, 0.01, 1.0))


def test_column_2_is_the_recon_loss_of_the_navier_stokes_loop():
    """main_pn.py:202-212: recon_loss = 5 mean((w_samples[-1] - take(desired, coords))^2), w of the CURRENT level; the
    step loss of model_pn.py:848-849 plus it is compose3(...)^2 . mean(0) . sum() at data_weight = sqrt(5)."""
    rng = np.random.default_rng(5)
    M, res, nu, dt = 61, 16, 0.05, 0.01
    levels = [{k: rng.normal(size=(M,) + (2,) * k + (2,)) for k in range(4)} for _ in range(2)]
    time_samples = rng.uniform(0, 1, M)
    samples = rng.uniform(-1, 1, (M, 2)).astype(np.float32)
    desired = rng.normal(size=(res, res))
    coords = reference_pixels(samples, res)
    w_samples = [o[1][:, 0, 1] - o[1][:, 1, 0] for o in levels]                          # model_pn.py:779
    recon_loss = 5.0 * np.mean((w_samples[-1].squeeze() - np.take(desired, coords).squeeze()) ** 2)      # main_pn.py:210
    data = desired.reshape(-1)[coords]
    out = compose3(combine(levels[-1]), combine(levels[-2]), time_samples, nu, dt, 1.0, data, np.sqrt(5.0))
    assert abs((out[:, 2] ** 2).mean() - recon_loss) <= 1e-13 * max(recon_loss, 1.0)
    two = compose(combine(levels[-1]), combine(levels[-2]), time_samples, nu, dt, 1.0)
    step = (two[:, 0] ** 2).mean() + (two[:, 1] ** 2).mean() + recon_loss
    assert abs((out ** 2).mean(0).sum() - step) <= 1e-13 * max(step, 1.0)


def test_column_2_is_the_loss_of_the_initialisation_fit():
    """test_initialize.py:112-114, 135-136: the vorticity of the field's first derivatives against the image's pixels,
    and the divergence beside it; nu = dt = time_term = 0 leaves column 1 exact zeros."""
    rng = np.random.default_rng(6)
    M, res = 47, 32
    o = {k: rng.normal(size=(M,) + (2,) * k + (2,)) for k in range(4)}
    ux = o[1]
    samples = rng.uniform(-1, 1, (M, 2)).astype(np.float32)
    img = rng.normal(size=(res, res))
    vorticity = ux[:, 0, 1] - ux[:, 1, 0]                                                # :112-114
    divergence = ux[:, 0, 0] + ux[:, 1, 1]
    coords = reference_pixels(samples, res)
    loss = np.mean((vorticity - np.take(img, coords)) ** 2)                              # :135
    out = compose3(combine(o), None, 1.0, 0.0, 0.0, 0.0, img.reshape(-1)[coords], 1.0)
    assert np.abs(out[:, 2] - (vorticity - img.reshape(-1)[coords])).max() <= 1e-13
    assert abs((out[:, 2] ** 2).mean() - loss) <= 1e-13 and np.abs(out[:, 0] - divergence).max() <= 1e-13
    assert np.array_equal(out[:, 1], np.zeros(M))


def test_names():
    import pigs_amd
    from pigs_amd import lookup, sampler
    assert pigs_amd.VORTICITY_FIT_COLUMNS == ("div", "r", "fit")
    assert pigs_amd.VORTICITY_FIT_COLUMNS is sampler.VORTICITY_FIT_COLUMNS
    assert pigs_amd.VORTICITY_FIT_COLUMNS[:2] == pigs_amd.VORTICITY_RESIDUAL_COLUMNS
    assert pigs_amd.grid_lookup is lookup.grid_lookup
    import inspect
    params = inspect.signature(sampler.GaussianSampler.vorticity_residual).parameters
    assert list(params) == ["self", "nu", "dt", "prev", "tau", "time_term", "data", "data_weight"]
    assert params["data"].default is None and params["data_weight"].default == 1.0
    assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("time_term", "data", "data_weight"))
    assert list(inspect.signature(lookup.grid_lookup).parameters) == ["image", "samples", "box"]
    assert inspect.signature(lookup.grid_lookup).parameters["box"].default == (-1.0, 1.0)


def test_both_cores_carry_the_underscored_method():
    import inspect
    from pigs_amd import _pigs_host, host_ctypes
    want = ["self", "nu", "dt", "time_term", "tau", "tau_field", "prev", "data", "data_weight"]
    assert list(inspect.signature(host_ctypes.SamplerCore._vorticity_fit).parameters) == want
    assert hasattr(_pigs_host.SamplerCore, "_vorticity_fit")
    assert all(n in _pigs_host.SamplerCore._vorticity_fit.__doc__ for n in want[1:])


def test_lib_binds_the_three_symbols_with_the_documented_arguments(hip_lib):
    from pigs_amd import _lib
    fwd, bwd = _lib.SIGNATURES["pigs_vorticity_fit_forward"], _lib.SIGNATURES["pigs_vorticity_fit_backward"]
    sibling = (_lib.SIGNATURES["pigs_vorticity_residual_forward"], _lib.SIGNATURES["pigs_vorticity_residual_backward"])
    for sig, sib in zip((fwd, bwd), sibling):      # the arguments of the sibling, the block apart
        assert sig[0] is ctypes.c_int and len(sig[1]) == len(sib[1])
        assert sig[1][:7] == sib[1][:7] and sig[1][8:] == sib[1][8:]
        assert sig[1][7] is ctypes.POINTER(_lib.PigsVorticityFit)
    assert [n for n, _ in _lib.PigsVorticityFit._fields_] == ["nu", "dt", "time_term", "tau", "data_weight", "tau_pt", "data"]
    assert ctypes.sizeof(_lib.PigsVorticityFit) == 56
    look = _lib.SIGNATURES["pigs_grid_lookup"]
    assert look[0] is ctypes.c_int
    assert look[1] == [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double,
                       ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert hip_lib.pigs_vorticity_fit_forward.argtypes == fwd[1]
    assert hip_lib.pigs_vorticity_fit_backward.argtypes == bwd[1]
    assert hip_lib.pigs_grid_lookup.argtypes == look[1]
    assert hip_lib.pigs_abi_version() == 10              # additive: no version bump


def test_argument_validation_needs_no_gpu(hip_lib):
    """Bad arguments are rejected before any HIP call (1 = invalid, 2 = unsupported)."""
    from pigs_amd import _lib
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below returns before a launch
    pz = ctypes.byref(_lib.PigsVorticityFit(0.05, 0.01, 1.0, 1.0, 2.0, None, 256))
    no_data = ctypes.byref(_lib.PigsVorticityFit(0.05, 0.01, 1.0, 1.0, 2.0, None, None))
    f, b = hip_lib.pigs_vorticity_fit_forward, hip_lib.pigs_vorticity_fit_backward
    assert f(0, 4, 4, one, one, one, one, pz, null, null, null, null, 0, null, 0, null) == 1          # no output
    assert f(0, 4, 4, one, one, one, one, None, null, one, null, null, 0, null, 0, null) == 1         # no params
    assert f(0, 4, 4, one, one, one, one, no_data, null, one, null, null, 0, null, 0, null) == 1      # no data
    assert f(0, 4, 4, null, one, one, one, pz, null, one, null, null, 0, null, 0, null) == 1          # no means
    assert f(7, 4, 4, one, one, one, one, pz, null, one, null, null, 0, null, 0, null) == 2           # dtype
    assert f(0, -1, 4, one, one, one, one, pz, null, one, null, null, 0, null, 0, null) == 1          # negative size
    assert f(1, 4, 4, one, one, one, one, pz, null, one, null, one, 64, one, 64, null) == 2           # binned float64
    assert b(0, 4, 4, one, one, one, one, pz, null, one, one, one, one, null, 0, null, 0, null) == 1      # no incoming gradient
    assert b(0, 4, 4, one, one, one, one, None, one, one, one, one, one, null, 0, null, 0, null) == 1     # no params
    assert b(0, 4, 4, one, one, one, one, pz, one, one, one, null, one, null, 0, null, 0, null) == 1      # no g_conics
    assert b(0, 4, 4, one, one, one, one, pz, one, null, one, one, one, null, 0, null, 0, null) == 1      # no aux
    assert b(7, 4, 4, one, one, one, one, no_data, one, one, one, one, one, null, 0, null, 0, null) == 2  # dtype; data unread
    assert b(1, 4, 4, one, one, one, one, pz, one, one, one, one, one, one, 64, one, 64, null) == 2       # binned float64
    g = hip_lib.pigs_grid_lookup
    assert g(0, 0, 8, 8, 4, -1.0, 1.0, null, one, one, null) == 1          # no image
    assert g(0, 0, 8, 8, 4, -1.0, 1.0, one, one, null, null) == 1          # no output
    assert g(0, 0, 0, 8, 4, -1.0, 1.0, one, one, one, null) == 1           # no rows
    assert g(0, 0, 8, 8, -1, -1.0, 1.0, one, one, one, null) == 1          # negative size
    assert g(0, 0, 8, 8, 4, 1.0, 1.0, one, one, one, null) == 1            # hi <= lo
    assert g(0, 0, 8, 8, 4, 1.0, float("nan"), one, one, one, null) == 1
    assert g(0, 0, 8, 8, 4, 1.0, 1.0 + 1e-12, one, one, one, null) == 1    # empty once rounded to the samples' float32
    assert g(0, 1, 8, 8, 0, 1.0, 1.0 + 1e-12, null, null, null, null) == 0   # M = 0: nothing to do
    assert g(2, 0, 8, 8, 4, -1.0, 1.0, one, one, one, null) == 2           # dtype
    assert g(0, 0, (1 << 24) + 1, 8, 4, -1.0, 1.0, one, one, one, null) == 2


def test_python_refusals_need_no_gpu():
    """data of the wrong length, on the CPU or requiring grad are refused by the facade before anything is launched
    (the checks are those of ``tau``); grid_lookup refuses a 1-D image, hi <= lo and CPU tensors."""
    import torch
    from pigs_amd import lookup
    from pigs_amd.sampler import GaussianSampler

    class Bound(GaussianSampler):      # the facade's checks alone: inputs bound without a core
        def __init__(self):
            pass

        def _require_inputs(self):
            return self._bound

    s = Bound()
    M = 6
    s._bound = tuple(torch.zeros(shape, device="meta") for shape in ((3, 2), (3, 2), (3, 3), (M, 2)))      # "the GPU"
    with pytest.raises(ValueError, match="shape"):
        s.vorticity_residual(0.1, 0.1, data=torch.zeros(M + 1, device="meta"))
    with pytest.raises(ValueError, match="constants"):
        s.vorticity_residual(0.1, 0.1, data=torch.zeros(M, requires_grad=True))
    with pytest.raises(RuntimeError, match="device"):
        s.vorticity_residual(0.1, 0.1, data=torch.zeros(M))
    with pytest.raises(RuntimeError, match="tensor"):
        s.vorticity_residual(0.1, 0.1, data=1.0)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        lookup.grid_lookup(torch.zeros(8), torch.zeros(4, 2))
    with pytest.raises(ValueError, match=r"\[M, 2\]"):
        lookup.grid_lookup(torch.zeros(8, 8), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="lo < hi"):
        lookup.grid_lookup(torch.zeros(8, 8), torch.zeros(4, 2), box=(1.0, 1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lookup.grid_lookup(torch.zeros(8, 8), torch.zeros(4, 2))
    with pytest.raises(TypeError):
        lookup.grid_lookup(torch.zeros(8, 8, dtype=torch.int32), torch.zeros(4, 2))
