"""CPU: the surface of GaussianSampler.vorticity_residual() that needs no GPU -- the two C ABI symbols, their ctypes
signatures and argument checks, the exported column names -- and the two numpy helpers that the GPU tests
(tests/test_vorticity_residual_gpu.py) take their expectations from:

  compose(now7, prev7, tau, nu, dt, time_term)          the two columns (div_b, r) from the seven vorticity terms of two
                                                        time levels (tests/test_vorticity.py combine gives the seven)
  adjoint(gout2, now7, prev7, tau, nu, dt, time_term)   the gradient [M, 7] that arrives at ``now7`` when gout2 [M, 2]
                                                        arrives at compose()

``adjoint`` is pinned as the derivative of ``compose`` by central differences (compose is quadratic in ``now7``, so the
difference quotient is exact up to rounding), and ``compose`` is pinned against the reference's own lines for its three
integration rules (model_pn.py:794-818, 629-631, 830, 848), written here in numpy with the index expressions used there.
"""
import ctypes

import numpy as np
import pytest

from test_vorticity import combine


def compose(now7, prev7, tau, nu, dt, time_term=1.0):
    """[M, 2] = (div_b, time_term (w_now - w_prev) - dt (nu lap_w_b - u_b . grad w_b)), X_b = tau X_now + (1 - tau) X_prev.
    ``prev7`` None reads as zeros; ``tau`` a float or [M]."""
    now7 = np.asarray(now7, dtype=np.float64)
    prev7 = np.zeros_like(now7) if prev7 is None else np.asarray(prev7, dtype=np.float64)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64).reshape(-1), (now7.shape[0],))[:, None]
    b = tau * now7 + (1 - tau) * prev7
    u_x, u_y, div, _, w_x, w_y, lap_w = (b[:, k] for k in range(7))
    r = time_term * (now7[:, 3] - prev7[:, 3]) - dt * (nu * lap_w - (u_x * w_x + u_y * w_y))
    return np.stack((div, r), -1)


def adjoint(gout2, now7, prev7, tau, nu, dt, time_term=1.0):
    """The gradient with respect to ``now7`` of sum(gout2 * compose(now7, ...))."""
    now7 = np.asarray(now7, dtype=np.float64)
    gout2 = np.asarray(gout2, dtype=np.float64)
    prev7 = np.zeros_like(now7) if prev7 is None else np.asarray(prev7, dtype=np.float64)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64).reshape(-1), (now7.shape[0],))
    b = tau[:, None] * now7 + (1 - tau[:, None]) * prev7
    g_d, g_r = gout2[:, 0], gout2[:, 1]
    k = g_r * dt * tau
    g = np.zeros_like(now7)
    g[:, 0], g[:, 1] = k * b[:, 4], k * b[:, 5]
    g[:, 2] = g_d * tau
    g[:, 3] = g_r * time_term
    g[:, 4], g[:, 5] = k * b[:, 0], k * b[:, 1]
    g[:, 6] = -k * nu
    return g


CONSTANTS = [dict(nu=0.05, dt=0.01, time_term=1.0), dict(nu=1.3, dt=-1.0, time_term=0.0), dict(nu=0.4, dt=0.7, time_term=-2.5)]


@pytest.mark.parametrize("k", CONSTANTS)
@pytest.mark.parametrize("with_prev", [True, False])
def test_adjoint_is_the_derivative_of_compose(k, with_prev):
    rng = np.random.default_rng(0)
    M, h = 41, 1e-3
    now, gout, tau = rng.normal(size=(M, 7)), rng.normal(size=(M, 2)), rng.uniform(0, 1, M)
    prev = rng.normal(size=(M, 7)) if with_prev else None
    g = adjoint(gout, now, prev, tau, **k)
    f = lambda x: (gout * compose(x, prev, tau, **k)).sum()      # noqa: E731
    for _ in range(8):      # random directions
        dn = rng.normal(size=(M, 7))
        fd = (f(now + h * dn) - f(now - h * dn)) / (2 * h)
        assert abs(fd - (g * dn).sum()) <= 1e-9 * max(abs(fd), 1.0), (fd, (g * dn).sum())
    for col in range(7):      # column by column, so that no two columns can trade places
        dn = np.zeros((M, 7))
        dn[:, col] = rng.normal(size=M)
        fd = (f(now + h * dn) - f(now - h * dn)) / (2 * h)
        assert abs(fd - (g * dn).sum()) <= 1e-9 * max(abs(fd), 1.0), (col, fd, (g * dn).sum())
    for out_col in range(2):      # and each of the two outputs alone
        go = np.zeros((M, 2))
        go[:, out_col] = gout[:, out_col]
        dn = rng.normal(size=(M, 7))
        fo = lambda x: (go * compose(x, prev, tau, **k)).sum()      # noqa: E731
        fd = (fo(now + h * dn) - fo(now - h * dn)) / (2 * h)
        assert abs(fd - (adjoint(go, now, prev, tau, **k) * dn).sum()) <= 1e-9 * max(abs(fd), 1.0)


def reference_lines(rule, levels, time_samples, nu, dt):
    """compute_loss of the reference's model for Problem.NAVIER_STOKES, its lines as written there; ``levels`` is the
    list of {order: array} the model appends to in Model.sample (:770-781).  Returns (the divergence that :848 squares,
    wt - rhs of :849).  The reference defines wx / wxx under TRAPEZOID only (:801-805); under FORWARD and BACKWARD they are
    selected like u, ux and uxx (:806-813)."""
    u_samples = [o[0] for o in levels]
    ux_samples = [o[1] for o in levels]
    uxx_samples = [o[2] for o in levels]
    w_samples = [o[1][:, 0, 1] - o[1][:, 1, 0] for o in levels]                           # :779
    wx_samples = [o[2][..., 0, 1] - o[2][..., 1, 0] for o in levels]                      # :780
    wxx_samples = [o[3][..., 0, 1] - o[3][..., 1, 0] for o in levels]                     # :781
    if rule == "TRAPEZOID":
        u_sample = time_samples.reshape(-1, 1) * u_samples[-1] \
            + (1 - time_samples.reshape(-1, 1)) * u_samples[-2]
        ux = time_samples.reshape(-1, 1, 1) * ux_samples[-1] \
            + (1 - time_samples.reshape(-1, 1, 1)) * ux_samples[-2]
        uxx = time_samples.reshape(-1, 1, 1, 1) * uxx_samples[-1] \
            + (1 - time_samples.reshape(-1, 1, 1, 1)) * uxx_samples[-2]
        wx = time_samples.reshape(-1, 1) * wx_samples[-1] \
            + (1 - time_samples.reshape(-1, 1)) * wx_samples[-2]
        wxx = time_samples.reshape(-1, 1, 1) * wxx_samples[-1] \
            + (1 - time_samples.reshape(-1, 1, 1)) * wxx_samples[-2]
    elif rule == "FORWARD":
        ux, uxx, u_sample, wx, wxx = ux_samples[-2], uxx_samples[-2], u_samples[-2], wx_samples[-2], wxx_samples[-2]
    elif rule == "BACKWARD":
        ux, uxx, u_sample, wx, wxx = ux_samples[-1], uxx_samples[-1], u_samples[-1], wx_samples[-1], wxx_samples[-1]
    assert uxx.shape == uxx_samples[-1].shape
    wt = w_samples[-1] - w_samples[-2]                                                    # :818
    u = u_sample
    pde_rhs = nu * (wxx[:, 0, 0] + wxx[:, 1, 1]) \
        - (u[:, 0] * wx[:, 0] + u[:, 1] * wx[:, 1])                                       # :630-631
    rhs = dt * pde_rhs                                                                    # :830
    return ux[:, 0, 0] + ux[:, 1, 1], wt - rhs                                            # :848, :849


@pytest.mark.parametrize("rule", ["TRAPEZOID", "BACKWARD", "FORWARD"])
def test_compose_is_the_references_loss_under_its_three_rules(rule):
    rng = np.random.default_rng(3)
    M, nu, dt = 53, 0.05, 0.01
    levels = [{k: rng.normal(size=(M,) + (2,) * k + (2,)) for k in range(4)} for _ in range(2)]      # [-2] = prev, [-1] = now
    time_samples = rng.uniform(0, 1, M)
    div, res = reference_lines(rule, levels, time_samples, nu, dt)
    tau = {"TRAPEZOID": time_samples, "BACKWARD": 1.0, "FORWARD": 0.0}[rule]
    got = compose(combine(levels[-1]), combine(levels[-2]), tau, nu, dt, 1.0)
    assert np.abs(got[:, 0] - div).max() <= 1e-13 and np.abs(got[:, 1] - res).max() <= 1e-13


def test_compose_gives_the_right_hand_side_of_model_forward():
    """time_term = 0, dt = -1, no prev: column 1 is sample_pde of Model.forward (:655-659)."""
    rng = np.random.default_rng(4)
    M, nu = 29, 0.3
    o = {k: rng.normal(size=(M,) + (2,) * k + (2,)) for k in range(4)}
    sample_u, sample_uxx, sample_uxxx = o[0], o[2], o[3]
    sample_wx = sample_uxx[..., 0, 1] - sample_uxx[..., 1, 0]
    sample_wxx = sample_uxxx[..., 0, 1] - sample_uxxx[..., 1, 0]
    sample_pde = nu * (sample_wxx[:, 0, 0] + sample_wxx[:, 1, 1]) - (sample_u[:, 0] * sample_wx[:, 0] + sample_u[:, 1] * sample_wx[:, 1])
    got = compose(combine(o), None, 1.0, nu, -1.0, 0.0)
    assert np.abs(got[:, 1] - sample_pde).max() <= 1e-13


def test_column_names():
    import pigs_amd
    from pigs_amd import sampler
    assert pigs_amd.VORTICITY_RESIDUAL_COLUMNS == ("div", "r")
    assert pigs_amd.VORTICITY_RESIDUAL_COLUMNS is sampler.VORTICITY_RESIDUAL_COLUMNS
    assert callable(sampler.GaussianSampler.vorticity_residual)
    assert "vorticity_terms()" in sampler.GaussianSampler.vorticity_residual.__doc__


def test_lib_binds_both_symbols_with_the_documented_arguments(hip_lib):
    """forward: dtype, N, M, means, conics, values, samples, params, prev, out, aux, plan_ws, bytes, samples_ws, bytes,
    stream (16); backward: ... params, gout, aux, g_means, g_conics, g_values ... (18)."""
    from pigs_amd import _lib
    fwd, bwd = _lib.SIGNATURES["pigs_vorticity_residual_forward"], _lib.SIGNATURES["pigs_vorticity_residual_backward"]
    assert fwd[0] is ctypes.c_int and bwd[0] is ctypes.c_int
    assert len(fwd[1]) == 16 and len(bwd[1]) == 18
    for sig in (fwd[1], bwd[1]):
        assert sig[:3] == [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
        assert sig[-5:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        assert sig[7] is ctypes.POINTER(_lib.PigsVorticityResidual)
        assert all(a is ctypes.c_void_p for a in sig[3:7] + sig[8:-5])
    assert [n for n, _ in _lib.PigsVorticityResidual._fields_] == ["nu", "dt", "time_term", "tau", "tau_pt"]
    assert ctypes.sizeof(_lib.PigsVorticityResidual) == 40
    assert hip_lib.pigs_vorticity_residual_forward.argtypes == fwd[1]
    assert hip_lib.pigs_vorticity_residual_backward.argtypes == bwd[1]
    assert hip_lib.pigs_abi_version() == 10              # additive: no version bump


def test_argument_validation_needs_no_gpu(hip_lib):
    """Bad arguments are rejected before any HIP call (1 = invalid, 2 = unsupported)."""
    from pigs_amd import _lib
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below returns before a launch
    pz = ctypes.byref(_lib.PigsVorticityResidual(0.05, 0.01, 1.0, 1.0, None))
    f, b = hip_lib.pigs_vorticity_residual_forward, hip_lib.pigs_vorticity_residual_backward
    assert f(0, 4, 4, one, one, one, one, pz, null, null, null, null, 0, null, 0, null) == 1          # no output
    assert f(0, 4, 4, one, one, one, one, None, null, one, null, null, 0, null, 0, null) == 1         # no params
    assert f(0, 4, 4, null, one, one, one, pz, null, one, null, null, 0, null, 0, null) == 1          # no means
    assert f(7, 4, 4, one, one, one, one, pz, null, one, null, null, 0, null, 0, null) == 2           # dtype
    assert f(0, -1, 4, one, one, one, one, pz, null, one, null, null, 0, null, 0, null) == 1          # negative size
    assert f(1, 4, 4, one, one, one, one, pz, null, one, null, one, 64, one, 64, null) == 2           # binned float64
    assert b(0, 4, 4, one, one, one, one, pz, null, one, one, one, one, null, 0, null, 0, null) == 1      # no incoming gradient
    assert b(0, 4, 4, one, one, one, one, None, one, one, one, one, one, null, 0, null, 0, null) == 1     # no params
    assert b(0, 4, 4, one, one, one, one, pz, one, one, one, null, one, null, 0, null, 0, null) == 1      # no g_conics
    assert b(0, 4, 4, one, one, one, one, pz, one, null, one, one, one, null, 0, null, 0, null) == 1      # no aux
    assert b(7, 4, 4, one, one, one, one, pz, one, one, one, one, one, null, 0, null, 0, null) == 2       # dtype
    assert b(1, 4, 4, one, one, one, one, pz, one, one, one, one, one, one, 64, one, 64, null) == 2       # binned float64
