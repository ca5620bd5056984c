"""CPU: the surface of GaussianSampler.vorticity_terms() that needs no GPU -- the two C ABI symbols and their ctypes
signatures, the exported column names -- and the two numpy helpers that the GPU tests (tests/test_vorticity_gpu.py) take
their expectations from:

  combine(o)   the seven columns from the oracle's outputs of orders 0..3, written with the reference's own index
               expressions (model_pn.py:848, :779, :655 / :780, :656 / :781 / :630)
  expand(g)    the four full-layout gradient arrays that a gradient g [M, 7] of those columns induces

``expand`` must be the adjoint of ``combine``; the dot-product test below pins that, so the expected outputs and the
expected gradients of the GPU tests cannot drift apart."""
import ctypes

import numpy as np


def combine(o):
    """{order: array} of a two-channel field in two dimensions (o[0] [M, 2], o[1] [M, 2, 2], o[2] [M, 2, 2, 2],
    o[3] [M, 2, 2, 2, 2]; last index: the channel) -> [M, 7] = (u_x, u_y, div, w, w_x, w_y, lap_w)."""
    u, ux, uxx, uxxx = o[0], o[1], o[2], o[3]
    div = ux[:, 0, 0] + ux[:, 1, 1]
    w = ux[:, 0, 1] - ux[:, 1, 0]
    wx = uxx[..., 0, 1] - uxx[..., 1, 0]            # [M, 2]
    wxx = uxxx[..., 0, 1] - uxxx[..., 1, 0]         # [M, 2, 2]
    lap_w = wxx[:, 0, 0] + wxx[:, 1, 1]
    return np.stack((u[:, 0], u[:, 1], div, w, wx[:, 0], wx[:, 1], lap_w), -1)


def expand(g):
    """The gradients {order: array} (full layouts) that arrive at orders 0..3 when g [M, 7] arrives at combine()."""
    g = np.asarray(g, dtype=np.float64)
    M = g.shape[0]
    g0 = g[:, 0:2].copy()
    g1 = np.zeros((M, 2, 2))
    g1[:, 0, 0] += g[:, 2]
    g1[:, 1, 1] += g[:, 2]
    g1[:, 0, 1] += g[:, 3]
    g1[:, 1, 0] -= g[:, 3]
    g2 = np.zeros((M, 2, 2, 2))
    g2[:, :, 0, 1] += g[:, 4:6]
    g2[:, :, 1, 0] -= g[:, 4:6]
    g3 = np.zeros((M, 2, 2, 2, 2))
    for i in range(2):
        g3[:, i, i, 0, 1] += g[:, 6]
        g3[:, i, i, 1, 0] -= g[:, 6]
    return {0: g0, 1: g1, 2: g2, 3: g3}


def column_scales(o):
    """Per column, the largest magnitude among the oracle entries that enter it (the columns are differences: a bar
    relative to the difference itself would be a cancellation test; tests/test_residual_terms_gpu.py term_scale)."""
    s = [np.abs(o[k]).max() for k in range(4)]
    return np.array([s[0], s[0], s[1], s[1], s[2], s[2], s[3]])


def test_expand_is_the_adjoint_of_combine():
    rng = np.random.default_rng(0)
    M = 37
    o = {k: rng.normal(size=(M,) + (2,) * k + (2,)) for k in range(4)}
    g = rng.normal(size=(M, 7))
    lhs = (combine(o) * g).sum()
    e = expand(g)
    rhs = sum((o[k] * e[k]).sum() for k in range(4))
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), 1.0), (lhs, rhs)
    # and column by column, so that no two columns can trade places
    for k in range(7):
        gk = np.zeros((M, 7))
        gk[:, k] = g[:, k]
        ek = expand(gk)
        lk, rk = (combine(o)[:, k] * g[:, k]).sum(), sum((o[j] * ek[j]).sum() for j in range(4))
        assert abs(lk - rk) <= 1e-13 * max(abs(lk), 1.0), (k, lk, rk)


def test_combine_on_a_field_with_known_derivatives():
    """u = (sin(a x) cos(b y), x^3 y + y^2): div, w, grad w and lap w by hand."""
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1, 1, 50), rng.uniform(-1, 1, 50)
    a, b = 1.3, 0.7
    M = len(x)
    o = {0: np.zeros((M, 2)), 1: np.zeros((M, 2, 2)), 2: np.zeros((M, 2, 2, 2)), 3: np.zeros((M, 2, 2, 2, 2))}
    s, c_, sy, cy = np.sin(a * x), np.cos(a * x), np.sin(b * y), np.cos(b * y)
    # channel 0: f = sin(a x) cos(b y)
    o[0][:, 0] = s * cy
    d1 = {(0,): a * c_ * cy, (1,): -b * s * sy}
    d2 = {(0, 0): -a * a * s * cy, (0, 1): -a * b * c_ * sy, (1, 1): -b * b * s * cy}
    d3 = {(0, 0, 0): -a ** 3 * c_ * cy, (0, 0, 1): a * a * b * s * sy, (0, 1, 1): -a * b * b * c_ * cy, (1, 1, 1): b ** 3 * s * sy}
    # channel 1: h = x^3 y + y^2
    o[0][:, 1] = x ** 3 * y + y ** 2
    e1 = {(0,): 3 * x * x * y, (1,): x ** 3 + 2 * y}
    e2 = {(0, 0): 6 * x * y, (0, 1): 3 * x * x, (1, 1): 2 + 0 * x}
    e3 = {(0, 0, 0): 6 * y, (0, 0, 1): 6 * x, (0, 1, 1): 0 * x, (1, 1, 1): 0 * x}
    for ch, (t1, t2, t3) in enumerate(((d1, d2, d3), (e1, e2, e3))):
        for i in range(2):
            o[1][:, i, ch] = t1[(i,)]
            for j in range(2):
                o[2][:, i, j, ch] = t2[tuple(sorted((i, j)))]
                for k in range(2):
                    o[3][:, i, j, k, ch] = t3[tuple(sorted((i, j, k)))]
    got = combine(o)
    div = d1[(0,)] + e1[(1,)]
    w = e1[(0,)] - d1[(1,)]                     # d_x u_y - d_y u_x
    w_x = e2[(0, 0)] - d2[(0, 1)]
    w_y = e2[(0, 1)] - d2[(1, 1)]
    lap_w = (e3[(0, 0, 0)] + e3[(0, 1, 1)]) - (d3[(0, 0, 1)] + d3[(1, 1, 1)])
    want = np.stack((o[0][:, 0], o[0][:, 1], div, w, w_x, w_y, lap_w), -1)
    assert np.abs(got - want).max() < 1e-13


def test_column_names():
    import pigs_amd
    from pigs_amd import sampler
    assert pigs_amd.VORTICITY_COLUMNS == ("u_x", "u_y", "div", "w", "w_x", "w_y", "lap_w")
    assert len(pigs_amd.VORTICITY_COLUMNS) == 7 and pigs_amd.VORTICITY_COLUMNS is sampler.VORTICITY_COLUMNS
    assert callable(sampler.GaussianSampler.vorticity_terms)
    assert "unbind(1)" in sampler.GaussianSampler.vorticity_terms.__doc__


def test_lib_binds_both_symbols_with_the_documented_arguments(hip_lib):
    """forward: dtype, N, M, means, conics, values, samples, out, plan_ws, bytes, samples_ws, bytes, stream (13);
    backward: ... gout, g_means, g_conics, g_values ... (16)."""
    from pigs_amd import _lib
    fwd, bwd = _lib.SIGNATURES["pigs_vorticity_forward"], _lib.SIGNATURES["pigs_vorticity_backward"]
    assert fwd[0] is ctypes.c_int and bwd[0] is ctypes.c_int
    assert len(fwd[1]) == 13 and len(bwd[1]) == 16
    for sig in (fwd[1], bwd[1]):
        assert sig[:3] == [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
        assert sig[-5:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        assert all(a is ctypes.c_void_p for a in sig[3:-5])
    assert hip_lib.pigs_vorticity_forward.argtypes == fwd[1] and hip_lib.pigs_vorticity_backward.argtypes == bwd[1]
    assert hip_lib.pigs_abi_version() == 10              # additive: no version bump


def test_argument_validation_needs_no_gpu(hip_lib):
    """Bad arguments are rejected before any HIP call (1 = invalid, 2 = unsupported)."""
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below returns before a launch
    f, b = hip_lib.pigs_vorticity_forward, hip_lib.pigs_vorticity_backward
    assert f(0, 4, 4, one, one, one, one, null, null, 0, null, 0, null) == 1          # no output
    assert f(0, 4, 4, null, one, one, one, one, null, 0, null, 0, null) == 1          # no means
    assert f(7, 4, 4, one, one, one, one, one, null, 0, null, 0, null) == 2           # dtype
    assert f(0, -1, 4, one, one, one, one, one, null, 0, null, 0, null) == 1          # negative size
    assert f(1, 4, 4, one, one, one, one, one, one, 64, one, 64, null) == 2           # binned float64
    assert b(0, 4, 4, one, one, one, one, null, one, one, one, null, 0, null, 0, null) == 1      # no incoming gradient
    assert b(0, 4, 4, one, one, one, one, one, one, null, one, null, 0, null, 0, null) == 1      # no g_conics
    assert b(1, 4, 4, one, one, one, one, one, one, one, one, one, 64, one, 64, null) == 2       # binned float64
