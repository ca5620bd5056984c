"""GPU: the stand-alone covariance builder (pigs_amd/covariances.py, csrc/covariances.hip) at its edges.  The MLP-free
drivers and the time step's un-fused route (after a refinement, and for the first state: tests/test_step_gpu.py) call
``build_covariances`` directly; tests/test_covariances.py holds it to one fixture, three extreme rows forward-only and
N = 0.  Here: N in {1, 255, 256, 257, 4 097}, float32 and float64, forward AND backward, against
oracle/covariances_numpy.py, on rows whose raw correlation t runs through {0, +-1e-4, +-3, +-6, +-9} and whose
variances span 1e-8 .. 1e2 with axis ratios up to 1e6.

Every element is held on its own, relative to its MAGNITUDE: for an output that is a product (the six forward entries)
the magnitude is the element itself; a gradient entry is a sum of up to four such products of either sign, and its
magnitude is the sum of their absolute values (no arithmetic of the dtype can add them closer than its rounding times
that sum, so an entry that is a small difference of large terms is not asked for more).
    float64     err <= 1e-12 magnitude                                    (the existing bar of tests/test_covariances.py)
    float32     err <= 4 err_torch32 + 1e-6 magnitude,                    err_torch32 the error, at the same element, of the
                reference's chain (tanh, prod, sqrt, a batched 2 x 2 inverse, the flat gather) in float32 torch ops on the
                GPU on the same rows; where that chain gives no finite number (tanh rounds to +-1 at |t| = 9 and the
                matrix is singular to it) its error counts as infinite and the element is held finite only.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import covariances_numpy as oracle

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 4097)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
T_VALUES = (0.0, 1e-4, -1e-4, 3.0, -3.0, 6.0, -6.0, 9.0, -9.0)
GOUTS = ("both", "covariances_only", "conics_only")


def make_rows(N, dtype, seed):
    """float64 arrays holding values of ``dtype``: s0 = 10^U(-8, 2), s1 = s0 x 10^U(-6, 6) folded back into [1e-8, 1e2],
    t cycling through T_VALUES (N = 1: the row of t = 9); the first nine rows take the corners: both variances at an end of the
    range, and the ratio 1e6 both ways"""
    rng = np.random.default_rng(seed)
    e0 = rng.uniform(-8.0, 2.0, N)
    e1 = e0 + rng.uniform(-6.0, 6.0, N)
    e1 = np.where(e1 > 2.0, e0 - (e1 - e0), np.where(e1 < -8.0, e0 - (e1 - e0), e1)).clip(-8.0, 2.0)
    corners = [(-8, -8), (2, 2), (-8, -2), (-4, 2), (2, -4), (-2, -8), (-8, -8), (2, 2), (0, 0)]
    for k, (a, b) in enumerate(corners[:N]):
        e0[k], e1[k] = a, b
    s = np.stack((10.0 ** e0, 10.0 ** e1), -1)
    t = np.array(T_VALUES)[(np.arange(N) + 7) % len(T_VALUES)][:, None]
    np_dtype = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    assert np.abs(e0 - e1).max() <= 6.0 + 1e-9
    return s.astype(np_dtype).astype(np.float64), t.astype(np_dtype).astype(np.float64)


def make_gouts(N, seed, which="both"):
    rng = np.random.default_rng(seed + 7919)
    g_cov, g_con = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    return (g_cov if which != "conics_only" else None), (g_con if which != "covariances_only" else None)


def gradient_magnitudes(s, t, g_cov, g_con):
    """the sums of the absolute values of the terms of oracle.build_covariances_backward, term by term"""
    gc = np.zeros((len(s), 3)) if g_cov is None else np.abs(g_cov)
    gq = np.zeros((len(s), 3)) if g_con is None else np.abs(g_con)
    s0, s1, tt = s[:, 0], s[:, 1], t[:, 0]
    h, r, k = np.abs(np.tanh(tt)), np.sqrt(s0 * s1), oracle.inverse_one_minus_tanh_squared(tt)
    m_s0 = gc[:, 0] + gc[:, 1] * h * r / (2 * s0) + gq[:, 0] * k / (s0 * s0) + gq[:, 1] * h * k / (2 * r * s0)
    m_s1 = gc[:, 2] + gc[:, 1] * h * r / (2 * s1) + gq[:, 2] * k / (s1 * s1) + gq[:, 1] * h * k / (2 * r * s1)
    m_h = gc[:, 1] * r + 2 * h * k * k * (gq[:, 0] / s0 + gq[:, 2] / s1) + gq[:, 1] * k * k * (1 + h * h) / r
    return np.stack((m_s0, m_s1), -1), (m_h / k)[:, None]


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().double().numpy()


def torch_chain(s, t):
    """the reference's lines in torch ops: tanh(t) sqrt(s0 s1) on both off-diagonals, the batched inverse, entries
    (xx, xy, yy).  inv_ex: a matrix that float32 sees as singular gives a non-finite row, not an exception"""
    tau = torch.tanh(t[:, 0]) * torch.sqrt(s[:, 0] * s[:, 1])
    full = torch.stack((s[:, 0], tau, tau, s[:, 1]), dim=-1).reshape(-1, 2, 2)
    inverse = torch.linalg.inv_ex(full).inverse

    def flat(m):
        return torch.stack((m[:, 0, 0], m[:, 0, 1], m[:, 1, 1]), dim=-1)
    return flat(full), flat(inverse)


def run(fn, s, t, g_cov, g_con, dtype):
    """(cov, conic, g_scaling, g_transform) of ``fn`` on the rows, as float64 numpy"""
    ts_, tt = dev(s, dtype).requires_grad_(True), dev(t, dtype).requires_grad_(True)
    cov, con = fn(ts_, tt)
    loss = sum((o * dev(g, dtype)).sum() for o, g in ((cov, g_cov), (con, g_con)) if g is not None)
    g_s, g_t = torch.autograd.grad(loss, (ts_, tt))
    assert g_t.shape == tt.shape
    return [host(x) for x in (cov, con, g_s, g_t)]


def reference(s, t, g_cov, g_con):
    cov, con = oracle.build_covariances(s, t)
    g_s, g_t = oracle.build_covariances_backward(s, t, g_cov, g_con)
    m_s, m_t = gradient_magnitudes(s, t, g_cov, g_con)
    return [cov, con, g_s, g_t], [np.abs(cov), np.abs(con), m_s, m_t]


NAMES = ("covariances", "conics", "d scaling", "d transform")


def hold(what, dtype, got, want, magnitudes, single=None):
    """the bar of the module text, element by element; returns the worst err / bound"""
    worst = 0.0
    for k, name in enumerate(NAMES):
        err = np.abs(got[k] - want[k])
        assert np.isfinite(got[k]).all(), f"{what} {name}: not finite"
        if dtype == torch.float64:
            bound = 1e-12 * magnitudes[k]
        else:
            err_t = np.abs(single[k] - want[k])
            bound = 4.0 * np.where(np.isfinite(err_t), err_t, np.inf) + 1e-6 * magnitudes[k]
        exact = (bound == 0) & (err == 0)                         # a zero the kernel also gives exactly (t = 0)
        ratio = np.where(exact, 0.0, err / np.where(bound == 0, 1e-300, bound))
        worst = max(worst, float(ratio.max()))
        i = np.unravel_index(ratio.argmax(), ratio.shape)
        assert ratio.max() <= 1.0, (f"{what} {name}{list(i)}: got {got[k][i]!r}, want {want[k][i]!r}, err {err[i]:.3g}, "
                                    f"bound {bound[i]:.3g}")
    return worst


@pytest.mark.parametrize("which", GOUTS)
@pytest.mark.parametrize("N", SIZES, ids=[f"N{n}" for n in SIZES])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_forward_and_backward_at_every_size(hip_lib, dtype, N, which):
    """the flat builder: forward and backward element by element; incoming gradients on both outputs and on one only (the
    other is absent: NULL at the C ABI)"""
    from pigs_amd import covariances
    dt = DTYPES[dtype]
    s, t = make_rows(N, dt, seed=N)
    g_cov, g_con = make_gouts(N, N, which)
    want, magnitudes = reference(s, t, g_cov, g_con)
    single = run(torch_chain, s, t, g_cov, g_con, dt) if dt == torch.float32 else None
    got = run(covariances.build_covariances, s, t, g_cov, g_con, dt)
    worst = hold(f"{dtype} N={N} {which}", dt, got, want, magnitudes, single)
    print(f"[figure] build_covariances {dtype} N={N} {which}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gradient_through_the_full_matrices(hip_lib, dtype):
    """build_full_covariances -> flatten_covariances, and a non-symmetric gradient on the full matrices themselves: the xy
    entry receives both off-diagonals"""
    from pigs_amd import covariances
    dt, N = DTYPES[dtype], 257
    s, t = make_rows(N, dt, seed=3)
    rng = np.random.default_rng(4)
    f_cov, f_con = rng.standard_normal((N, 2, 2)), rng.standard_normal((N, 2, 2))
    g_cov, g_con = make_gouts(N, 5)

    def folded(flat, full):
        return flat + np.stack((full[:, 0, 0], full[:, 0, 1] + full[:, 1, 0], full[:, 1, 1]), -1)
    want, magnitudes = reference(s, t, folded(g_cov, f_cov), folded(g_con, f_con))
    # the magnitudes of the folded gradient's own terms: |a| + |b| on the xy entry, not |a + b|
    _, magnitudes = reference(s, t, folded(np.abs(g_cov), np.abs(f_cov)), folded(np.abs(g_con), np.abs(f_con)))
    magnitudes[0], magnitudes[1] = np.abs(want[0]), np.abs(want[1])

    def through(build_full, flatten):
        def fn(ts_, tt):
            full_cov, full_con = build_full(ts_, tt)
            assert full_cov.shape == (N, 2, 2) and torch.equal(full_cov[:, 0, 1], full_cov[:, 1, 0])
            cov, con = flatten(full_cov, full_con)
            fn.extra = (full_cov * dev(f_cov, dt)).sum() + (full_con * dev(f_con, dt)).sum()
            return cov, con
        return fn

    def run_full(fn):
        ts_, tt = dev(s, dt).requires_grad_(True), dev(t, dt).requires_grad_(True)
        cov, con = fn(ts_, tt)
        loss = (cov * dev(g_cov, dt)).sum() + (con * dev(g_con, dt)).sum() + fn.extra
        return [host(x) for x in (cov, con) + torch.autograd.grad(loss, (ts_, tt))]

    def torch_full(ts_, tt):
        tau = torch.tanh(tt[:, 0]) * torch.sqrt(ts_[:, 0] * ts_[:, 1])
        full = torch.stack((ts_[:, 0], tau, tau, ts_[:, 1]), dim=-1).reshape(-1, 2, 2)
        return full, torch.linalg.inv_ex(full).inverse
    got = run_full(through(covariances.build_full_covariances, covariances.flatten_covariances))
    single = run_full(through(torch_full, covariances.flatten_covariances)) if dt == torch.float32 else None
    worst = hold(f"{dtype} full matrices", dt, got, want, magnitudes, single)
    print(f"[figure] build_full_covariances + flatten_covariances {dtype}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("N", [255, 257])
def test_canaries_behind_every_output(hip_lib, N, dtype):
    """through the C ABI with buffers of its own: 64 sentinel elements behind the covariances, the conics and both
    gradients; a NULL output is not written and the other one is"""
    dt, pad, sentinel = DTYPES[dtype], 64, -12345.0
    code = {torch.float32: 0, torch.float64: 1}[dt]
    s, t = make_rows(N, dt, seed=N + 1)
    g_cov, g_con = make_gouts(N, N + 1)
    ts_, tt, gc, gq = dev(s, dt), dev(t[:, 0], dt), dev(g_cov, dt), dev(g_con, dt)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def padded(n):
        return torch.full((n + pad,), sentinel, dtype=dt, device="cuda")

    def ptr(x):
        return ctypes.c_void_p(x.data_ptr()) if x is not None else None
    cov, con, con_alone, g_s, g_t = padded(3 * N), padded(3 * N), padded(3 * N), padded(2 * N), padded(N)
    assert hip_lib.pigs_build_covariances(code, N, ptr(ts_), ptr(tt), ptr(cov), ptr(con), stream) == 0
    assert hip_lib.pigs_build_covariances(code, N, ptr(ts_), ptr(tt), None, ptr(con_alone), stream) == 0
    assert hip_lib.pigs_build_covariances_backward(code, N, ptr(ts_), ptr(tt), ptr(gc), ptr(gq), ptr(g_s), ptr(g_t), stream) == 0
    torch.cuda.synchronize()
    for name, x in (("covariances", cov), ("conics", con), ("conics alone", con_alone), ("d scaling", g_s), ("d transform", g_t)):
        assert (x[-pad:] == sentinel).all(), f"{name}: written past its end"
        assert not (x[:-pad] == sentinel).any(), f"{name}: not all of it was written"
    assert torch.equal(con, con_alone)
    want, magnitudes = reference(s, t, g_cov, g_con)
    got = [host(cov[:-pad]).reshape(N, 3), host(con[:-pad]).reshape(N, 3), host(g_s[:-pad]).reshape(N, 2), host(g_t[:-pad]).reshape(N, 1)]
    tol = 1e-12 if dt == torch.float64 else 1e-5
    for name, g, w, m in zip(NAMES, got, want, magnitudes):
        assert (np.abs(g - w) <= tol * m).all(), name


def test_capture_and_a_replay_on_rewritten_inputs(hip_lib):
    """torch.cuda.graph around the builder and its backward; the replay runs on rows and gradients written in place"""
    from pigs_amd import covariances
    dt, N = torch.float64, 257
    cases = [(make_rows(N, dt, seed=20 + k), make_gouts(N, 30 + k)) for k in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (s, t), (g_cov, g_con) = cases[0]
        leaves = [dev(s, dt).requires_grad_(True), dev(t, dt).requires_grad_(True)]
        static_g = [dev(g_cov, dt), dev(g_con, dt)]

        def step():
            cov, con = covariances.build_covariances(*leaves)
            return (cov, con) + torch.autograd.grad((cov * static_g[0]).sum() + (con * static_g[1]).sum(), leaves)
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    torch.cuda.current_stream().wait_stream(side)
    (s, t), (g_cov, g_con) = cases[1]
    with torch.no_grad():
        for dst, a in zip(leaves + static_g, (s, t, g_cov, g_con)):
            dst.copy_(dev(a, dt))
    graph.replay()
    torch.cuda.synchronize()
    want, magnitudes = reference(s, t, g_cov, g_con)
    hold("replay", dt, [host(o) for o in outs], want, magnitudes)
