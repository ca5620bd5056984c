"""GPU: the input transform (pigs_amd/input_transform.py, csrc/input_transform.hip) against the float64 oracle of
tests/test_input_transform.py.

The bar is the project's, from tests/test_mlp_gpu.py: for latent, the packed matrices, t_params and every gradient

    err_hip <= 4 err_torch32 + 1e-6 scale,      both errors against the float64 oracle,

err_torch32 that of the oracle run in float32 torch ops on the GPU on the same tensors, scale the tensor's largest
magnitude in float64.  Each case prints its worst err_hip / (4 err_torch32 + 1e-6 scale).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_input_transform as ti
from test_input_transform import KEYS, RESULTS, load_fixture, make_case, oracle_all, scale_of, shapes, sizes

pytestmark = pytest.mark.gpu

# the tile edge (16 rows), the workgroup edge (64), the model's size, and 4 097 = 257 tiles: one more than the 256 waves
# of the capped grids, so that the grid-stride loops of the three reducing kernels run
SIZES = (1, 15, 16, 17, 63, 64, 65, 1600, 4097)
CASES = [(c, p, N) for c, p in ((1, 1), (2, 1), (2, 2)) for N in SIZES]
CASES += [(c, p, N) for c, p in ((3, 3), (4, 4), (4, 1)) for N in (17, 1600)]
CASES += [(3, 3, 16 * 257)]                    # 257 full tiles: the last wave's second tile is a whole one
CASES += [(2, 1, 16 * 2048 + 1)]               # 2 049 tiles: one more than the latent forward's own cap of 2 048 waves


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def leaves(rows, params, row_grad=True, param_grad=True):
    trows = [dev(a).requires_grad_(row_grad and k < 3) for k, a in enumerate(rows)]
    tparams = [dev(a).requires_grad_(param_grad) for a in params]
    return trows, tparams


def hip_forward(trows, tparams):
    import pigs_amd
    matrices, latent = pigs_amd.transform_matrices(*trows, tparams, return_latent=True)
    return latent, matrices, pigs_amd.apply_transforms(matrices, *trows[1:])[0]


def hip_all(rows, params, w):
    trows, tparams = leaves(rows, params)
    latent, matrices, t_params = hip_forward(trows, tparams)
    grads = torch.autograd.grad(t_params, trows[:3] + tparams, dev(w))
    return dict(zip(RESULTS, [latent.detach(), matrices.detach(), t_params.detach()] + list(grads)))


def hold(what, got, ref32, want, names=RESULTS):
    """the bar of the module text over ``names``; returns the worst err_hip / allowance"""
    worst, bad = 0.0, []
    for k in names:
        g = host(got[k]).reshape(want[k].shape) if host(got[k]).size == want[k].size else host(got[k])
        assert g.shape == want[k].shape, (what, k, g.shape, want[k].shape)
        scale = scale_of(want[k])
        err_h, err_t = np.abs(g - want[k]).max(), np.abs(ref32[k] - want[k]).max()
        bound = 4.0 * err_t + 1e-6 * scale
        worst = max(worst, err_h / bound)
        if not err_h <= bound:
            bad.append(f"{k}: hip {err_h:.3g}, torch32 {err_t:.3g}, scale {scale:.3g}")
    print(f"[figure] {what}: worst err_hip / (4 err_torch32 + 1e-6 scale) = {worst:.3f}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return worst


_reference = {}


def reference(key):
    """the case's tensors, the float64 oracle's results and the float32 torch results on the GPU: computed once, shared,
    never changed.  ``key``: a fixture's name or (c, p, N)"""
    if key not in _reference:
        if isinstance(key, str):
            rows, params, w, _ = load_fixture(key)
            rows, params, w = [ti_round(a) for a in rows], [ti_round(a) for a in params], ti_round(w)
        else:
            c, p, N = key
            rows, params, w = make_case(c, p, N, seed=10000 * c + 1000 * p + N)
        _reference[key] = (rows, params, w, oracle_all(rows, params, w),
                           oracle_all(rows, params, w, dtype=torch.float32, device="cuda"))
    return _reference[key]


def ti_round(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- accuracy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diffusion", "navier_stokes"])
def test_the_recorded_steps(hip_lib, name):
    rows, params, w, want, ref32 = reference(name)
    hold(name, hip_all(rows, params, w), ref32, want)


@pytest.mark.parametrize("c,p,N", CASES, ids=[f"c{c}p{p}N{N}" for c, p, N in CASES])
def test_every_shape_at_every_size(hip_lib, c, p, N):
    """seeded weights and rows with biases of order 1: a dead row of the last tile, counted, would move the mean by
    tanh(bias chain) x (dead rows / N)"""
    rows, params, w, want, ref32 = reference((c, p, N))
    hold(f"c={c} p={p} N={N}", hip_all(rows, params, w), ref32, want)


# ---- exactness ----------------------------------------------------------------------------------------------
def integer_matrices(c, p):
    """non-symmetric small-integer I + B_j, packed"""
    out = []
    for j, k in enumerate(sizes(c, p)):
        i, m = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
        out.append((np.eye(k) + (2 * i - m + (i * m + j) % 3 - 1)).astype(np.float64))
    return out


@pytest.mark.parametrize("N", [16, 37, 4097])
@pytest.mark.parametrize("c,p", [(2, 1), (3, 2), (4, 4)])
def test_small_integers_are_exact(hip_lib, c, p, N):
    """the last layer of every TransformNet has zero weights and integer biases, the rows and the incoming gradient are
    small integers: t_params, g_Sigma, g_u and the five dT (read through the ABI) are bit-equal to the integer results.
    The matrices are not symmetric and differ from block to block: no transposition or swapped block passes."""
    from pigs_amd import _lib
    import pigs_amd
    rng = np.random.default_rng(N + 10 * c + p)
    rows, params, _ = make_case(c, p, N, seed=N)
    rows = [rng.integers(-4, 5, a.shape).astype(np.float64) for a in rows]
    T = integer_matrices(c, p)
    for j, t in enumerate(T):
        params[6 * (j + 1) + 4] = np.zeros_like(params[6 * (j + 1) + 4])
        params[6 * (j + 1) + 5] = (t - np.eye(t.shape[0])).ravel()
    trows, tparams = leaves(rows, params, False, False)
    _, matrices, t_params = hip_forward(trows, tparams)
    packed = np.concatenate([t.ravel() for t in T])
    assert np.array_equal(host(matrices), packed)
    cov, u, bnd, su, ux, uxx, pde = rows[1:]
    sigma = cov.reshape(N, 2, 2)
    want = np.concatenate([(T[0] @ sigma).reshape(N, 4), u @ T[1].T, bnd, su @ T[1].T, ux @ T[2].T, uxx @ T[3].T, pde @ T[4].T], 1)
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(host(t_params), want)

    g = rng.integers(-3, 4, want.shape).astype(np.float64)
    edges = np.cumsum([0, 4, c, 1, c, 2 * c, 2 * c, p])
    gs = [g[:, a:b] for a, b in zip(edges[:-1], edges[1:])]
    want_cov = (T[0].T @ gs[0].reshape(N, 2, 2)).reshape(N, 4)
    want_u = gs[1] @ T[1]
    want_dT = np.concatenate([np.einsum("nij,nkj->ik", gs[0].reshape(N, 2, 2), sigma).ravel(), (gs[1].T @ u + gs[3].T @ su).ravel(),
                              (gs[4].T @ ux).ravel(), (gs[5].T @ uxx).ravel(), (gs[6].T @ pde).ravel()])
    assert np.abs(want_dT).max() < 2 ** 24
    lib = hip_lib
    nbytes = lib.pigs_input_transform_scratch_bytes(N, c, p)
    scratch = torch.empty(nbytes // 4, device="cuda")
    g_cov, g_u, g_m, tg = torch.empty(N, 4, device="cuda"), torch.empty(N, c, device="cuda"), torch.empty_like(matrices), dev(g)
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in (matrices, trows[1], trows[2], trows[4], trows[5], trows[6], trows[7], tg)]
    rc = lib.pigs_input_transform_apply_backward(_lib.PIGS_F32, N, c, p, *ptr, scratch.data_ptr(), nbytes, g_cov.data_ptr(),
                                                 g_u.data_ptr(), g_m.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(g_cov), want_cov) and np.array_equal(host(g_u), want_u)
    assert np.array_equal(host(g_m), want_dT)
    assert pigs_amd.input_transform.matrix_floats(c, p) == want_dT.size


# ---- memory -------------------------------------------------------------------------------------------------
CANARY = 12345.0


def guarded(a, pad=64, fill=float("nan")):
    """(the tensor holding ``a``, its whole buffer): ``pad`` floats of ``fill`` behind the data"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((a.size + pad,), fill, dtype=torch.float32, device="cuda")
    buf[:a.size] = torch.as_tensor(a.ravel()).cuda()
    return buf[:a.size].view(a.shape), buf


def intact(buf, size):
    return bool((buf[size:] == CANARY).all())


@pytest.mark.parametrize("c,p,N", [(2, 1, 37), (4, 4, 17), (1, 1, 4097)])
def test_nothing_is_read_or_written_past_the_arrays(hip_lib, c, p, N):
    """through the C ABI, N no multiple of 16: NaN behind every input (a read past the end would reach a result),
    canaries behind every output, every gradient and the scratch; the results are those of the Python path, bit for bit"""
    from pigs_amd import _lib
    lib = hip_lib
    rows, params, w, _, _ = reference((c, p, N)) if (c, p, N) in CASES else (*make_case(c, p, N, seed=7), None, None)
    want = hip_all(rows, params, w)
    g_rows = [guarded(a) for a in rows]
    g_params = [guarded(a) for a in params]
    PM, D = 4 + 9 * c * c + p * p, 5 + 6 * c + p
    nbytes = lib.pigs_input_transform_scratch_bytes(N, c, p)

    def out(*shape):
        return guarded(np.zeros(shape), fill=CANARY)
    latent, matrices, t_params, scratch = out(16), out(PM), out(N, D), out(nbytes // 4)
    g_m, g_cov, g_u = out(PM), out(N, 4), out(N, c)
    g_means, g_cov2, g_u2 = out(N, 2), out(N, 4), out(N, c)
    grads = [out(*a.shape) for a in params]
    g_t = guarded(w)
    rp = [t.data_ptr() for t, _ in g_rows]
    pp = (ctypes.c_void_p * 36)(*[t.data_ptr() for t, _ in g_params])
    gp = (ctypes.c_void_p * 36)(*[t.data_ptr() for t, _ in grads])
    F = _lib.PIGS_F32
    rc = lib.pigs_input_transform_matrices_forward(F, N, c, p, *rp, pp, scratch[0].data_ptr(), nbytes, latent[0].data_ptr(),
                                                   matrices[0].data_ptr(), None)
    assert rc == 0
    rc = lib.pigs_input_transform_apply_forward(F, N, c, p, matrices[0].data_ptr(), *rp[1:], t_params[0].data_ptr(), None)
    assert rc == 0
    rc = lib.pigs_input_transform_apply_backward(F, N, c, p, matrices[0].data_ptr(), rp[1], rp[2], *rp[4:], g_t[0].data_ptr(),
                                                 scratch[0].data_ptr(), nbytes, g_cov[0].data_ptr(), g_u[0].data_ptr(),
                                                 g_m[0].data_ptr(), None)
    assert rc == 0
    rc = lib.pigs_input_transform_matrices_backward(F, N, c, p, *rp, pp, latent[0].data_ptr(), g_m[0].data_ptr(),
                                                    scratch[0].data_ptr(), nbytes, g_means[0].data_ptr(), g_cov2[0].data_ptr(),
                                                    g_u2[0].data_ptr(), gp, None)
    assert rc == 0
    torch.cuda.synchronize()
    for name, (t, buf) in (("latent", latent), ("matrices", matrices), ("t_params", t_params), ("scratch", scratch),
                           ("g_matrices", g_m), ("g_cov", g_cov), ("g_u", g_u), ("g_means", g_means), ("g_cov2", g_cov2),
                           ("g_u2", g_u2)) + tuple((f"g_{k}", v) for k, v in zip(KEYS, grads)):
        assert intact(buf, t.numel()), f"{name}: written past its end"
        if name != "scratch":
            assert bool(torch.isfinite(t).all()), f"{name}: something past an input's end was read"
    assert torch.equal(latent[0], want["latent"]) and torch.equal(matrices[0], want["matrices"])
    assert torch.equal(t_params[0], want["t_params"]) and torch.equal(g_means[0], want["g_means"])
    assert torch.equal(g_cov[0] + g_cov2[0], want["g_full_covariances"]) and torch.equal(g_u[0] + g_u2[0], want["g_u"])
    for k, (t, _) in zip(KEYS, grads):
        assert torch.equal(t, want["g_" + k].reshape(t.shape)), k


# ---- determinism, the gradient patterns, strides ------------------------------------------------------------
def test_three_calls_give_the_same_bits(hip_lib):
    rows, params, w, _, _ = reference((2, 2, 4097))
    first = hip_all(rows, params, w)
    for _ in range(2):
        again = hip_all(rows, params, w)
        for k in RESULTS:
            assert torch.equal(first[k], again[k]), f"{k} differs between two calls on the same inputs"


PATTERNS = {
    "inputs_only": lambda k: k < 3,
    "parameters_only": lambda k: k >= 3,
    "one_net_frozen": lambda k: not 3 + 12 <= k < 3 + 18,          # transform_u_net
    "latent_net_frozen": lambda k: not 3 <= k < 3 + 6,
    "means_alone": lambda k: k == 0,
    "u_and_last_net": lambda k: k == 2 or k >= 3 + 30,
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_every_needs_input_grad_pattern_gives_the_bits_of_the_full_backward(hip_lib, pattern):
    rows, params, w, _, _ = reference((2, 1, 65))
    full = hip_all(rows, params, w)
    trows, tparams = leaves(rows, params, False, False)
    asked = [(name, t) for k, (name, t) in enumerate(zip(RESULTS[3:], trows[:3] + tparams)) if PATTERNS[pattern](k)]
    for _, t in asked:
        t.requires_grad_(True)
    _, _, t_params = hip_forward(trows, tparams)
    grads = torch.autograd.grad(t_params, [t for _, t in asked], dev(w))
    assert 0 < len(asked) < 39
    for (name, _), g in zip(asked, grads):
        assert torch.equal(g, full[name]), f"{pattern}: {name} differs from the full backward"


def test_a_strided_incoming_gradient(hip_lib):
    rows, params, w, _, _ = reference((2, 1, 65))
    full = hip_all(rows, params, w)
    trows, tparams = leaves(rows, params)
    _, _, t_params = hip_forward(trows, tparams)
    wide = torch.zeros(w.shape[0], 2 * w.shape[1], device="cuda")
    wide[:, ::2] = dev(w)
    g = wide[:, ::2]
    assert not g.is_contiguous()
    grads = torch.autograd.grad(t_params, trows[:3] + tparams, g)
    for name, got in zip(RESULTS[3:], grads):
        assert torch.equal(got, full[name]), name


def module_of(params, c, p):
    """the stand-in of the reference's module (tests/test_input_transform.py) on the GPU, holding ``params``"""
    module = ti.reference_like(c, p).cuda()
    named = dict(module.named_parameters())
    with torch.no_grad():
        for k, a in zip(KEYS, params):
            named[k].copy_(dev(a).reshape(named[k].shape))
    return module


def test_transform_gaussians_applies_the_same_matrices_to_new_rows(hip_lib):
    """the split path: 33 new rows under the matrices of the forward; the matrices' gradient is the sum of both uses"""
    import pigs_amd
    c, p, N, n = 2, 1, 65, 33
    rows, params, w, _, _ = reference((c, p, N))
    new_rows, _, new_w = make_case(c, p, n, seed=99)
    new_rows[3] = np.zeros_like(new_rows[3])               # model_pn.py:282

    def chain(dtype, device):
        def leaf(a, grad=False):
            return torch.as_tensor(a, dtype=dtype, device=device).requires_grad_(grad)
        trows = [leaf(a, k < 3) for k, a in enumerate(rows)]
        tnew = [leaf(a, k in (1, 2)) for k, a in enumerate(new_rows)]
        tparams = [leaf(a, True) for a in params]
        _, matrices, t = ti.oracle(trows, tparams)
        T = [matrices[o:o + k * k].reshape(k, k) for o, k in pigs_amd.input_transform.matrix_blocks(c, p)]
        more = torch.cat([(T[0] @ tnew[1].reshape(n, 2, 2)).reshape(n, 4), tnew[2] @ T[1].T, tnew[3], tnew[4] @ T[1].T,
                          tnew[5] @ T[2].T, tnew[6] @ T[3].T, tnew[7] @ T[4].T], dim=1)
        wrt = trows[:3] + tnew[1:3] + tparams
        grads = torch.autograd.grad((leaf(w) * t).sum() + (leaf(new_w) * more).sum(), wrt)
        return [host(more)] + [host(g) for g in grads]
    want, ref32 = chain(torch.float64, "cpu"), chain(torch.float32, "cuda")

    module = module_of(params, c, p)
    net = pigs_amd.FusedInputTransform.from_module(module)
    trows = [dev(a).requires_grad_(k < 3) for k, a in enumerate(rows)]
    tnew = [dev(a).requires_grad_(k in (1, 2)) for k, a in enumerate(new_rows)]
    t = net(*trows)
    more = net.transform_gaussians(tnew[1], tnew[2], *tnew[4:])
    assert t.shape == (1, N, 5 + 6 * c + p) and more.shape == (1, n, 5 + 6 * c + p)
    grads = torch.autograd.grad((dev(w) * t[0]).sum() + (dev(new_w) * more[0]).sum(), trows[:3] + tnew[1:3] + net.params())
    got = [more[0]] + list(grads)
    names = ["new t_params", "g_means", "g_full_covariances", "g_u", "g_new_full_covariances", "g_new_u"] + ["g_" + k for k in KEYS]
    hold("transform_gaussians, 65 + 33 rows", dict(zip(names, got)), dict(zip(names, ref32)), dict(zip(names, want)), names)


# ---- capture ------------------------------------------------------------------------------------------------
def test_forward_and_backward_in_one_graphed_step(hip_lib):
    """GraphedStep over FusedInputTransform and autograd.grad: three replays on rewritten rows and weights, each bit-equal
    to the eager call on the same values"""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    c, p, N = 2, 1, 1600
    cases = [make_case(c, p, N, seed=40 + k) for k in range(4)]
    net = pigs_amd.FusedInputTransform.from_module(module_of(cases[0][1], c, p))

    def run(trows, w):
        t = net(*trows)
        return (t,) + torch.autograd.grad(t[0], list(trows[:3]) + net.params(), w)

    def make_inputs():
        rows, _, w = cases[0]
        return tuple(dev(a).requires_grad_(k < 3) for k, a in enumerate(rows)) + (dev(w),)
    step = GraphedStep(lambda *x: run(x[:8], x[8]), make_inputs, warmup=2)
    for k in (1, 2, 3):
        rows, params, w = cases[k]
        rewritten = {KEYS[i]: params[i] for i in (0, 5, 16, 35)}
        named = dict(net.named_parameters())
        with torch.no_grad():
            for leaf, a in zip(step.inputs, rows + [w]):
                leaf.copy_(dev(a))
            for key, a in rewritten.items():
                named[key].copy_(dev(a).reshape(named[key].shape))
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        eager = run([dev(a).requires_grad_(i < 3) for i, a in enumerate(rows)], dev(w))
        assert len(got) == len(eager) == 1 + 3 + 36
        for i, (a, b) in enumerate(zip(got, eager)):
            assert torch.equal(a, b), f"replay {k}: output {i} differs from the eager call"
        assert not torch.equal(got[0], eager[0] * 0)


# ---- the seam -----------------------------------------------------------------------------------------------
def test_input_transform_into_the_hip_step_and_the_loss(hip_lib):
    """FusedInputTransform -> the HIP step of tests/test_step_gpu.py -> the loss on the Navier-Stokes fixture, against the
    float64 oracle of the same chain: t_params, every intermediate, and the gradient of every parameter --
    ``input_transform.*`` included -- under that file's own allowance (floor 1e-6 upstream of the sampler, 1e-5 for the
    gradients)"""
    import pigs_amd
    import test_step as ts
    from test_step_gpu import HipOps, hold as hold_step

    scene = ts.all_scenes()["navier_stokes"]
    rows, params, _, _ = load_fixture("navier_stokes")
    consts, params = [ti_round(a) for a in rows[3:]], [ti_round(a) for a in params]
    c, p = rows[2].shape[1], rows[7].shape[1]

    class WithTransform:
        """a scene's operations with t_params made from the state in front of every step"""

        def __init__(self, inner, dtype, device):
            self.inner = inner
            self.consts = [torch.as_tensor(a, dtype=dtype, device=device) for a in consts]
            self.refine, self.sample = inner.refine, inner.sample

        def step(self, net, t_params, means, u, scaling, transforms, mask, wrap, k, covs=None):
            flat = ts.flat_covariances(scaling, transforms)[0]
            full = torch.stack((flat[:, 0], flat[:, 1], flat[:, 1], flat[:, 2]), dim=-1)
            t = net.input_transform(means, full, u, *self.consts)
            return dict(self.inner.step(net, t, means, u, scaling, transforms, mask, wrap, k, covs), t_params=t)

    class Net(ts.Network):
        def __init__(self, dtype, device, fused):
            super().__init__(scene.sd, dtype, device)
            if fused:
                self.fuse(pigs_amd.FusedMLP.from_sequential)
                module = pigs_amd.FusedInputTransform.from_module(module_of(params, c, p))
                self.it_params = module.params()
                self.input_transform = lambda *r: module(*r)[0]
            else:
                self.it_params = [torch.tensor(a, dtype=dtype, device=device, requires_grad=True) for a in params]
                self.input_transform = lambda *r: ti.oracle(list(r), self.it_params)[2]

        def named_parameters(self):
            return super().named_parameters() + [("input_transform." + k, t) for k, t in zip(KEYS, self.it_params)]

    want = ts.run_scene(scene, WithTransform(ts.OracleOps(), torch.float64, "cpu"), Net(torch.float64, "cpu", False))
    full = host(want["s0/t_params"])
    recorded = ts.load_fixture("navier_stokes")["t_params"]
    assert np.abs(full - recorded).max() <= 1e-5 * scale_of(recorded)        # the fixture's step, from float32 inputs
    single = ts.run_scene(scene, WithTransform(ts.OracleOps(), torch.float32, "cuda"), Net(torch.float32, "cuda", False),
                          torch.float32, "cuda")
    got = ts.run_scene(scene, WithTransform(HipOps(hip_lib), torch.float32, "cuda"), Net(torch.float32, "cuda", True),
                       torch.float32, "cuda")
    got = {k: (v.reshape(want[k].shape) if k in want else v) for k, v in got.items()}
    assert all("grad/input_transform." + k in got for k in KEYS)
    assert all(float(want["grad/input_transform." + k].abs().max()) > 0 for k in KEYS)
    hold_step("input transform -> HIP step -> loss, navier_stokes", got, single, want)
