"""CPU: the input transform (pigs_amd/input_transform.py, csrc/input_transform.hip) -- a torch statement of what it
computes against the recorded InputTransform of the reference (tests/golden/input_transform/, tools/gen_input_transform.py)
and against a closed-form numpy backward, the proof that the GPU bar tells the likely mistakes apart, the C ABI (symbols,
refusals, scratch size) and the module's refusals.  No GPU call is made here.

Shared with tests/test_input_transform_gpu.py:
    load_fixture()      a recorded step: rows, params, recorded results
    make_case()         seeded random rows and parameters with biases of order 1
    oracle()            latent, packed matrices and t_params in torch, generic in dtype; ``mistake`` makes one on purpose
    oracle_all()        those and the gradients of <w, t_params>, as float64 numpy
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "input_transform")

NETS = ("latent_net", "transform_net", "transform_u_net", "transform_ux_net", "transform_uxx_net", "transform_pde_net")
KEYS = tuple(f"{net}.layers.{2 * l}.{kind}" for net in NETS for l in range(3) for kind in ("weight", "bias"))
ROWS = ("means", "full_covariances", "u", "boundaries", "sample_u", "sample_ux", "sample_uxx", "sample_pde")
MATRICES = ("transform", "transform_u", "transform_ux", "transform_uxx", "transform_pde")
RESULTS = ("latent", "matrices", "t_params", "g_means", "g_full_covariances", "g_u") + tuple("g_" + k for k in KEYS)


def sizes(c, p):
    """k of the five matrices"""
    return (2, c, 2 * c, 2 * c, p)


def shapes(c, p):
    """the 36 parameter shapes in the order of KEYS, two-dimensional"""
    out = []
    for i, o in zip((7 + 6 * c + p, 16, 32), (16, 32, 16)):
        out += [(o, i), (o,)]
    for k in sizes(c, p):
        for i, o in ((16, 48), (48, 32), (32, k * k)):
            out += [(o, i), (o,)]
    return out


def scale_of(a):
    a = np.asarray(a)
    return max(float(np.abs(a).max()), 1e-300) if a.size else 1e-300


def load_fixture(name):
    """(rows [8], params [36] two-dimensional, w, recorded {name: array}) of a recorded step, float64 numpy"""
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    rows = [fx["in/" + k] for k in ROWS]
    rows[1] = rows[1].reshape(-1, 4)
    params = [fx["sd/" + k].reshape(fx["sd/" + k].shape[:2]) if fx["sd/" + k].ndim == 3 else fx["sd/" + k] for k in KEYS]
    rec = {"latent": fx["latent"], "matrices": np.concatenate([fx["T/" + k].ravel() for k in MATRICES]),
           "t_params": fx["t_params"], "g_means": fx["grad/means"], "g_full_covariances": fx["grad/full_covariances"].reshape(-1, 4),
           "g_u": fx["grad/u"]}
    for k, prm in zip(KEYS, params):
        rec["g_" + k] = fx["grad/sd/" + k].reshape(prm.shape)
    return rows, params, fx["w"], rec


def make_case(c, p, N, seed, dtype=np.float32):
    """seeded rows and parameters: weights in nn.Linear's range, biases of order 1 (so that a dead row's tanh(bias chain)
    is far from zero), covariances like small Gaussians', a boundary column of zeros and ones; values of ``dtype`` held
    in float64.  The last layer of each TransformNet keeps nn.Linear's own bias range: T = I + B with |B| well below 1,
    what the model's matrices are.  (With a bias of order 1 there a diagonal element 1 + B_ii cancels to a few hundredths
    in some seeds; T_u^T g is then a tensor thirty times smaller than the matrices' rounding times g, and the bar, which
    takes each tensor's own scale, asks of it more digits than a float32 T_u holds.)  Returns (rows, params, w)."""
    rng = np.random.default_rng(seed)

    def cast(a):
        return a.astype(dtype).astype(np.float64)
    widths = {"means": 2, "full_covariances": 4, "u": c, "boundaries": 1, "sample_u": c, "sample_ux": 2 * c,
              "sample_uxx": 2 * c, "sample_pde": p}
    rows = []
    for k in ROWS:
        a = rng.standard_normal((N, widths[k]))
        if k == "boundaries":
            a = (a > 0.5).astype(np.float64)
        if k == "full_covariances":
            a = 0.3 * a
        rows.append(cast(a))
    params = []
    for k, shape in enumerate(shapes(c, p)):
        if len(shape) == 2:
            bound = 1.0 / np.sqrt(shape[1])
            params.append(cast(rng.uniform(-bound, bound, shape)))
        else:
            bound = 1.0 / np.sqrt(32.0) if k >= 6 and k % 6 == 5 else 1.0
            params.append(cast(rng.uniform(-bound, bound, shape)))
    w = cast(rng.standard_normal((N, 5 + 6 * c + p)))
    return rows, params, w


MISTAKES = ("sigma_t", "t_sigma_tt", "transposed", "sum_not_mean", "no_last_tanh", "ux_uxx_exchanged", "sample_u_untouched",
            "no_identity", "dead_rows_counted")


def oracle(rows, params, mistake=None):
    """latent [16], the packed matrices and t_params [N, 5 + 6c + p] from torch tensors of one dtype: steps 1-4 of the
    operator's description.  ``mistake``: one of MISTAKES, made on purpose."""
    means, cov, u, bnd, su, ux, uxx, pde = rows
    N, c, p = u.shape[0], u.shape[1], pde.shape[1]
    x = torch.cat([means, cov, u, bnd.reshape(N, 1), su, ux, uxx, pde], dim=1)
    if mistake == "dead_rows_counted":         # the last tile of 16 filled with rows of zeros
        x = torch.cat([x, x.new_zeros((-N) % 16, x.shape[1])], dim=0)
    a = x
    for l in range(3):
        a = a @ params[2 * l].T + params[2 * l + 1]
        if l < 2 or mistake != "no_last_tanh":
            a = torch.tanh(a)
    latent = a.sum(0) if mistake == "sum_not_mean" else a.sum(0) / N
    T = []
    for j, k in enumerate(sizes(c, p)):
        W1, b1, W2, b2, W3, b3 = params[6 * (j + 1):6 * (j + 2)]
        out = (torch.tanh(torch.tanh(latent @ W1.T + b1) @ W2.T + b2) @ W3.T + b3).reshape(k, k)
        if mistake != "no_identity":
            out = out + torch.eye(k, dtype=out.dtype, device=out.device)
        T.append(out.T if mistake == "transposed" else out)
    if mistake == "ux_uxx_exchanged":
        T[2], T[3] = T[3], T[2]
    sigma = cov.reshape(N, 2, 2)
    t_cov = sigma @ T[0] if mistake == "sigma_t" else T[0] @ sigma @ T[0].T if mistake == "t_sigma_tt" else T[0] @ sigma
    t_su = su if mistake == "sample_u_untouched" else su @ T[1].T
    t_params = torch.cat([t_cov.reshape(N, 4), u @ T[1].T, bnd.reshape(N, 1), t_su, ux @ T[2].T, uxx @ T[3].T, pde @ T[4].T],
                         dim=1)
    return latent, torch.cat([t.reshape(-1) for t in T]), t_params


def oracle_all(rows, params, w, dtype=torch.float64, mistake=None, device="cpu"):
    """{name of RESULTS: float64 numpy}: the oracle and the gradients of <w, t_params> in ``dtype``"""
    def leaf(a, grad):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device).requires_grad_(grad)
    trows = [leaf(a, k < 3) for k, a in enumerate(rows)]
    tparams = [leaf(a, True) for a in params]
    latent, matrices, t_params = oracle(trows, tparams, mistake)
    grads = torch.autograd.grad((leaf(w, False) * t_params).sum(), trows[:3] + tparams)
    out = dict(zip(RESULTS, [latent, matrices, t_params] + list(grads)))
    return {k: v.detach().cpu().double().numpy() for k, v in out.items()}


def numpy_all(rows, params, w):
    """the same in closed form: float64 numpy, no autograd"""
    means, cov, u, bnd, su, ux, uxx, pde = rows
    N, c, p = u.shape[0], u.shape[1], pde.shape[1]
    x = np.concatenate([means, cov, u, bnd.reshape(N, 1), su, ux, uxx, pde], axis=1)
    acts = [x]
    for l in range(3):
        acts.append(np.tanh(acts[-1] @ params[2 * l].T + params[2 * l + 1]))
    latent = acts[3].sum(0) / N
    ks = sizes(c, p)
    T, hidden = [], []
    for j, k in enumerate(ks):
        W1, b1, W2, b2, W3, b3 = params[6 * (j + 1):6 * (j + 2)]
        h1 = np.tanh(W1 @ latent + b1)
        h2 = np.tanh(W2 @ h1 + b2)
        hidden.append((h1, h2))
        T.append(np.eye(k) + (W3 @ h2 + b3).reshape(k, k))
    sigma = cov.reshape(N, 2, 2)
    t_params = np.concatenate([(T[0] @ sigma).reshape(N, 4), u @ T[1].T, bnd.reshape(N, 1), su @ T[1].T, ux @ T[2].T,
                               uxx @ T[3].T, pde @ T[4].T], axis=1)
    # backward of <w, t_params>
    edges = np.cumsum([0, 4, c, 1, c, 2 * c, 2 * c, p])
    g = [w[:, a:b] for a, b in zip(edges[:-1], edges[1:])]       # cov, u, boundaries, sample_u, ux, uxx, pde
    g_sigma = (T[0].T @ g[0].reshape(N, 2, 2)).reshape(N, 4)
    g_u = g[1] @ T[1]
    dT = [np.einsum("nij,nkj->ik", g[0].reshape(N, 2, 2), sigma), g[1].T @ u + g[3].T @ su, g[4].T @ ux, g[5].T @ uxx,
          g[6].T @ pde]
    out = {"latent": latent, "matrices": np.concatenate([t.ravel() for t in T]), "t_params": t_params}
    g_latent = np.zeros(16)
    for j, k in enumerate(ks):
        W1, b1, W2, b2, W3, b3 = params[6 * (j + 1):6 * (j + 2)]
        h1, h2 = hidden[j]
        go = dT[j].ravel()
        dz2 = (W3.T @ go) * (1 - h2 ** 2)
        dz1 = (W2.T @ dz2) * (1 - h1 ** 2)
        grads = [np.outer(dz1, latent), dz1, np.outer(dz2, h1), dz2, np.outer(go, h2), go]
        out.update({"g_" + KEYS[6 * (j + 1) + i]: v for i, v in enumerate(grads)})
        g_latent += W1.T @ dz1
    dz = np.tile(g_latent / N, (N, 1)) * (1 - acts[3] ** 2)
    for l in (2, 1, 0):
        out["g_" + KEYS[2 * l]] = dz.T @ acts[l]
        out["g_" + KEYS[2 * l + 1]] = dz.sum(0)
        da = dz @ params[2 * l]
        if l:
            dz = da * (1 - acts[l] ** 2)
    out["g_means"] = da[:, :2]
    out["g_full_covariances"] = da[:, 2:6] + g_sigma
    out["g_u"] = da[:, 6:6 + c] + g_u
    return out


def worst_gap(got, want):
    """(the largest |got - want| / scale of want over RESULTS, its name)"""
    worst = (0.0, None)
    for k in RESULTS:
        assert got[k].shape == want[k].shape, k
        worst = max(worst, (float(np.abs(got[k] - want[k]).max() / scale_of(want[k])), k))
    return worst


# ---- the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diffusion", "navier_stokes"])
def test_oracle_reproduces_the_recorded_input_transform(name):
    """float64: every recorded tensor and gradient of the reference's module within 1e-10 of the tensor's scale"""
    rows, params, w, recorded = load_fixture(name)
    assert rows[2].shape[0] == {"diffusion": 149, "navier_stokes": 117}[name]
    gap, where = worst_gap(oracle_all(rows, params, w), recorded)
    print(f"{name}: oracle vs the recording, worst {gap:.3g} of a tensor's scale ({where})")
    assert gap <= 1e-10, where


@pytest.mark.parametrize("c,p,N", [(1, 1, 17), (2, 1, 37), (2, 2, 16), (3, 3, 5), (4, 4, 33), (4, 1, 1)])
def test_autograd_through_the_oracle_agrees_with_the_closed_form(c, p, N):
    rows, params, w = make_case(c, p, N, seed=100 * c + 10 * p + N, dtype=np.float64)
    gap, where = worst_gap(numpy_all(rows, params, w), oracle_all(rows, params, w))
    print(f"c={c} p={p} N={N}: closed form vs float64 autograd, worst {gap:.3g} of a tensor's scale ({where})")
    assert gap <= 1e-12, where


def test_closed_form_reproduces_the_recording_too():
    rows, params, w, recorded = load_fixture("navier_stokes")
    gap, where = worst_gap(numpy_all(rows, params, w), recorded)
    assert gap <= 1e-10, where


def allowance(rows, params, w, want):
    """{name: 4 err_torch32 + 1e-6 scale}: what the GPU bar allows each tensor, with the float32 composition's error
    measured here on the CPU"""
    low = oracle_all(rows, params, w, dtype=torch.float32)
    return {k: 4.0 * float(np.abs(low[k] - want[k]).max()) + 1e-6 * scale_of(want[k]) for k in RESULTS}


def discrimination_cases():
    rows, params, w, _ = load_fixture("navier_stokes")
    yield "navier_stokes", rows, params, w
    yield "random c=2 p=2 N=17", *make_case(2, 2, 17, seed=5)


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_bar_tells_each_mistake_from_the_operator(mistake):
    """each mistake, made in the oracle, moves some checked tensor by at least 100 times what the GPU bar allows it, on
    the recorded Navier-Stokes step (N = 117: 11 dead rows in the last tile) and on a random case"""
    for what, rows, params, w in discrimination_cases():
        want = oracle_all(rows, params, w)
        allowed = allowance(rows, params, w, want)
        wrong = oracle_all(rows, params, w, mistake=mistake)
        ratio, where = max((float(np.abs(wrong[k] - want[k]).max()) / allowed[k], k) for k in RESULTS)
        print(f"{mistake} on {what}: {where} moves by {ratio:.3g} allowances")
        assert ratio >= 100.0, (what, where, ratio)


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_input_transform_scratch_bytes", "pigs_input_transform_matrices_forward",
         "pigs_input_transform_matrices_backward", "pigs_input_transform_apply_forward",
         "pigs_input_transform_apply_backward")


def pointers(*v):
    return (ctypes.c_void_p * len(v))(*v)


def test_symbols_declared_exported_and_bound(hip_lib):
    from pigs_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name       # one ctypes type per parameter
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION
    assert _lib.SIGNATURES["pigs_input_transform_scratch_bytes"][0] is ctypes.c_size_t


def record_floats(c, p):
    """the latent net's parameter count: the largest record any launch writes"""
    return 16 * (7 + 6 * c + p + 1) + 32 * 17 + 16 * 33


def test_scratch_size_is_monotone_up_to_its_cap(hip_lib):
    """16 floats and one record per wave, one wave per 16 rows, at most 256 waves"""
    size = hip_lib.pigs_input_transform_scratch_bytes
    for c in (1, 2, 3, 4):
        for p in (1, 2, 3, 4):
            last = 0
            for N in (1, 15, 16, 17, 1600, 4095, 4096, 4097, 65536, 1 << 30):
                got = size(N, c, p)
                assert got == 4 * (16 + min((N + 15) // 16, 256) * record_floats(c, p)), (c, p, N)
                assert got >= last
                last = got
            assert size(4096, c, p) == size(1 << 30, c, p)
            assert size(0, c, p) == 0 and size(-5, c, p) == 0
            assert record_floats(c, p) >= max(16, 2 * (4 + 9 * c * c + p * p))      # the other launches' records fit
    assert size(16, 0, 1) == 0 and size(16, 5, 1) == 0 and size(16, 1, 0) == 0 and size(16, 1, 5) == 0


def test_abi_refusals_come_before_any_hip_call(hip_lib):
    """device pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some, big = None, 1 << 12, 1 << 30
    lib = hip_lib
    full = pointers(*[some] * 36)
    holed = pointers(*([some] * 35 + [null]))

    def mf(dtype=0, N=20, c=2, p=1, rows=None, params=full, scratch=some, nbytes=big, latent=some, matrices=some, hole=None):
        rows = [some] * 8 if rows is None else rows
        if hole is not None:
            rows = list(rows)
            rows[hole] = null
        return lib.pigs_input_transform_matrices_forward(dtype, N, c, p, *rows, params, scratch, nbytes, latent, matrices, None)

    def mb(dtype=0, N=20, c=2, p=1, hole=None, params=full, latent=some, g_matrices=some, scratch=some, nbytes=big,
           g_rows=(some, some, some), g_params=full):
        rows = [some] * 8
        if hole is not None:
            rows[hole] = null
        return lib.pigs_input_transform_matrices_backward(dtype, N, c, p, *rows, params, latent, g_matrices, scratch, nbytes,
                                                          *g_rows, g_params, None)

    def af(dtype=0, N=20, c=2, p=1, matrices=some, hole=None, out=some):
        rows = [some] * 7                      # covariances, u, boundaries, sample_u, ux, uxx, pde
        if hole is not None:
            rows[hole] = null
        return lib.pigs_input_transform_apply_forward(dtype, N, c, p, matrices, *rows, out, None)

    def ab(dtype=0, N=20, c=2, p=1, matrices=some, hole=None, g_t=some, scratch=some, nbytes=big, outs=(some, some, some)):
        rows = [some] * 6                      # covariances, u, sample_u, ux, uxx, pde
        if hole is not None:
            rows[hole] = null
        return lib.pigs_input_transform_apply_backward(dtype, N, c, p, matrices, *rows, g_t, scratch, nbytes, *outs, None)

    need = lib.pigs_input_transform_scratch_bytes(20, 2, 1)
    assert need == 4 * (16 + 2 * record_floats(2, 1))
    for call in (mf, mb, af, ab):
        assert call(dtype=1) == 2 and call(dtype=7) == 2                    # float64, no such dtype
        assert call(c=0) == 2 and call(c=5) == 2 and call(p=0) == 2 and call(p=5) == 2
        assert call(N=0) == 1 and call(N=-3) == 1
    for hole in range(8):
        assert mf(hole=hole) == 1 and mb(hole=hole) == 1
    for hole in (0, 1, 3, 4, 5, 6):            # boundaries (2) may be null in the apply: zeros
        assert af(hole=hole) == 1
    for hole in range(6):
        assert ab(hole=hole) == 1
    assert mf(params=None) == 1 and mf(params=holed) == 1 and mf(latent=null) == 1 and mf(matrices=null) == 1
    assert mb(params=None) == 1 and mb(params=holed) == 1 and mb(latent=null) == 1 and mb(g_matrices=null) == 1
    assert af(matrices=null) == 1 and af(out=null) == 1
    assert ab(matrices=null) == 1 and ab(g_t=null) == 1
    for call in (mf, mb, ab):                  # a null, misaligned or short scratch
        assert call(scratch=null) == 1 and call(scratch=some + 2) == 1
        assert call(nbytes=need - 1) == 1 and call(nbytes=0) == 1
        assert call(N=4097, nbytes=lib.pigs_input_transform_scratch_bytes(4097, 2, 1) - 1) == 1
    # no gradient wanted
    assert mb(g_rows=(null, null, null), g_params=None) == 1
    assert mb(g_rows=(null, null, null), g_params=pointers(*[null] * 36)) == 1
    assert ab(outs=(null, null, null)) == 1


# ---- the Python surface -------------------------------------------------------------------------------------
def reference_like(c=2, p=1, d=2, act=torch.nn.Tanh, kernel=1, bias=True, hidden=48, latent_in=None):
    """a module with the reference's child names and layer types, built here"""
    nn = torch.nn

    class Net(nn.Module):
        def __init__(self, layers):
            super().__init__()
            self.layers = layers

    def transform_net(k):
        return Net(nn.Sequential(nn.Linear(16, hidden), act(), nn.Linear(hidden, 32), act(), nn.Linear(32, k * k, bias=bias)))

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            width = 5 + d * d - 4 + 6 * c + p + d if latent_in is None else latent_in
            self.latent_net = Net(nn.Sequential(nn.Conv1d(width, 16, kernel), act(), nn.Conv1d(16, 32, 1), act(),
                                                nn.Conv1d(32, 16, 1), act()))
            self.transform_net = transform_net(d)
            self.transform_u_net = transform_net(c)
            self.transform_ux_net = transform_net(d * c)
            self.transform_uxx_net = transform_net(d * c)
            self.transform_pde_net = transform_net(p)
    return Holder()


def test_from_module_shares_parameters_and_keeps_the_state_dict(hip_lib):
    import pigs_amd
    nn = torch.nn
    module = reference_like()
    keys, params = list(module.state_dict()), list(module.parameters())
    assert sorted(keys) == sorted(KEYS)
    net = pigs_amd.FusedInputTransform.from_module(module)
    assert isinstance(net, nn.Module) and (net.c, net.d, net.pde_size) == (2, 2, 1)
    assert len(list(net.parameters())) == len(params) and all(a is b for a, b in zip(net.parameters(), params))
    assert list(net.state_dict()) == keys
    by_name = dict(module.named_parameters())
    assert all(a is by_name[k] for a, k in zip(net.params(), KEYS))          # the ABI's order

    class Parent(nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.input_transform = inner
    before = {k: v.clone() for k, v in Parent(module).state_dict().items()}
    after = Parent(net)
    assert list(after.state_dict()) == list(before)            # "input_transform.latent_net.layers.0.weight", ...
    after.load_state_dict({k: v + 1 for k, v in before.items()})
    key = "input_transform.transform_ux_net.layers.4.bias"
    assert torch.equal(module.transform_ux_net.layers[4].bias, before[key] + 1)      # the same storage was loaded into
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(*cpu_rows())


UNSUPPORTED = {                     # the words the refusal must hold: the module that makes it
    "ReLU": dict(act=torch.nn.ReLU),
    "Sigmoid": dict(act=torch.nn.Sigmoid),
    "kernel size": dict(kernel=3),
    "bias=False": dict(bias=False),
    "widths": dict(hidden=40),
    "latent_net has widths": dict(latent_in=21),
    "d = 2": dict(d=3),
    "1..4": dict(c=5),
}


@pytest.mark.parametrize("what", list(UNSUPPORTED), ids=[re.sub(r"\W+", "_", k) for k in UNSUPPORTED])
def test_from_module_refuses_by_name(hip_lib, what):
    import pigs_amd
    with pytest.raises(NotImplementedError, match=re.escape(what)):
        pigs_amd.FusedInputTransform.from_module(reference_like(**UNSUPPORTED[what]))


def test_from_module_needs_the_reference_child_names(hip_lib):
    import pigs_amd
    with pytest.raises(TypeError, match="latent_net"):
        pigs_amd.FusedInputTransform.from_module(torch.nn.Linear(4, 4))
    module = reference_like()
    module.transform_u_net.layers = torch.nn.Linear(16, 4)
    with pytest.raises(TypeError, match="transform_u_net"):
        pigs_amd.FusedInputTransform.from_module(module)
    module = reference_like()
    module.transform_pde_net.layers = torch.nn.Sequential(*list(module.transform_pde_net.layers)[:3])
    with pytest.raises(NotImplementedError, match="transform_pde_net"):
        pigs_amd.FusedInputTransform.from_module(module)


def cpu_rows(N=5, c=2, p=1, dtype=torch.float32):
    widths = (2, 4, c, 1, c, 2 * c, 2 * c, p)
    return [torch.zeros(N, w, dtype=dtype) for w in widths]


def test_the_functions_refuse_cpu_tensors_and_bad_arguments(hip_lib):
    import pigs_amd
    tm, ap = pigs_amd.transform_matrices, pigs_amd.apply_transforms
    params = [torch.zeros(s) for s in shapes(2, 1)]
    matrices = torch.zeros(4 + 36 + 1)
    rows = cpu_rows()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tm(*rows, params)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap(matrices, *rows[1:])
    with pytest.raises(TypeError):
        tm(*cpu_rows(dtype=torch.float64), [t.double() for t in params])           # float64 is not built
    with pytest.raises(TypeError):
        ap(matrices.double(), *cpu_rows(dtype=torch.float64)[1:])
    with pytest.raises(TypeError):
        tm(rows[0].numpy(), *rows[1:], params)
    with pytest.raises(TypeError):
        tm(*rows[:3], None, *rows[4:], params)                                     # the latent net reads boundaries
    for k in range(3, 8):                      # what the model makes under no_grad
        bad = list(rows)
        bad[k] = bad[k].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=ROWS[k]):
            tm(*bad, params)
        with pytest.raises(NotImplementedError, match=ROWS[k]):
            ap(matrices, *bad[1:])
    with pytest.raises(NotImplementedError, match="d = 2"):
        tm(torch.zeros(5, 3), *rows[1:], params)
    with pytest.raises(NotImplementedError, match="d = 2"):
        ap(matrices, torch.zeros(5, 3, 3), *rows[2:])
    with pytest.raises(NotImplementedError, match="1..4"):
        ap(matrices, *cpu_rows(c=5)[1:])
    with pytest.raises(ValueError):
        tm(*cpu_rows(N=0), params)
    with pytest.raises(ValueError):
        tm(*rows[:5], torch.zeros(5, 3), *rows[6:], params)                        # sample_ux is not [N, 2c]
    with pytest.raises(ValueError):
        tm(*rows, params[:-1])
    with pytest.raises(ValueError):
        tm(*rows, params[:4] + [torch.zeros(16, 33)] + params[5:])
    with pytest.raises(ValueError):
        ap(torch.zeros(40), *rows[1:])
    with pytest.raises(ValueError, match="contiguous"):
        tm(*rows[:2], torch.zeros(5, 4)[:, ::2], *rows[3:], params)
    with pytest.raises(ValueError, match="contiguous"):
        tm(*rows, [torch.zeros(params[0].shape[::-1]).t()] + params[1:])
