"""CPU: refinement (pigs_amd/refine.py, csrc/refine.hip) -- its float64 checker against an independent restatement
of the reference's lines, the closed form's float32 error, the C ABI's refusals.  No GPU call is made here.

The checker, shared with tests/test_refine_gpu.py:
    refine_oracle()            the semantics of include/pigs_amd.h (pigs_refine_*) in float64 numpy, the eigenpair
                               from np.linalg.eigh
    reference_split_restated() model_pn.py:703-714 + :586-601 restated with torch.linalg.eig on the CPU
    closed_form_displacement() the kernel's closed form in a numpy dtype of choice
Both canonicalise the order of a pair of children by the sign convention e_x > 0, or e_x = 0 and e_y > 0.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the input family ---------------------------------------------------------------------------------------
def family(N, c=1, seed=0):
    """means U[-1,1]^2, scaling log-uniform in [1e-4, 0.5], transforms N(0,1), values N(0,1); float64"""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1.0, 1.0, (N, 2))
    scaling = np.exp(rng.uniform(np.log(1e-4), np.log(0.5), (N, 2)))
    transforms = rng.standard_normal((N, 1))
    values = rng.standard_normal((N, c))
    return means, scaling, transforms, values


def covariance_matrices(scaling, t):
    tau = np.tanh(t) * np.sqrt(scaling[:, 0] * scaling[:, 1])
    return np.stack((np.stack((scaling[:, 0], tau), -1), np.stack((tau, scaling[:, 1]), -1)), -2)


def canonical_sign(e):
    flip = (e[:, 0] < 0) | ((e[:, 0] == 0) & (e[:, 1] < 0))
    return np.where(flip[:, None], -e, e)


def eigh_displacement(scaling, t):
    """(e, lambda_max) of every row: lambda_max times the unit eigenvector (model_pn.py:587-589), float64"""
    if len(scaling) == 0:
        return np.zeros((0, 2)), np.zeros(0)
    w, V = np.linalg.eigh(covariance_matrices(scaling.astype(np.float64), t.astype(np.float64)))
    lam = w[:, 1]                       # ascending; the matrices are positive definite, so the last is max |lambda|
    return canonical_sign(lam[:, None] * V[:, :, 1]), lam


def refine_oracle(means, scaling, transforms, values, keep, split, mode="split", value_scale=0.5):
    """The semantics of pigs_refine_* in float64 numpy.  Returns a namespace: means, scaling, transforms [N'],
    values, source, child, n_kept, n_split, and for mode "split" e, lam (per split parent, input order)."""
    N = len(means)
    keep = np.ones(N, bool) if keep is None else np.asarray(keep, bool)
    split = np.zeros(N, bool) if split is None else np.asarray(split, bool)
    split = split & keep                                         # pruned wins
    t = np.asarray(transforms, np.float64).reshape(N)
    means, scaling, values = (np.asarray(a, np.float64) for a in (means, scaling, values))
    parents = np.flatnonzero(split)
    o = types.SimpleNamespace(n_kept=int(keep.sum()), n_split=len(parents), e=None, lam=None)
    if mode == "clone":
        o.source = np.concatenate((np.flatnonzero(keep), parents))
        o.child = np.concatenate((np.full(o.n_kept, -1), np.zeros(o.n_split, int))).astype(np.int32)
        o.means, o.values = means[o.source], values[o.source]
    else:
        plain = np.flatnonzero(keep & ~split)
        o.source = np.concatenate((plain, np.repeat(parents, 2)))
        o.child = np.concatenate((np.full(len(plain), -1), np.tile([0, 1], o.n_split))).astype(np.int32)
        o.e, o.lam = eigh_displacement(scaling[parents], t[parents])
        o.means = means[o.source].copy()
        o.means[len(plain)::2] -= o.e
        o.means[len(plain) + 1::2] += o.e
        o.values = values[o.source] * np.where(o.child >= 0, value_scale, 1.0)[:, None]
    o.scaling, o.transforms = scaling[o.source], t[o.source]
    return o


def reference_split_restated(means, scaling, transforms, values, keep, split):
    """model_pn.py:703-714 (prune by one mask) and :586-601 (Model.split) in float64 torch on the CPU:
    torch.linalg.eig, the eigenpair of largest |eigenvalue|, children at -/+ eigenvalue * eigenvector, u / 2.
    Itself held to a recorded forward of the reference in tests/test_model_split.py."""
    m, s, t, u = (torch.as_tensor(np.asarray(a, np.float64)) for a in (means, scaling, transforms, values))
    kept = torch.as_tensor(keep)
    m, s, t, u = m[kept], s[kept], t[kept], u[kept]
    chosen = torch.as_tensor(split)[kept]
    off = torch.tanh(t[:, 0]) * torch.sqrt(s[:, 0] * s[:, 1])
    full = torch.stack((s[:, 0], off, off, s[:, 1]), -1).reshape(-1, 2, 2)
    n = int(chosen.sum())
    w, V = torch.linalg.eig(full[chosen])
    size, which = w.real.abs().max(dim=-1)
    vec = V.real[torch.arange(n), :, which]                      # the columns of V are the eigenvectors
    e = torch.as_tensor(canonical_sign((size[:, None] * vec).numpy()))
    pairs = torch.stack((m[chosen] - e, m[chosen] + e), dim=1).reshape(-1, 2)
    twice = torch.arange(n).repeat_interleave(2)
    return (torch.cat((m[~chosen], pairs)).numpy(), torch.cat((s[~chosen], s[chosen][twice])).numpy(),
            torch.cat((t[~chosen], t[chosen][twice])).numpy()[:, 0], torch.cat((u[~chosen], u[chosen][twice] / 2.0)).numpy())


def closed_form_displacement(scaling, t, dtype):
    """The kernel's closed form (csrc/refine.hip, split_displacement) with every operation in `dtype`."""
    s0, s1, t = scaling[:, 0].astype(dtype), scaling[:, 1].astype(dtype), t.astype(dtype)
    half = dtype(0.5)
    tau = np.tanh(t) * np.sqrt(s0 * s1)
    m, delta = half * (s0 + s1), half * (s0 - s1)
    r = np.sqrt(delta * delta + tau * tau)
    lam = m + r
    pos = delta >= 0
    vx, vy = np.where(pos, r + delta, tau), np.where(pos, tau, r - delta)
    n = np.sqrt(vx * vx + vy * vy)
    iso = r == 0
    n = np.where(iso, dtype(1), n)
    vx, vy = np.where(iso, dtype(1), vx / n), np.where(iso, dtype(0), vy / n)
    flip = vx < 0
    vx, vy = np.where(flip, -vx, vx), np.where(flip, -vy, vy)
    assert lam.dtype == dtype and vx.dtype == dtype
    return np.stack((lam * vx, lam * vy), -1), lam


def random_masks(N, p_split, p_prune, seed):
    rng = np.random.default_rng(seed + 7919)
    return rng.random(N) >= p_prune, rng.random(N) < p_split


# ---- the checker against the reference's lines --------------------------------------------------------------
def test_oracle_agrees_with_the_restated_reference():
    """eigh vs torch.linalg.eig on 20 000 rows of the family, all split: 1e-12 * lambda_max"""
    N = 20000
    means, scaling, transforms, values = family(N, c=2, seed=1)
    keep, _ = random_masks(N, 0.0, 0.05, 1)
    split = np.ones(N, bool)
    o = refine_oracle(means, scaling, transforms, values, keep, split)
    rm, rs, rt, ru = reference_split_restated(means, scaling, transforms, values, keep, split & keep)
    lam = np.repeat(o.lam, 2)[:, None]
    worst = (np.abs(o.means - rm) / lam).max()
    print(f"eigh vs linalg.eig: worst |child difference| / lambda_max = {worst:.3g}")
    assert worst <= 1e-12
    assert np.array_equal(o.scaling, rs) and np.array_equal(o.transforms, rt) and np.array_equal(o.values, ru)


def test_oracle_order_with_unsplit_rows_matches_the_restated_reference():
    N = 3000
    means, scaling, transforms, values = family(N, c=3, seed=2)
    keep, split = random_masks(N, 0.3, 0.2, 2)
    o = refine_oracle(means, scaling, transforms, values, keep, split)
    rm, rs, rt, ru = reference_split_restated(means, scaling, transforms, values, keep, split & keep)
    assert o.means.shape == rm.shape and len(o.source) == o.n_kept + o.n_split
    plain = o.child < 0
    assert np.array_equal(o.means[plain], rm[plain])
    assert (np.abs(o.means - rm)[~plain] <= 1e-12 * np.repeat(o.lam, 2)[:, None]).all()
    assert np.array_equal(o.scaling, rs) and np.array_equal(o.transforms, rt) and np.array_equal(o.values, ru)


def test_clone_oracle_is_the_densification_of_test_no_mlp():
    """test_no_mlp.py:198-240: cat((x[keep_mask], x[split_indices])) on the four arrays, zeros appended to Adam's
    moments -- the latter through source / child"""
    N = 2000
    arrays = family(N, c=2, seed=3)
    keep, split = random_masks(N, 0.1, 0.3, 3)
    split_indices = split & keep                                 # :205
    o = refine_oracle(*arrays, keep, split, mode="clone")
    for got, x in zip((o.means, o.scaling, o.transforms, o.values), arrays):
        want = torch.cat((torch.as_tensor(x)[torch.as_tensor(keep)], torch.as_tensor(x)[torch.as_tensor(split_indices)]))
        assert np.array_equal(got, want.numpy().reshape(got.shape))
    rng = np.random.default_rng(3)
    for x in arrays:
        exp_avg = torch.as_tensor(rng.standard_normal(x.shape))
        extension = torch.as_tensor(x)[torch.as_tensor(split_indices)]
        want = torch.cat((exp_avg[torch.as_tensor(keep)], torch.zeros_like(extension)), dim=0)      # :222-225
        carried = exp_avg.index_select(0, torch.as_tensor(o.source))
        got = torch.where(torch.as_tensor(o.child >= 0)[:, None], torch.zeros_like(carried), carried)
        assert torch.equal(got, want)


# ---- the closed form ----------------------------------------------------------------------------------------
def test_float64_closed_form_is_the_oracle():
    _, scaling, transforms, _ = family(20000, seed=4)
    e, lam = closed_form_displacement(scaling, transforms[:, 0], np.float64)
    want, wlam = eigh_displacement(scaling, transforms[:, 0])
    worst = (np.abs(e - want).max(-1) / wlam).max()
    print(f"float64 closed form vs eigh: {worst:.3g} lambda_max")
    assert worst <= 1e-12 and (np.abs(lam - wlam) <= 1e-12 * wlam).all()


def test_float32_closed_form_error():
    """inputs held in float32; 1e-5 is the project's float32 bar"""
    _, scaling, transforms, _ = family(20000, seed=5)
    scaling, t = scaling.astype(np.float32), transforms[:, 0].astype(np.float32)
    e, lam = closed_form_displacement(scaling, t, np.float32)
    want, wlam = eigh_displacement(scaling, t)
    worst = (np.abs(e.astype(np.float64) - want).max(-1) / wlam).max()
    sigma = covariance_matrices(scaling.astype(np.float64), t.astype(np.float64))
    e64 = e.astype(np.float64)
    resid = np.linalg.norm(np.einsum("nij,nj->ni", sigma, e64) - wlam[:, None] * e64, axis=-1) / wlam ** 2
    print(f"float32 closed form: {worst:.3g} lambda_max, eigen-residual {resid.max():.3g} lambda_max^2")
    assert worst <= 1e-5
    assert resid.max() <= 1e-5


def test_closed_form_planted_rows():
    s = np.array([[0.3, 0.3], [0.4, 0.1], [0.1, 0.4], [0.2, 0.3], [0.2, 0.3]])
    t = np.array([0.0, 0.0, 0.0, 8.0, -8.0])
    for dtype in (np.float32, np.float64):
        e, lam = closed_form_displacement(s, t, dtype)
        assert e[0, 0] == dtype(0.3) and e[0, 1] == 0           # isotropic: (lambda, 0) exactly
        assert e[1, 1] == 0 and abs(e[1, 0] - 0.4) <= 1e-6      # axis-aligned
        assert e[2, 0] == 0 and abs(e[2, 1] - 0.4) <= 1e-6
        assert np.isfinite(e).all() and (e[:, 0] >= 0).all()


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_refine_workspace_bytes", "pigs_refine_index", "pigs_refine_apply", "pigs_refine_backward")


def test_symbols_declared_exported_and_bound(hip_lib):
    from pigs_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION


def test_workspace_bytes_is_a_pure_monotone_function_of_n(hip_lib):
    from pigs_amd import refine
    f = hip_lib.pigs_refine_workspace_bytes
    last = 0
    for N in (1, 63, 1024, 1025, 300001, 1 << 24, (1 << 31) - 1):
        b = f(N)
        assert b >= last and b > 0 and b == f(N)
        last = b
    assert f(-1) == 0 and f(-(1 << 40)) == 0 and f(0) == 0 and f(1 << 31) == 0
    # 16 bytes per workgroup of ROWS_PER_WORKGROUP rows: the module's constant is the kernels'
    R = refine.ROWS_PER_WORKGROUP
    assert f(R) == 16 and f(R + 1) == 32


def test_refusals_come_before_any_hip_call(hip_lib):
    """null pointers everywhere: a call that got as far as a launch would fault; none does"""
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(1 << 12)                               # never dereferenced: the call is refused first
    index, apply, backward = hip_lib.pigs_refine_index, hip_lib.pigs_refine_apply, hip_lib.pigs_refine_backward
    assert index(2, 4, *([null] * 3), 0, *([null] * 4)) == 2                  # mode
    assert index(0, -1, *([null] * 3), 0, *([null] * 4)) == 1                 # negative size
    assert index(0, 1 << 31, *([null] * 3), 0, *([null] * 4)) == 2            # a size the path does not take
    assert index(0, 4, *([null] * 3), 0, *([null] * 4)) == 1                  # null required arrays
    assert index(0, 0, *([null] * 3), 0, *([null] * 4)) == 0                  # N = 0: ok, no launch
    need = hip_lib.pigs_refine_workspace_bytes(5000)
    assert index(0, 5000, null, null, some, need - 1, some, some, some, null) == 4    # workspace one byte short
    for f, n in ((apply, 13), (backward, 11)):
        nulls = [null] * n
        assert f(7, 0, 1, 4, 4, 0.5, *nulls) == 2                             # dtype
        assert f(0, 5, 1, 4, 4, 0.5, *nulls) == 2                             # mode
        assert f(0, 0, 0, 4, 4, 0.5, *nulls) == 1                             # c < 1
        assert f(0, 0, 1, -4, 4, 0.5, *nulls) == 1                            # negative N
        assert f(0, 0, 1, 4, -4, 0.5, *nulls) == 1                            # negative rows
        assert f(0, 0, 1, 4, 4, 0.5, *nulls) == 1                             # null maps
        assert f(1, 1, 3, 0, 0, 0.5, *nulls) == 0                             # N = 0: ok, no launch
    assert apply(0, 0, 1, 4, 0, 0.5, *([null] * 13)) == 0                     # rows = 0: nothing to write
    # a wanted output without its input; a misaligned row array
    assert apply(0, 0, 1, 4, 4, 0.5, some, some, null, null, null, null, some, null, null, null, null, null, null) == 1
    odd = ctypes.c_void_p((1 << 12) + 4)
    assert apply(0, 1, 1, 4, 4, 0.5, some, some, odd, null, null, null, some, null, null, null, null, null, null) == 1


# ---- the Python surface -------------------------------------------------------------------------------------
def test_split_gaussians_refuses_cpu_tensors_and_bad_shapes(hip_lib):
    import pigs_amd
    from pigs_amd import refine
    assert pigs_amd.split_gaussians is refine.split_gaussians and pigs_amd.refine_index is refine.refine_index
    means, s, t, u = torch.zeros(4, 2), torch.ones(4, 2), torch.zeros(4, 1), torch.ones(4, 3)
    mask = torch.zeros(4, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.split_gaussians(means, s, t, u, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        refine.refine_index(mask, None)
    with pytest.raises(NotImplementedError):
        refine.split_gaussians(torch.zeros(4, 1), torch.ones(4, 1), t, u, mask)          # d = 1
    with pytest.raises(NotImplementedError):
        refine.split_gaussians(torch.zeros(4, 3), s, t, u, mask)
    with pytest.raises(ValueError):
        refine.split_gaussians(means, s, t, torch.ones(5, 3), mask)                       # row counts differ
    with pytest.raises(ValueError):
        refine.split_gaussians(means, s, t, u, mask, mode="halve")
    with pytest.raises(TypeError):
        refine.split_gaussians(means, s, t, u, mask.to(torch.uint8))                      # an integer mask
    with pytest.raises(TypeError):
        refine.split_gaussians(means, s, t, u, torch.zeros(4, requires_grad=True))        # a mask that wants a gradient
