"""GPU: refinement (pigs_amd.refine -> pigs_refine_*) against the float64 checker of tests/test_refine.py.

Bars: 1e-5 (float32, the project's bar) and 1e-12 (float64), each times the scale the quantity lives on: lambda_max
for e, lambda_max^2 for the eigen-residual, max(|mu|_inf, lambda_max) for a child (a child is mu -/+ e rounded to the
dtype).  Everything that is a copy or a multiplication by 0.5 is compared bit for bit.

The kernel's own e is read exactly: a second call on the same rows with all means zero returns children -e and +e.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from test_refine import covariance_matrices, family, random_masks, refine_oracle

pytestmark = pytest.mark.gpu

BAR = {torch.float32: 1e-5, torch.float64: 1e-12}
NP = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module")
def refine(hip_lib):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from pigs_amd import refine
    return refine


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().double().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


# ---- sizes and masks ----------------------------------------------------------------------------------------
R, W = 1024, 256                     # asserted against the module's constants in test_sizes_cover_the_mechanisms
MULTI_PASS = 300001                  # > R * W: the one-workgroup scan of the totals takes a second pass
SIZES = [0, 1, 63, 64, 65, R - 1, R, R + 1, MULTI_PASS]
MASKS = ["none_split", "all_split", "all_pruned", "alternating", "random_2_5", "random_50_50", "split_on_pruned",
         "keep_none", "split_none"]


def test_sizes_cover_the_mechanisms(refine):
    assert (refine.ROWS_PER_WORKGROUP, refine.SCAN_WIDTH) == (R, W)
    assert MULTI_PASS > R * W


def masks_of(kind, N, seed):
    """(keep, split) as numpy bool arrays or None"""
    i = np.arange(N)
    if kind == "none_split":
        return random_masks(N, 0.0, 0.05, seed)[0], np.zeros(N, bool)
    if kind == "all_split":
        return np.ones(N, bool), np.ones(N, bool)
    if kind == "all_pruned":
        return np.zeros(N, bool), random_masks(N, 0.5, 0.0, seed)[1]
    if kind == "alternating":
        return i % 3 != 0, i % 2 == 0
    if kind == "random_2_5":
        return random_masks(N, 0.02, 0.05, seed)
    if kind == "random_50_50":
        return random_masks(N, 0.5, 0.5, seed)
    if kind == "split_on_pruned":                                 # every pruned row carries a split bit: pruned wins
        keep, split = random_masks(N, 0.3, 0.5, seed)
        return keep, split | ~keep
    if kind == "keep_none":
        return None, random_masks(N, 0.2, 0.0, seed)[1]
    if kind == "split_none":
        return random_masks(N, 0.0, 0.3, seed)[0], None
    raise KeyError(kind)


# ---- one case against the oracle ----------------------------------------------------------------------------
def check_case(refine, N, kind, mode, dtype, c, seed=0, value_scale=0.5):
    arrays = [a.astype(NP[dtype]) for a in family(N, c, seed)]   # held in the dtype: the oracle sees the same numbers
    keep, split = masks_of(kind, N, seed)
    o = refine_oracle(*arrays, keep, split, mode=mode, value_scale=value_scale)
    means, scaling, transforms, values = (dev(a) for a in arrays)
    got = refine.split_gaussians(means, scaling, transforms, values, dev(split), dev(keep), mode=mode,
                                 value_scale=value_scale)
    rows = o.n_kept + o.n_split
    assert got.means.shape == (rows, 2) and got.scaling.shape == (rows, 2) and got.transforms.shape == (rows, 1)
    assert got.values.shape == (rows, c) and got.source.shape == (rows,) and got.child.shape == (rows,)
    assert got.source.dtype == torch.int64 and got.child.dtype == torch.int32 and got.means.dtype == dtype
    assert np.array_equal(host(got.source), o.source) and np.array_equal(host(got.child), o.child)
    assert int((got.child < 0).sum()) == (o.n_kept - o.n_split if mode == "split" else o.n_kept)
    # copies and the exact scaling: bit for bit against the gathered inputs
    is_child = (got.child >= 0)[:, None]
    assert torch.equal(got.scaling, scaling.index_select(0, got.source))
    assert torch.equal(got.transforms, transforms.index_select(0, got.source))
    carried = values.index_select(0, got.source)
    assert torch.equal(got.values, torch.where(is_child, value_scale * carried, carried) if mode == "split" else carried)
    carried = means.index_select(0, got.source)
    if mode == "clone":
        assert torch.equal(got.means, carried)
        return
    assert torch.equal(got.means[got.child < 0], carried[got.child < 0])
    if o.n_split == 0:
        return
    # the children
    bar = BAR[dtype]
    first = o.n_kept - o.n_split
    zero = refine.split_gaussians(torch.zeros_like(means), scaling, transforms, values, dev(split), dev(keep))
    e = host(zero.means)[first + 1::2]                            # the kernel's e, exactly
    assert np.array_equal(host(zero.means)[first::2], -e)
    children, mu, lam = host(got.means)[first:], host(carried)[first::2], o.lam
    parents = o.source[first::2]
    scale = np.maximum(np.abs(mu).max(-1), lam)
    mid = np.abs(0.5 * (children[0::2] + children[1::2]) - mu).max(-1) / scale
    length = np.abs(np.linalg.norm(e, axis=-1) - lam) / lam
    sigma = covariance_matrices(arrays[1][parents].astype(np.float64), arrays[2][parents, 0].astype(np.float64))
    resid = np.linalg.norm(np.einsum("nij,nj->ni", sigma, e) - lam[:, None] * e, axis=-1) / lam ** 2
    # against the oracle's children, in order; the two exceptions of the direction
    r_over_m = (2 * lam - (arrays[1][parents].astype(np.float64).sum(-1))) / arrays[1][parents].astype(np.float64).sum(-1)
    skip = r_over_m < 0.05                                        # lambda_max = m + r: r / m = (2 lambda - 2 m) / 2 m
    swap_ok = ~skip & (np.abs(o.e[:, 0] / lam) < 1e-3)
    err = np.abs(children - o.means[first:]).max(-1).reshape(-1, 2).max(-1) / scale
    swapped = np.abs(children.reshape(-1, 2, 2)[:, ::-1].reshape(-1, 2) - o.means[first:]).max(-1).reshape(-1, 2).max(-1) / scale
    err = np.where(swap_ok, np.minimum(err, swapped), err)
    err = np.where(skip, 0.0, err)
    n_exc = int(skip.sum() + swap_ok.sum())
    print(f"N={N} {kind} {mode} {dtype} c={c}: split rows {o.n_split}, exceptions {n_exc}; worst / bar: "
          f"midpoint {mid.max() / bar:.3g}, |e| {length.max() / bar:.3g}, residual {resid.max() / bar:.3g}, "
          f"children {err.max() / bar:.3g}")
    assert np.isfinite(children).all()
    assert mid.max() <= bar and length.max() <= bar and resid.max() <= bar
    assert err.max() <= bar
    # at most 1 % of the split rows; below 100 split rows 1 % is less than one row, and one row is the granularity
    assert n_exc <= max(0.01 * o.n_split, 1), (n_exc, o.n_split)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("N", SIZES)
def test_split_f32(refine, N, kind):
    check_case(refine, N, kind, "split", torch.float32, 1, seed=N % 1000 + len(kind))


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("N", SIZES)
def test_clone_f64(refine, N, kind):
    check_case(refine, N, kind, "clone", torch.float64, 2, seed=N % 1000 + len(kind))


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("mode", ["split", "clone"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [R + 1, 2 * R + 451])
def test_dtypes_modes_channels(refine, N, dtype, mode, c):
    check_case(refine, N, "random_2_5", mode, dtype, c, seed=11 + c)
    check_case(refine, N, "random_50_50", mode, dtype, c, seed=12 + c, value_scale=0.25)


def test_transforms_keep_their_trailing_shape_and_views_are_taken(refine):
    N = 200
    means, scaling, transforms, values = (dev(a, torch.float32) for a in family(N, 2, 5))
    split = dev(random_masks(N, 0.3, 0.0, 5)[1])
    a = refine.split_gaussians(means, scaling, transforms, values, split)
    b = refine.split_gaussians(means, scaling, transforms[:, 0], values, split)
    assert a.transforms.dim() == 2 and b.transforms.dim() == 1 and torch.equal(a.transforms[:, 0], b.transforms)
    wide = torch.zeros(N, 5, device="cuda")
    wide[:, 1:3], wide[:, 3:5] = means, scaling                   # non-contiguous, rows not aligned to 8 bytes
    c = refine.split_gaussians(wide[:, 1:3], wide[:, 3:5], transforms, values, split)
    assert torch.equal(a.means, c.means) and torch.equal(a.scaling, c.scaling)
    flat = torch.zeros(2 * N + 1, device="cuda")
    flat[1:] = means.reshape(-1)                                  # contiguous, but every row straddles an 8-byte boundary
    d = refine.split_gaussians(flat[1:].view(N, 2), scaling, transforms, values, split)
    assert flat[1:].data_ptr() % 8 == 4 and torch.equal(a.means, d.means)
    src, child = refine.refine_index(None, split)
    assert torch.equal(src, a.source) and torch.equal(child, a.child)
    with pytest.raises(TypeError):
        refine.split_gaussians(means, scaling.double(), transforms, values, split)
    with pytest.raises(TypeError):
        refine.split_gaussians(means.long(), scaling.long(), transforms.long(), values.long(), split)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_planted_rows(refine, dtype):
    s = dev([[0.3, 0.3], [0.4, 0.1], [0.1, 0.4], [0.2, 0.3], [0.2, 0.3]], dtype)
    t = dev([[0.0], [0.0], [0.0], [8.0], [-8.0]], dtype)
    zero, ones = torch.zeros(5, 2, dtype=dtype, device="cuda"), torch.ones(5, 1, dtype=dtype, device="cuda")
    out = refine.split_gaussians(zero, s, t, ones, torch.ones(5, dtype=torch.bool, device="cuda"))
    e = out.means[1::2]
    assert torch.equal(out.means[0::2], -e)
    assert torch.equal(e[0], s[0, 0] * dev([1.0, 0.0], dtype))   # exactly isotropic: (lambda, 0) exactly
    assert e[1, 1] == 0 and abs(float(e[1, 0]) - 0.4) <= BAR[dtype] * 0.4     # t = 0: the longer axis
    assert e[2, 0] == 0 and abs(float(e[2, 1]) - 0.4) <= BAR[dtype] * 0.4
    assert torch.isfinite(out.means).all() and (e[:, 0] >= 0).all()
    lam = 0.25 + np.sqrt(0.05 ** 2 + np.tanh(8.0) ** 2 * 0.06)    # |t| = 8: the closed form in float64
    assert abs(float(e[3].double().norm()) - lam) <= BAR[dtype] * lam and e[3, 1] > 0 and e[4, 1] < 0


# ---- backward -----------------------------------------------------------------------------------------------
def composition(inputs, out, mode, value_scale):
    """index_select by source, add the kernel's own e as a constant, scale: what torch.autograd differentiates"""
    means, scaling, transforms, values = inputs
    with torch.no_grad():
        e = out.means - means.index_select(0, out.source)         # exactly 0 on the kept rows
        factor = torch.where(out.child >= 0, value_scale, 1.0).to(values.dtype)[:, None] if mode == "split" else 1.0
    return (means.index_select(0, out.source) + e, scaling.index_select(0, out.source),
            transforms.index_select(0, out.source), values.index_select(0, out.source) * factor)


def normal_range(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return ((0.5 + 1.5 * torch.rand(shape, generator=g)) * sign).to(dtype).cuda()


def grads(outputs, inputs, gouts, present):
    outs = [o for o, p in zip(outputs, present) if p]
    got = torch.autograd.grad(outs, inputs, [g for g, p in zip(gouts, present) if p], allow_unused=True, retain_graph=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(got, inputs)]


@pytest.mark.parametrize("mode", ["split", "clone"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_backward_equals_autograd_of_the_composition(refine, dtype, mode):
    """sums of at most two terms in the same dtype: torch.equal, for every subset of incoming gradients"""
    N, c = 2 * R + 77, 3
    inputs = [dev(a, dtype).requires_grad_(True) for a in family(N, c, 21)]
    keep, split = (dev(m) for m in random_masks(N, 0.3, 0.2, 21))
    out = refine.split_gaussians(*inputs, split, keep, mode=mode)
    ref = composition(inputs, out, mode, 0.5)
    for a, b in zip(out[1:4], ref[1:]):                           # (the means are mu + fl(child - mu): not the same rounding)
        assert torch.equal(a, b)
    gouts = [normal_range(o.shape, dtype, 30 + k) for k, o in enumerate(out[:4])]
    for present in itertools.product([False, True], repeat=4):
        if not any(present):
            continue
        got, want = grads(out[:4], inputs, gouts, present), grads(ref, inputs, gouts, present)
        again = grads(out[:4], inputs, gouts, present)            # a second backward through the retained graph
        for g, w, g2, x in zip(got, want, again, inputs):
            assert g.shape == x.shape and torch.equal(g, w) and torch.equal(g, g2), present
    pruned = ~keep
    assert pruned.any() and all((g[pruned] == 0).all() for g in got)


def test_backward_values_alone_and_no_incoming_gradient(refine):
    N = 300
    means, scaling, transforms, values = (dev(a, torch.float32) for a in family(N, 2, 22))
    values.requires_grad_(True)
    keep, split = (dev(m) for m in random_masks(N, 0.3, 0.2, 22))
    out = refine.split_gaussians(means, scaling, transforms, values, split, keep)
    assert out.values.requires_grad and not out.source.requires_grad and not out.child.requires_grad
    g = normal_range(out.values.shape, torch.float32, 1)
    (got,) = torch.autograd.grad(out.values, values, g)
    factor = torch.where(out.child >= 0, 0.5, 1.0)[:, None]
    want = torch.zeros_like(values).index_add_(0, out.source, g * factor)
    assert torch.equal(got, want)
    # nothing flows into an output: the inputs' gradients are None or zero, and nothing is launched for them
    means.requires_grad_(True)
    out = refine.split_gaussians(means, scaling, transforms, values.detach(), split, keep)
    (got,) = torch.autograd.grad(out.scaling.sum() * 0 + out.means.sum(), means)
    assert torch.equal(got, torch.zeros_like(means).index_add_(0, out.source, torch.ones_like(out.means)))


def test_gradcheck_f64(refine):
    """N = 37, float64.  e is a constant of the backward (model_pn.py:584-585) but a function of scaling and transforms
    in the forward, so finite differences see d(children) / d(scaling) where the analytic Jacobian has 0 by design:
    the check runs wherever e does not move -- all inputs and outputs in clone mode; in split mode means and values
    against all outputs, and scaling and transforms against every output but the means."""
    N = 37
    means, scaling, transforms, values = (dev(a, torch.float64) for a in family(N, 2, 23))
    keep, split = (dev(m) for m in random_masks(N, 0.4, 0.2, 23))
    assert int((split & keep).sum()) >= 5 and int((~keep).sum()) >= 3
    from torch.autograd import gradcheck

    def var(*ts):
        return [t.clone().requires_grad_(True) for t in ts]
    assert gradcheck(lambda m, s, t, v: tuple(refine.split_gaussians(m, s, t, v, split, keep, mode="clone"))[:4],
                     var(means, scaling, transforms, values))
    assert gradcheck(lambda m, v: tuple(refine.split_gaussians(m, scaling, transforms, v, split, keep))[:4], var(means, values))
    assert gradcheck(lambda s, t: tuple(refine.split_gaussians(means, s, t, values, split, keep, value_scale=0.3))[1:4],
                     var(scaling, transforms))


# ---- the C ABI directly -------------------------------------------------------------------------------------
def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_c_abi_truncation_canaries_null_keep_and_short_workspace(refine, hip_lib):
    N, c, CANARY = 3000, 2, 777.0
    arrays = [a.astype(np.float32) for a in family(N, c, 31)]
    _, split = random_masks(N, 0.3, 0.0, 31)
    o = refine_oracle(*arrays, None, split)
    means, scaling, transforms, values = (dev(a) for a in arrays)
    transforms = transforms.reshape(N).contiguous()
    d_split = dev(split)
    need = hip_lib.pigs_refine_workspace_bytes(N)
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    kept_pos, child_pos = (torch.full((N,), -5, dtype=torch.int64, device="cuda") for _ in range(2))
    counts = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (0, N, None, ptr(d_split), ptr(ws))                    # a null keep: all rows kept
    assert hip_lib.pigs_refine_index(*args, need - 1, ptr(kept_pos), ptr(child_pos), ptr(counts), stream) == 4
    torch.cuda.synchronize()
    assert (kept_pos == -5).all() and (counts == -5).all()        # refused: nothing was launched
    assert hip_lib.pigs_refine_index(*args, need, ptr(kept_pos), ptr(child_pos), ptr(counts), stream) == 0
    assert counts.tolist() == [o.n_kept, o.n_split] == [N, int(split.sum())]
    truth = o.n_kept + o.n_split
    for rows in (truth, truth - 1, truth - 2 * o.n_split - 1, 1):  # ends inside a pair, inside the kept rows, at once
        outs = [torch.full((truth + 1,) + s, CANARY, dtype=torch.float32, device="cuda") for s in ((2,), (2,), (), (c,))]
        source = torch.full((truth + 1,), -7, dtype=torch.int64, device="cuda")
        child = torch.full((truth + 1,), -7, dtype=torch.int32, device="cuda")
        rc = hip_lib.pigs_refine_apply(0, 0, c, N, rows, 0.5, ptr(kept_pos), ptr(child_pos), ptr(means), ptr(scaling),
                                       ptr(transforms), ptr(values), *[ptr(t) for t in outs], ptr(source), ptr(child), stream)
        assert rc == 0
        assert all((t[rows:] == CANARY).all() for t in outs) and (source[rows:] == -7).all() and (child[rows:] == -7).all()
        assert np.array_equal(host(source[:rows]), o.source[:rows]) and np.array_equal(host(child[:rows]), o.child[:rows])
        assert torch.equal(outs[1][:rows], scaling.index_select(0, source[:rows]))
        assert not (outs[0][:rows] == CANARY).any() and not (outs[3][:rows] == CANARY).any()
    # the backward with a short `rows` reads nothing behind it: the rows behind count as zero
    rows = truth - 3
    g_out = normal_range((rows, c), torch.float32, 2)
    g_values = torch.full((N, c), CANARY, dtype=torch.float32, device="cuda")
    rc = hip_lib.pigs_refine_backward(0, 0, c, N, rows, 0.5, ptr(kept_pos), ptr(child_pos), None, None, None, ptr(g_out),
                                      None, None, None, ptr(g_values), stream)
    assert rc == 0
    src = dev(o.source[:rows])
    factor = dev(np.where(o.child[:rows] >= 0, 0.5, 1.0), torch.float32)[:, None]
    assert torch.equal(g_values, torch.zeros(N, c, device="cuda").index_add_(0, src, g_out * factor))


# ---- end to end ---------------------------------------------------------------------------------------------
def rel(a, b):
    a = host(a)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def test_model_forward_split_recipe(refine, hip_lib):
    """INTEGRATION.md, 'Model.forward(split=True)': prune (:703-714) and split (:764) as two calls, boundaries and
    boundary_mask through source / child, then build_covariances -- through preprocess / sample_gaussians."""
    from diff_gaussian_sampling import GaussianSampler
    from oracle import covariances_numpy, dense_numpy
    from pigs_amd.covariances import build_covariances
    N, c = 400, 2
    rng = np.random.default_rng(41)
    means = dev(rng.uniform(-1, 1, (N, 2)), torch.float32)
    scaling = dev(np.exp(rng.uniform(np.log(2e-3), np.log(2e-2), (N, 2))), torch.float32)
    transforms = dev(0.5 * rng.standard_normal((N, 1)), torch.float32)
    u = dev(rng.standard_normal((N, c)) * (rng.random((N, 1)) > 0.1), torch.float32)      # a tenth of the rows is empty
    boundary_mask = dev(rng.random((N, 1)) > 0.1)
    boundaries = dev(rng.random((N, 1)), torch.float32) * ~boundary_mask
    samples = dev(rng.uniform(-1, 1, (700, 2)), torch.float32)
    sampler = GaussianSampler(True)

    def field(m, s, t, v, at):
        cov, con = build_covariances(s, t)
        sampler.preprocess(m, v, cov, con, at)
        return sampler.sample_gaussians()

    # the prune
    keep = (torch.norm(torch.abs(u), dim=-1) > 0.01) | ~boundary_mask.squeeze(-1)
    assert 0 < int((~keep).sum()) < N
    p = refine.split_gaussians(means, scaling, transforms, u, None, keep)
    boundary_mask, boundaries = boundary_mask.index_select(0, p.source), boundaries.index_select(0, p.source)
    assert torch.equal(p.means, means[keep])
    assert (p.child == -1).all() and p.means.shape[0] == int(keep.sum())
    # the split (the criterion is not this library's: any mask over the kept rows)
    metric = field(p.means, p.scaling, p.transforms, p.values, p.means).abs().amax(-1)
    indices = (metric > torch.quantile(metric, 0.9)) & boundary_mask.squeeze(-1)
    n = int(indices.sum())
    assert n > 5
    r = refine.split_gaussians(p.means, p.scaling, p.transforms, p.values, indices)
    is_child = (r.child >= 0)[:, None]
    new_boundaries = torch.where(is_child, torch.zeros_like(boundaries[:1]), boundaries.index_select(0, r.source))
    new_mask = torch.where(is_child, torch.ones_like(boundary_mask[:1]), boundary_mask.index_select(0, r.source))
    assert r.means.shape[0] == p.means.shape[0] + n == new_mask.shape[0] == new_boundaries.shape[0]
    assert torch.equal(new_boundaries, torch.cat((boundaries[~indices], torch.zeros(2 * n, 1, device="cuda"))))   # :602-605
    assert torch.equal(new_mask, torch.cat((boundary_mask[~indices], torch.ones(2 * n, 1, dtype=torch.bool, device="cuda"))))
    # (b) the refined field is the dense float64 oracle's on the refined arrays
    got = field(r.means, r.scaling, r.transforms, r.values, samples)
    _, conics = covariances_numpy.build_covariances(host(r.scaling), host(r.transforms))
    full = np.stack((conics[:, 0], conics[:, 1], conics[:, 1], conics[:, 2]), -1).reshape(-1, 2, 2)
    want = dense_numpy.forward(host(r.means), full, host(r.values), host(samples), orders=(0,))[0]
    assert rel(got, want) < 1e-5
    # (a) a child with value_scale = 1 is its parent moved by -/+ e: its field at x is the parent's at x +/- e, which
    # tends to the parent's own field with e -> 0
    one = torch.zeros_like(indices)
    one[int(indices.nonzero()[0])] = True
    w = refine.split_gaussians(p.means, p.scaling, p.transforms, p.values, one, one, value_scale=1.0)
    assert w.child.tolist() == [0, 1]
    parent = [a[one] for a in (p.means, p.scaling, p.transforms, p.values)]
    e = 0.5 * (w.means[1] - w.means[0])
    conic_norm = 1.0 / np.linalg.eigvalsh(covariance_matrices(host(parent[1]), host(parent[2])[:, 0]))[0, 0]
    near = parent[0] + 0.1 * dev(rng.standard_normal((300, 2)), torch.float32)
    for k, sign in ((0, 1.0), (1, -1.0)):
        child_field = field(w.means[k:k + 1], w.scaling[k:k + 1], w.transforms[k:k + 1], w.values[k:k + 1], near)
        parent_field = field(*parent, near + sign * e)
        # the two sides round mu - e and x + e separately, so their offsets x - mu differ by dx <= 4 eps (coordinates
        # below 2, three roundings).  |d exp(-q/2)| <= sqrt(q) exp(-q/2) sqrt(|conic|) dx <= 0.61 sqrt(|conic|) dx, on
        # top of the suite's float32 bar for each evaluation; relative to the parent's largest value
        bound = 1e-5 + 0.61 * np.sqrt(conic_norm) * 4 * np.finfo(np.float32).eps
        err = np.abs(host(child_field) - host(parent_field)).max() / np.abs(host(parent[3])).max()
        print(f"child {k}: {err:.3g} (bound {bound:.3g})")
        assert err <= bound


def test_densification_recipe_with_adam(refine):
    """INTEGRATION.md, the densification block of test_no_mlp.py:198-240 with a real torch.optim.Adam"""
    N, c = 300, 2
    arrays = family(N, c, 51)
    names = ("means", "values", "scaling", "transform")
    params = {n: torch.nn.Parameter(dev(a, torch.float32)) for n, a in
              zip(names, (arrays[0], arrays[3], np.log(arrays[1]), arrays[2]))}
    optim = torch.optim.Adam([{"params": [params[n]], "name": n} for n in names], lr=1e-3)

    def step():
        loss = sum((p ** 2).sum() for g in optim.param_groups for p in g["params"])
        loss.backward()
        optim.step()
        optim.zero_grad()
    step()
    keep_mask, split_indices = (dev(m) for m in random_masks(N, 0.1, 0.2, 51))
    split_indices = split_indices & keep_mask
    with torch.no_grad():
        out = refine.split_gaussians(params["means"], torch.exp(params["scaling"]), params["transform"], params["values"],
                                     split_indices, keep_mask, mode="clone")
        rows = out.source.shape[0]
        assert rows == int(keep_mask.sum()) + int(split_indices.sum())
        fresh = (out.child >= 0)[:, None]
        before = {}
        for group in optim.param_groups:
            old = group["params"][0]
            state = optim.state.pop(old)
            before[group["name"]] = (old.detach().clone(), state["exp_avg"].clone(), state["exp_avg_sq"].clone())
            for key in ("exp_avg", "exp_avg_sq"):
                carried = state[key].index_select(0, out.source)
                state[key] = torch.where(fresh, torch.zeros_like(carried), carried)
            group["params"][0] = torch.nn.Parameter(old.index_select(0, out.source))
            optim.state[group["params"][0]] = state
    kept = out.child < 0
    for group in optim.param_groups:
        p, state = group["params"][0], optim.state[group["params"][0]]
        old, avg, sq = before[group["name"]]
        assert p.shape[0] == rows and state["exp_avg"].shape == p.shape and state["exp_avg_sq"].shape == p.shape
        # test_no_mlp.py:222-233, line for line
        assert torch.equal(p, torch.cat((old[keep_mask], old[split_indices])))
        assert torch.equal(state["exp_avg"][kept], avg[keep_mask]) and torch.equal(state["exp_avg_sq"][kept], sq[keep_mask])
        assert (state["exp_avg"][~kept] == 0).all() and (state["exp_avg_sq"][~kept] == 0).all()
    assert torch.equal(out.means, optim.param_groups[0]["params"][0]) and torch.equal(out.values, optim.param_groups[1]["params"][0])
    step()
    assert all(torch.isfinite(g["params"][0]).all() and g["params"][0].shape[0] == rows for g in optim.param_groups)
