"""GPU: advance_gaussians (pigs_amd/advance.py, csrc/advance.hip) against the float64 checker of tests/test_advance.py.

Bars, the project's own:
    float64   outputs and gradients within 1e-11 of each tensor's scale (its largest magnitude) of the checker (the bar of
              tests/test_optim_gpu.py).
    float32   within 1e-5 of each tensor's scale of the checker applied to the float32 inputs promoted; the conics also
              element-wise, 1e-5 (1e-4 in the family whose transforms' reach +-6: the bars of tests/test_covariances.py).
    exact     means', u' and transforms' are torch's ``x + delta * m`` on the GPU bit for bit (means' after torch's
              ``where`` wrap); covariances / conics are ``build_covariances(out.scaling, out.transforms)`` bit for bit; the
              full forms are the flat ones entry by entry; a boundary row is its input bit for bit.
    penalty   within 4 ulp of the dtype of the checker's exactly rounded value, and the same bits over three calls.
Sizes sit at the kernel's edges: one row, both sides of a workgroup boundary (255, 256, 257), the model's 1 600, 4 097.
Each check prints its figure in units of its bar.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_advance import (INPUTS, MASKS, OUTPUTS, checker_backward, checker_forward, make_case, make_gout, scale_of,
                          torch_forward, wrap_targets)

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}
BAR = {torch.float32: 1e-5, torch.float64: 1e-11}
SIZES = (1, 255, 256, 257, 1600, 4097)
DTYPES = (torch.float32, torch.float64)


@pytest.fixture(scope="module")
def adv(hip_lib):
    assert torch.cuda.is_available()
    import pigs_amd
    return pigs_amd.advance_gaussians


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().double().numpy()


def leaves_of(case, dtype, requires=(True,) * 5):
    return [dev(case[k], dtype).requires_grad_(r) for k, r in zip(INPUTS, requires)]


def incoming(gout, outs, dtype):
    """the incoming gradients rounded to the dtype, as the kernel and the checker both see them"""
    g = {k: None if v is None else v.astype(NP[dtype]).astype(np.float64) for k, v in gout.items()}
    loss = None
    for o, name in zip(outs, OUTPUTS):
        if g[name] is not None:
            term = (o * dev(g[name], dtype).reshape(o.shape)).sum()
            loss = term if loss is None else loss + term
    return g, loss


def assert_close(what, got, want, bar):
    got = host(got).reshape(want.shape) if isinstance(got, torch.Tensor) else got
    assert np.isfinite(got).all(), f"{what}: not finite"
    fig = float(np.abs(got - want).max()) / (bar * scale_of(want)) if want.size else 0.0
    assert fig <= 1.0, f"{what}: {fig:.3g} x its bar ({bar:g} of the tensor's scale)"
    return fig


def assert_penalty(what, got, want, dtype):
    got = host(got)
    if np.isnan(want).all():
        assert np.isnan(got).all(), (what, got)
        return 0.0
    ulp = np.spacing(np.abs(want).astype(NP[dtype])).astype(np.float64)
    fig = float((np.abs(got - want) / (4.0 * ulp)).max())
    assert fig <= 1.0, f"{what}: penalty {fig:.3g} x its bar (4 ulp): {got} vs {want}"
    return fig


def run_case(adv, what, case, dtype, present=OUTPUTS, requires=(True,) * 5, conic_bar=1e-5, nan_deltas=False):
    """one forward and one backward on the GPU, everything held to its bar; returns (out, grads)"""
    leaves = leaves_of(case, dtype, requires)
    mask = dev(case["mask"], torch.bool)
    out = adv(*leaves, mask, wrap=case["wrap"])
    want = checker_forward(case)
    worst = 0.0
    for name, o in zip(OUTPUTS[:-1], out):
        worst = max(worst, assert_close(f"{what} {name}", o, want[name], BAR[dtype]))
    if dtype == torch.float32:
        fig = float(np.abs(host(out.conics) / want["conics"] - 1.0).max()) / conic_bar
        worst = max(worst, fig)
        assert fig <= 1.0, f"{what} conics, element-wise: {fig:.3g} x its bar ({conic_bar:g})"
    worst = max(worst, assert_penalty(what, out.penalty, want["penalty"], dtype))
    for _ in range(2):                                            # three calls, the same bits
        again = adv(*leaves, mask, wrap=case["wrap"])
        assert torch.equal(again.penalty.view(torch.uint8), out.penalty.view(torch.uint8)), what

    # exact: torch's own x + delta * m on the GPU (the deltas of boundary rows taken as zero where they hold NaN / Inf)
    means, u, scaling, transforms, deltas = (t.detach() for t in leaves)
    m = mask[:, None].to(dtype)
    d = torch.where(mask[:, None], deltas, torch.zeros_like(deltas)) if nan_deltas else deltas
    c = case["c"]
    ref_means = means + d[:, 0:2] * m
    if case["wrap"] is not None:
        lo, hi = case["wrap"]
        ref_means = torch.where(ref_means > hi, ref_means - (hi - lo), ref_means)
        ref_means = torch.where(ref_means < lo, ref_means + (hi - lo), ref_means)
    assert torch.equal(out.means, ref_means), f"{what}: means' is not torch's x + delta m"
    assert torch.equal(out.u, u + d[:, 5:5 + c] * m) and torch.equal(out.transforms, transforms + d[:, 4:5] * m), what
    from pigs_amd import covariances
    cov, con = covariances.build_covariances(out.scaling.detach(), out.transforms.detach())
    assert torch.equal(out.covariances, cov) and torch.equal(out.conics, con), f"{what}: not build_covariances' bits"
    for full, flat in ((out.full_covariances, out.covariances), (out.full_conics, out.conics)):
        assert full.shape == (case["N"], 2, 2)
        assert torch.equal(full.reshape(-1, 4), flat[:, [0, 1, 1, 2]]), f"{what}: full forms differ from the flat ones"
    bound = ~mask
    for o, x in zip(out[:4], (means, u, scaling, transforms)):
        assert torch.equal(o[bound], x[bound]), f"{what}: a boundary row moved"

    wanted = [t for t in leaves if t.requires_grad]
    gout, loss = incoming(make_gout(case, seed=case["N"] + 31 * c, present=present), out, dtype)
    got = dict(zip([k for k, r in zip(INPUTS, requires) if r], torch.autograd.grad(loss, wanted, allow_unused=True)))
    grads = checker_backward(case, want, gout)
    for name in got:
        assert got[name] is not None and got[name].shape == case[name].shape, (what, name)
        worst = max(worst, assert_close(f"{what} d {name}", got[name], grads[name], BAR[dtype]))
    if "deltas" in got:
        assert not got["deltas"][bound].any(), f"{what}: a boundary row's deltas received a gradient"
    print(f"[figure] {what} {str(dtype)[6:]} N={case['N']} c={c}: worst {worst:.3g} x its bar")
    return out, got


# ---- sizes x masks: every N, every c and both dtypes with every mask family ---------------------------------
@pytest.mark.parametrize("k", range(len(SIZES)), ids=[f"N{n}" for n in SIZES])
@pytest.mark.parametrize("mask", MASKS)
def test_sizes_and_masks(adv, mask, k):
    """six cases per mask family: N runs through SIZES, c through 1, 2, 3, 4, 1, 2, the dtype alternates (starting with
    a different one per family); wrap (-1, 1) on every other case"""
    N, c = SIZES[k], (1, 2, 3, 4, 1, 2)[k]
    dtype = DTYPES[(k + MASKS.index(mask)) % 2]
    case = make_case(N, c, seed=100 + k, mask=mask, wrap=(-1.0, 1.0) if k % 2 else None, dtype=NP[dtype])
    out, grads = run_case(adv, f"sizes x masks, {mask}", case, dtype)
    if mask == "none" or not case["mask"].any():
        assert torch.isnan(out.penalty).all()
        for name in ("means", "u", "scaling", "transforms"):
            assert torch.equal(getattr(out, name), dev(case[name], dtype)), name
        assert not grads["deltas"].any()                          # and the state gradients are the pass-through ones


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_channel_count_in_both_dtypes(adv, c, dtype):
    run_case(adv, "channels x dtypes", make_case(1600, c, seed=120 + c, mask="prefix", wrap=(-1.0, 1.0), dtype=NP[dtype]), dtype)


def test_no_free_row_gives_zero_gradients(adv):
    """penalty NaN, every other output the input bitwise; a gradient on the NaN penalty too leaves every gradient zero"""
    N, c, dtype = 257, 2, torch.float32
    case = make_case(N, c, seed=130, mask="none", values="naninf", dtype=np.float32)
    leaves, mask = leaves_of(case, dtype), dev(case["mask"], torch.bool)
    out = adv(*leaves, mask)
    assert torch.isnan(out.penalty).all()
    for o, x in zip(out[:4], leaves):
        assert torch.equal(o, x.detach())
    grads = torch.autograd.grad(out.penalty.sum(), leaves, allow_unused=True)
    assert all(g is not None and not g.any() for g in grads)


# ---- value families -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mask", ["all", "prefix", "half"])
def test_transforms_reaching_six(adv, mask, dtype):
    case = make_case(257, 2, seed=140, mask=mask, values="t6", dtype=NP[dtype])
    out, _ = run_case(adv, "transforms' = +-6", case, dtype, conic_bar=1e-4)
    assert float(out.transforms.detach().abs().max()) == 6.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mask", ["all", "prefix", "half"])
def test_dscaling_of_ten(adv, mask, dtype):
    run_case(adv, "dscaling = +-10", make_case(257, 3, seed=141, mask=mask, values="ds10", dtype=NP[dtype]), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mask", ["prefix", "half", "single"])
def test_nan_and_inf_in_the_deltas_of_boundary_rows(adv, mask, dtype):
    """outputs and gradients of EVERY row stay finite (assert_close checks it) and equal to the checker's"""
    case = make_case(257, 2, seed=142, mask=mask, values="naninf", wrap=(-1.0, 1.0), dtype=NP[dtype])
    assert not np.isfinite(case["deltas"][~case["mask"]]).any() and np.isfinite(case["deltas"][case["mask"]]).all()
    run_case(adv, "NaN / Inf on boundary rows", case, dtype, nan_deltas=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("wrap", [(-1.0, 1.0), (-0.5, 1.75)], ids=["box11", "boxother"])
@pytest.mark.parametrize("mask", ["all", "prefix"])
def test_wrap_edges(adv, mask, wrap, dtype):
    """means' planted exactly on lo and hi (stay), one ulp outside each (shift), 1.25 periods outside (ONE shift)"""
    case = make_case(257, 2, seed=143, mask=mask, values="wrap", wrap=wrap, dtype=NP[dtype])
    out, _ = run_case(adv, f"wrap edges {wrap}", case, dtype)
    lo, hi = wrap
    t = wrap_targets(lo, hi, NP[dtype]).astype(np.float64)
    period = hi - lo
    want = np.array([lo, hi, t[2] + period, t[3] - period, lo - 0.25 * period, hi + 0.25 * period])
    rows = np.flatnonzero(case["mask"])[:6]
    got = host(out.means)[rows]
    assert np.array_equal(got[:, 0], want.astype(NP[dtype])) and np.array_equal(got[:, 1], want.astype(NP[dtype])), (got, want)


# ---- gradient subsets ---------------------------------------------------------------------------------------
SUBSETS = {"penalty": ("penalty",), "conics": ("conics",), "full_covariances": ("full_covariances",), "all": OUTPUTS}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("subset", list(SUBSETS))
def test_gradient_subsets(adv, subset, dtype):
    run_case(adv, f"gradient on {subset}", make_case(257, 3, seed=150, mask="half", wrap=(-1.0, 1.0), dtype=NP[dtype]),
             dtype, present=SUBSETS[subset])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("without", ["scaling", "deltas"])
def test_needs_input_grad(adv, without, dtype):
    requires = tuple(k != without for k in INPUTS)
    _, grads = run_case(adv, f"no gradient towards {without}", make_case(257, 2, seed=151, mask="half", dtype=NP[dtype]),
                        dtype, requires=requires)
    assert set(grads) == set(INPUTS) - {without}


def test_nothing_requires_grad_and_flat_transforms(adv):
    case = make_case(257, 1, seed=152, mask="half", dtype=np.float32)
    leaves = leaves_of(case, torch.float32, (False,) * 5)
    mask = dev(case["mask"], torch.bool)
    out = adv(*leaves, mask)
    assert not any(o.requires_grad for o in out)
    flat = adv(leaves[0], leaves[1], leaves[2], leaves[3][:, 0].contiguous(), leaves[4][None], mask[:, None])
    assert flat.transforms.shape == (257,) and torch.equal(flat.transforms, out.transforms[:, 0])
    assert all(torch.equal(a, b) for a, b in zip(flat[4:], out[4:]))
    leaves[4].requires_grad_(True)                                # the gradient keeps the caller's [1, N, 5 + c]
    lead = leaves[4].detach()[None].requires_grad_(True)
    (g,) = torch.autograd.grad(adv(*leaves[:4], lead, mask).penalty.sum(), (lead,))
    assert g.shape == (1, 257, 6)


def test_gradcheck(adv):
    """float64 torch.autograd.gradcheck at N = 7, c = 2, a mixed mask; means' stay away from the wrap edges"""
    case = make_case(7, 2, seed=153, mask="half")
    assert 0 < case["mask"].sum() < 7
    case["means"] = np.random.default_rng(153).uniform(-0.5, 0.5, (7, 2))
    leaves, mask = leaves_of(case, torch.float64), dev(case["mask"], torch.bool)
    assert torch.autograd.gradcheck(lambda *a: tuple(adv(*a, mask, wrap=(-1.0, 1.0))), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- canaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [255, 257])
def test_canaries_after_every_output_the_scratch_and_the_deltas_gradient(hip_lib, N, dtype):
    """through the C ABI with buffers of its own: 64 sentinel elements behind every array the kernels write"""
    c, pad, sentinel = 3, 64, -12345.0
    case = make_case(N, c, seed=160, mask="half", dtype=NP[dtype])
    ins = [dev(case[k], dtype) for k in INPUTS]
    mask = dev(case["mask"], torch.bool).view(torch.uint8)
    code = {torch.float32: 0, torch.float64: 1}[dtype]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def padded(n, dt=dtype):
        return torch.full((n + pad,), sentinel, dtype=dt, device="cuda")

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())
    widths = (2, c, 2, 1, 3, 3, 4, 4)
    outs = [padded(N * w) for w in widths] + [padded(4)]
    nbytes = hip_lib.pigs_advance_scratch_bytes(N)
    scratch = padded(nbytes // 8, torch.float64)
    rc = hip_lib.pigs_advance_forward(code, c, N, 1, -1.0, 1.0, *[ptr(t) for t in ins], ptr(mask), ptr(scratch), nbytes,
                                      *[ptr(o) for o in outs], stream)
    assert rc == 0
    gouts = [dev(np.random.default_rng(161 + k).standard_normal(o.numel() - pad), dtype) for k, o in enumerate(outs)]
    grads = [padded(N * w) for w in (2, c, 2, 1, 5 + c)]
    rc = hip_lib.pigs_advance_backward(code, c, N, ptr(outs[2]), ptr(outs[3]), ptr(ins[4]), ptr(mask), ptr(scratch),
                                       *[ptr(g) for g in gouts], *[ptr(g) for g in grads], stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, t in zip(OUTPUTS + ("scratch",) + tuple("d " + k for k in INPUTS), outs + [scratch] + grads):
        assert (t[-pad:] == sentinel).all(), f"{name}: written past its end"
        assert not (t[:-pad] == sentinel).any(), f"{name}: not all of it was written"
    want = checker_forward(case | {"wrap": (-1.0, 1.0)})
    assert_close("canaries: conics", outs[5][:-pad], want["conics"].reshape(-1), BAR[dtype])
    assert_penalty("canaries", outs[8][:-pad], want["penalty"], dtype)
    assert host(scratch)[4] == case["mask"].sum()                 # n_free stays on the device, in record 0


# ---- capture ------------------------------------------------------------------------------------------------
def test_capture_of_the_operator_and_its_backward(adv):
    """torch.cuda.graph around the operator and autograd.grad; three replays with the inputs rewritten in place, each
    against the checker"""
    N, c, dtype = 1600, 2, torch.float64
    cases = [make_case(N, c, seed=170 + k, mask="half", wrap=(-1.0, 1.0)) for k in range(4)]
    gouts = [make_gout(cases[k], seed=180 + k) for k in range(4)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaves = leaves_of(cases[0], dtype)
        mask = dev(cases[0]["mask"], torch.bool)
        static_g = [dev(gouts[0][k], dtype) for k in OUTPUTS]

        def step():
            out = adv(*leaves, mask, wrap=(-1.0, 1.0))
            loss = sum((o * g).sum() for o, g in zip(out, static_g))
            return out, torch.autograd.grad(loss, leaves)
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, grads = step()
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        with torch.no_grad():
            for leaf, name in zip(leaves, INPUTS):
                leaf.copy_(dev(cases[k][name], dtype))
            mask.copy_(dev(cases[k]["mask"], torch.bool))
            for s, name in zip(static_g, OUTPUTS):
                s.copy_(dev(gouts[k][name], dtype))
        graph.replay()
        torch.cuda.synchronize()
        want = checker_forward(cases[k])
        for name, o in zip(OUTPUTS[:-1], out):
            assert_close(f"replay {k} {name}", o, want[name], 1e-11)
        assert_penalty(f"replay {k}", out.penalty, want["penalty"], dtype)
        for name, g in zip(INPUTS, grads):
            assert_close(f"replay {k} d {name}", g, checker_backward(cases[k], want, gouts[k])[name], 1e-11)


def test_capture_inside_a_graphed_step(adv):
    """GraphedStep over advance_gaussians -> preprocess -> sample((0, 1, 2)) -> loss + penalty -> backward at N = 1 600:
    three replays with new deltas against the same step run eagerly, 1e-4 of each tensor's scale (float32 sums of
    1 024 x 1 600 pairs in two launch orders; the operator's own bars are held above)"""
    from diff_gaussian_sampling import GaussianSampler
    from pigs_amd.graphs import GraphedStep
    N, c, M, dtype = 1600, 1, 1024, torch.float32
    cases = [make_case(N, c, seed=190 + k, mask="prefix", wrap=(-1.0, 1.0), dtype=np.float32) for k in range(4)]
    for case in cases:
        case["scaling"] = np.full((N, 2), np.exp(-5.0)).astype(np.float32).astype(np.float64)
    samples = np.random.default_rng(191).uniform(-1.0, 1.0, (M, 2))
    weights = torch.tensor([1.0, 0.5, 0.25, 2.0], device="cuda")

    def step_of(sampler):
        def fn(means, u, scaling, transforms, deltas, mask, pts):
            out = adv(means, u, scaling, transforms, deltas, mask, wrap=(-1.0, 1.0))
            sampler.preprocess(out.means, out.u, out.covariances, out.conics, pts)
            f, fx, fxx = sampler.sample((0, 1, 2))
            loss = torch.mean(f ** 2) + 1e-3 * torch.mean(fx ** 2) + 1e-6 * torch.mean(fxx ** 2) + (out.penalty * weights).sum()
            return (loss.detach(),) + torch.autograd.grad(loss, (means, u, scaling, transforms, deltas))
        return fn

    def inputs_of(case):
        return leaves_of(case, dtype) + [dev(case["mask"], torch.bool), dev(samples, dtype)]
    eager_fn = step_of(GaussianSampler(False))
    holder = {}

    def make_inputs():
        holder["fn"] = step_of(GaussianSampler(False))
        return inputs_of(cases[0])
    step = GraphedStep(lambda *a: holder["fn"](*a), make_inputs, warmup=2)
    for k in (1, 2, 3):
        with torch.no_grad():
            step.inputs[4].copy_(dev(cases[k]["deltas"], dtype))
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        eager = eager_fn(*inputs_of(dict(cases[0], deltas=cases[k]["deltas"])))
        for name, g, e in zip(("loss",) + INPUTS, got, eager):
            assert_close(f"graphed step, replay {k}, {name}", g, host(e), 1e-4)
        assert float(got[0]) > 0 and got[5].abs().max() > 0


# ---- end to end ---------------------------------------------------------------------------------------------
def test_five_chained_steps_against_the_torch_composition(adv):
    """N = 400, c = 2, wrap (-1, 1), float64: deltas from a fixed small nn.Linear on the state, the state re-fed, the
    loss backpropagated through all five steps at once; outputs and the layer's gradient at 1e-11 of scale"""
    N, c, dtype = 400, 2, torch.float64
    case = make_case(N, c, seed=200, mask="prefix", wrap=(-1.0, 1.0))
    torch.manual_seed(200)
    layer = torch.nn.Linear(5 + c, 5 + c).to("cuda", dtype)
    with torch.no_grad():
        layer.weight.mul_(0.2)
        layer.bias.mul_(0.05)
    mask = dev(case["mask"], torch.bool)
    rng = np.random.default_rng(201)
    w = {name: dev(rng.standard_normal(s), dtype) for name, s in
         (("means", (N, 2)), ("u", (N, c)), ("conics", (N, 3)), ("full_covariances", (N, 2, 2)))}

    def chain(op):
        state = [dev(case[k], dtype) for k in INPUTS[:4]]
        loss, last = 0.0, None
        for _ in range(5):
            deltas = layer(torch.cat(state, dim=-1))
            out = op(*state, deltas)
            named = dict(zip(OUTPUTS, out))
            loss = loss + sum((named[k] * w[k]).sum() for k in w) * 1e-3 + named["penalty"].sum()
            state, last = list(out[:4]), out
        grads = torch.autograd.grad(loss, (layer.weight, layer.bias))
        return [loss.detach()] + [t.detach() for t in last] + list(grads)
    got = chain(lambda *a: adv(*a, mask, wrap=(-1.0, 1.0)))
    want = chain(lambda *a: torch_forward(*a, mask, wrap=(-1.0, 1.0)))
    worst = 0.0
    for name, g, e in zip(("loss",) + OUTPUTS + ("d weight", "d bias"), got, want):
        worst = max(worst, assert_close(f"five steps, {name}", g, host(e), 1e-11))
    print(f"[figure] five chained steps: worst {worst:.3g} x its bar")
