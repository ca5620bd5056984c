"""GPU: state_loss_terms (pigs_amd/state_loss.py, csrc/state_loss.hip) against the float64 checker of
tests/test_state_loss.py and against the reference's recorded ``compute_loss`` of Problem.TEST.

Bars, the project's own (tests/test_advance_gpu.py):
    gradients  within 1e-5 (float32) / 1e-11 (float64) of each tensor's scale (its largest magnitude) of the checker
               evaluated on the same inputs; every entry of a boundary row an exact zero.
    terms      within 4 ulp of the dtype of the checker's value, whose sums are exactly rounded; the same NaN pattern; an
               entry the checker has at zero (an empty set) is an exact zero; the same bits over three calls.
    recorded   the three losses composed from the operator's terms and the six gradients behind ``prev + delta * mask``
               within 1e-11 of each recorded number's scale (a loss is a weighted sum of at most five terms, each held to
               4 ulp above).
Sizes sit at the kernel's edges: one row, both sides of a wave (63, 64, 65), the 256-thread and the 1 024-thread
workgroup (257, 1 025), the one-launch bound and the first size that takes two launches (4 096, 4 097).
Each check prints its figure in units of its bar.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_advance import MASKS, scale_of
from test_advance import torch_forward as advance_torch
from test_state_loss import (COLUMNS, INPUTS, RECORDED_GRADS, SCENES, WEIGHTS, checker_grads, checker_terms,
                             compose_losses, make_case, make_g, masked_penalty, scene_losses, state_loss_recipe, statistics)

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}
BAR = {torch.float32: 1e-5, torch.float64: 1e-11}
DTYPES = (torch.float32, torch.float64)
BOUND = 4096                                     # PIGS_STATE_LOSS_ONE_LAUNCH_ROWS (tests/test_state_loss.py reads the header)
SIZES = (1, 63, 64, 65, 257, 1025, BOUND, BOUND + 1)


@pytest.fixture(scope="module")
def op(hip_lib):
    assert torch.cuda.is_available()
    import pigs_amd
    return pigs_amd.state_loss_terms


def dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().double().numpy()


def leaves_of(case, dtype, requires=(True,) * 3):
    return [dev(case[k], dtype).requires_grad_(r) for k, r in zip(INPUTS, requires)]


def assert_close(what, got, want, bar):
    got = host(got).reshape(want.shape) if isinstance(got, torch.Tensor) else got
    assert np.isfinite(got).all(), f"{what}: not finite"
    fig = float(np.abs(got - want).max()) / (bar * scale_of(want)) if want.size else 0.0
    assert fig <= 1.0, f"{what}: {fig:.3g} x its bar ({bar:g} of the tensor's scale)"
    return fig


def assert_terms(what, got, want, dtype):
    got = host(got)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern {got} vs {want}"
    ok = ~np.isnan(want)
    ulp = np.spacing(np.abs(want[ok]).astype(NP[dtype])).astype(np.float64)
    figs = np.abs(got[ok] - want[ok]) / (4.0 * ulp)
    fig = float(figs.max()) if figs.size else 0.0
    assert fig <= 1.0, f"{what}: terms {figs} x their bar (4 ulp): {got} vs {want}"
    return fig


def run_case(op, what, case, dtype, requires=(True,) * 3, g=None, shapes=False):
    """one forward (three calls, the same bits) and one backward on the GPU, everything held to its bar"""
    leaves = leaves_of(case, dtype, requires)
    mask = dev(case["mask"], torch.bool)
    if shapes:                                   # the other two shapes the interface takes
        leaves[2] = leaves[2].detach()[None].requires_grad_(requires[2])
        mask = mask[:, None]
    terms = op(*leaves, mask, wall=case["wall"], drift=case["drift"])
    assert terms.shape == (len(COLUMNS),) and terms.dtype == dtype
    want = checker_terms(case)
    worst = assert_terms(what, terms, want, dtype)
    for _ in range(2):
        again = op(*leaves, mask, wall=case["wall"], drift=case["drift"])
        assert torch.equal(again.view(torch.uint8), terms.view(torch.uint8)), f"{what}: the bits changed between calls"
    if not any(requires):
        assert not terms.requires_grad
        return terms, {}
    g = make_g(case["N"] + 31 * case["c"], NP[dtype]) if g is None else g
    wanted = [t for t in leaves if t.requires_grad]
    got = dict(zip([k for k, r in zip(INPUTS, requires) if r],
                   torch.autograd.grad((terms * dev(g, dtype)).sum(), wanted, allow_unused=True)))
    grads = checker_grads(case, g)
    bound = ~dev(case["mask"], torch.bool)
    for name, leaf in zip([k for k, r in zip(INPUTS, requires) if r], wanted):
        assert got[name] is not None and got[name].shape == leaf.shape, (what, name)
        flat = got[name].reshape(case[name].shape)
        worst = max(worst, assert_close(f"{what} d {name}", flat, grads[name], BAR[dtype]))
        assert not flat[bound].any(), f"{what}: a boundary row's {name} received a gradient"
    if "deltas" in got:
        assert not got["deltas"].reshape(case["deltas"].shape)[:, 2:5].any(), f"{what}: dscaling / dtransforms moved"
    print(f"[figure] {what} {str(dtype)[6:]} N={case['N']} c={case['c']}: worst {worst:.3g} x its bar")
    return terms, got


# ---- the recorded scenes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SCENES)), ids=[f"{k}-{s['kind']}" for k, s in enumerate(SCENES)])
def test_recorded_compute_loss(op, k):
    """float64: the reference's own pde_loss, bc_loss, conservation_loss and gradients from the operator's terms"""
    scene = SCENES[k]
    got = scene_losses(scene, lambda means, u, deltas, mask: op(means, u, deltas, mask), device="cuda")
    worst = 0.0
    for name in ("pde_loss", "bc_loss", "conservation_loss") + RECORDED_GRADS:
        worst = max(worst, assert_close(f"scene {k} ({scene['kind']}) {name}", got[name], scene[name], 1e-11))
    case = {"means": scene["means"], "u": scene["u"], "deltas": scene["deltas"], "mask": scene["boundary_mask"], "c": 1,
            "N": 56, "dtype": np.float64, "wall": 0.8, "drift": 5.0}
    terms, _ = run_case(op, f"scene {k} ({scene['kind']})", case, torch.float64)
    low, high, mid = (int(v) for v in scene["counts"])
    assert [bool(terms[1] != 0), bool(terms[2] != 0), bool(terms[6] != 0)] == [low > 0, high > 0, mid > 0]
    print(f"[figure] scene {k} ({scene['kind']}) against the recorded numbers: worst {worst:.3g} x its bar")


# ---- sizes x masks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SIZES)), ids=[f"N{n}" for n in SIZES])
@pytest.mark.parametrize("mask", MASKS)
def test_sizes_and_masks(op, mask, k):
    """eight sizes per mask family: c runs through 1..4 twice, the dtype alternates (starting with a different one per
    family); every other case hands over deltas [1, N, 5 + c] and a mask [N, 1]"""
    N, c = SIZES[k], 1 + k % 4
    dtype = DTYPES[(k + MASKS.index(mask)) % 2]
    case = make_case(N, c, seed=100 + k, mask=mask, dtype=NP[dtype])
    terms, grads = run_case(op, f"sizes x masks, {mask}", case, dtype, shapes=bool(k % 2))
    if not case["mask"].any():
        assert torch.isnan(terms).tolist() == [True, False, False, True, True, True, False, False]
        assert all(not g.any() for g in grads.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_channel_count_in_both_dtypes(op, c, dtype):
    run_case(op, "channels x dtypes", make_case(1600, c, seed=120 + c, mask="prefix", dtype=NP[dtype]), dtype)


# ---- sets and edge values -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("heights", ["nolow", "nohigh", "nomid"])
def test_an_empty_set_gives_zero_terms_and_zero_gradients(op, heights, dtype):
    case = make_case(257, 3, seed=130, mask="half", heights=heights, dtype=NP[dtype])
    empty = {"nolow": [1], "nohigh": [2], "nomid": [6, 7]}[heights]
    terms, _ = run_case(op, f"empty set, {heights}", case, dtype)
    assert not terms[empty].any() and torch.isfinite(terms).all()
    g = np.zeros(8)
    g[empty] = 1.5                               # a gradient on the empty set's terms alone: exact zeros everywhere
    _, grads = run_case(op, f"empty set, {heights}, gradient on its terms", case, dtype, g=g)
    assert all(torch.isfinite(v).all() and not v.any() for v in grads.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_no_free_row(op, dtype):
    """the NaN pattern of torch.mean of nothing, zeros in the conditional entries, every gradient an exact zero"""
    case = make_case(257, 2, seed=131, mask="none", values="naninf", dtype=NP[dtype])
    terms, grads = run_case(op, "no free row", case, dtype)
    assert torch.isnan(terms).tolist() == [True, False, False, True, True, True, False, False]
    assert not terms[[1, 2, 6, 7]].any()
    assert len(grads) == 3 and all(not g.any() for g in grads.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mask", ["all", "prefix"])
def test_heights_at_the_walls(op, mask, dtype):
    """free rows at exactly -wall and +wall (in no set) and one ulp either side of each, in the dtype"""
    case = make_case(64, 2, seed=132, mask=mask, values="walls", dtype=NP[dtype])
    s = statistics(case)
    rows = np.flatnonzero(case["mask"])[:6]
    assert [int(s[k][rows].sum()) for k in ("low", "high", "mid")] == [1, 1, 2]
    run_case(op, "heights at the walls", case, dtype)
    # each planted row carries its set: moved one ulp across the wall, it moves the terms of the sets it leaves and joins
    on_wall = dict(case, means=case["means"].copy())
    on_wall["means"][rows[2:], 1] = np.array([-1.0, -1.0, 1.0, 1.0]) * float(NP[dtype](0.8))
    a = op(*leaves_of(case, dtype), dev(case["mask"], torch.bool))
    b = op(*leaves_of(on_wall, dtype), dev(case["mask"], torch.bool))
    assert all(bool(a[j] != b[j]) for j in (1, 2, 6, 7))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mask", ["prefix", "half", "single"])
def test_nan_and_inf_on_boundary_rows(op, mask, dtype):
    """NaN / Inf in the state and the deltas of every boundary row: terms and gradients finite and the checker's"""
    case = make_case(257, 2, seed=133, mask=mask, values="naninf", dtype=NP[dtype])
    bound = ~case["mask"]
    assert all(not np.isfinite(case[k][bound]).any() and np.isfinite(case[k][~bound]).all() for k in INPUTS)
    terms, _ = run_case(op, "NaN / Inf on boundary rows", case, dtype)
    assert torch.isfinite(terms).all()


# ---- centring, float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [257, BOUND + 1], ids=["one-launch", "two-launches"])
def test_equal_heights_have_no_spread(op, N):
    """every free height 0.37: height_spread <= (2 ulp x 0.37)^2 and its gradient <= 2 ulp x 0.37 x 2 |g5| / F, with
    ulp = 2^-52.  sum y^2 - (sum y)^2 / F errs by about 1e-16 x 0.37^2 x F here and fails both."""
    case = make_case(N, 1, seed=140, mask="half", values="equal")
    F, eps = int(case["mask"].sum()), 2.0 ** -52
    leaves, mask = leaves_of(case, torch.float64), dev(case["mask"], torch.bool)
    terms = op(*leaves, mask)
    spread, bar = float(terms[5].detach()), (2.0 * eps * 0.37) ** 2
    print(f"[figure] equal heights N={N}: height_spread {spread:.3g}, {spread / bar:.3g} x its bar")
    assert 0.0 <= spread <= bar
    g5 = 3.0
    (g_means,) = torch.autograd.grad(terms[5] * g5, leaves[:1])
    worst, bar = float(g_means.abs().max()), 2.0 * eps * 0.37 * 2.0 * g5 / F
    print(f"[figure] equal heights N={N}: d means {worst:.3g}, {worst / bar:.3g} x its bar")
    assert worst <= bar


@pytest.mark.parametrize("N", [257, BOUND + 1], ids=["one-launch", "two-launches"])
def test_offset_dmeans_keep_the_ordinary_bars(op, N):
    """dmeans = 100 + 1e-3 x normal: dmeans_spread is 1e-6 beside squares of 1e4.  4 ulp and 1e-11 of scale as ever; an
    uncentred sum errs by about 1e-16 x 1e4 on a value of 1e-6."""
    case = make_case(N, 2, seed=141, mask="half", values="offset")
    terms, _ = run_case(op, "offset dmeans", case, torch.float64)
    assert 2e-7 < float(terms[4]) < 5e-6
    g = np.zeros(8)
    g[4] = 1.0                                   # the spread's gradient alone: its own scale, not that of 2 g3 dx / F
    run_case(op, "offset dmeans, the spread's gradient", case, torch.float64, g=g)


# ---- gradient plumbing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("select", [(0,), (1, 2), (3, 4, 5), (6, 7)], ids=lambda s: "+".join(COLUMNS[j] for j in s))
def test_gradient_subsets(op, select, dtype):
    """a loss that uses some of the terms: the incoming gradient is zero elsewhere"""
    case = make_case(257, 3, seed=150, mask="half", dtype=NP[dtype])
    g = np.zeros(8)
    g[list(select)] = make_g(151, NP[dtype])[list(select)]
    run_case(op, f"gradient on {select}", case, dtype, g=g)
    leaves, mask = leaves_of(case, dtype), dev(case["mask"], torch.bool)
    terms = op(*leaves, mask)
    got = torch.autograd.grad(sum(terms[j] * float(g[j]) for j in select), leaves)      # through indexing, not a product
    for name, t in zip(INPUTS, got):
        assert_close(f"indexed terms {select} d {name}", t, checker_grads(case, g)[name], BAR[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("requires", [(True, False, False), (False, True, False), (False, False, True), (True, True, False),
                                      (False, False, False)], ids=["means", "u", "deltas", "means+u", "none"])
def test_needs_input_grad(op, requires, dtype):
    _, grads = run_case(op, f"gradients towards {requires}", make_case(257, 2, seed=152, mask="half", dtype=NP[dtype]),
                        dtype, requires=requires)
    assert set(grads) == {k for k, r in zip(INPUTS, requires) if r}


def test_gradcheck(op):
    """float64 torch.autograd.gradcheck at N = 7, c = 2, a mixed mask; the heights stay 0.05 away from the walls, so
    the sets are constants of the finite differences too"""
    case = make_case(7, 2, seed=153, mask="half")
    case["mask"][:3] = [True, False, True]
    case["means"][:, 1] = [-1.0, -0.9, -0.5, 0.0, 0.3, 0.9, 1.05]
    case["mask"][-1] = True
    s = statistics(case)
    assert all(int(s[k].sum()) > 0 for k in ("low", "high", "mid")) and 0 < case["mask"].sum() < 7
    leaves, mask = leaves_of(case, torch.float64), dev(case["mask"], torch.bool)
    assert torch.autograd.gradcheck(lambda *a: op(*a, mask), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [255, 257, BOUND + 1])
def test_canaries_after_the_terms_the_scratch_and_every_gradient(hip_lib, N, dtype):
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
    terms = padded(8)
    nbytes = hip_lib.pigs_state_loss_scratch_bytes(N)
    scratch = padded(nbytes // 8, torch.float64)
    rc = hip_lib.pigs_state_loss_forward(code, c, N, 0.8, 5.0, *[ptr(t) for t in ins], ptr(mask), ptr(scratch), nbytes,
                                         ptr(terms), stream)
    assert rc == 0
    g = make_g(161, NP[dtype])
    grads = [padded(N * w) for w in (2, c, 5 + c)]
    g_terms = dev(g, dtype)
    rc = hip_lib.pigs_state_loss_backward(code, c, N, 0.8, 5.0, *[ptr(t) for t in ins], ptr(mask), ptr(scratch),
                                          ptr(g_terms), *[ptr(t) for t in grads], stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, t in zip(("terms", "scratch") + tuple("d " + k for k in INPUTS), [terms, scratch] + grads):
        assert (t[-pad:] == sentinel).all(), f"{name}: written past its end"
        assert not (t[:-pad] == sentinel).any(), f"{name}: not all of it was written"
    assert_terms("canaries", terms[:-pad], checker_terms(case), dtype)
    s = statistics(case)
    assert host(scratch)[:4].tolist() == [s["F"]] + [int(s[k].sum()) for k in ("low", "high", "mid")]      # the statistics record
    for name, t in zip(INPUTS, grads):
        assert_close(f"canaries d {name}", t[:-pad], checker_grads(case, g)[name].reshape(-1), BAR[dtype])


# ---- capture ------------------------------------------------------------------------------------------------
def test_capture_of_the_operator_and_its_backward(op):
    """torch.cuda.graph around the operator and autograd.grad; three replays with every input rewritten in place.  From
    one replay to the next rows cross the walls and a set becomes empty (no LOW, then no MID, then no HIGH): a host
    decision baked into the capture would keep the first scene's branches."""
    N, c, dtype = 257, 2, torch.float64
    families = ("all", "nolow", "nomid", "nohigh")
    cases = [make_case(N, c, seed=170 + k, mask="half", heights=h) for k, h in enumerate(families)]
    gs = [make_g(180 + k) for k in range(4)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaves = leaves_of(cases[0], dtype)
        mask = dev(cases[0]["mask"], torch.bool)
        static_g = dev(gs[0], dtype)

        def step():
            terms = op(*leaves, mask)
            return terms, torch.autograd.grad((terms * static_g).sum(), leaves)
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        terms, grads = step()
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        with torch.no_grad():
            for leaf, name in zip(leaves, INPUTS):
                leaf.copy_(dev(cases[k][name], dtype))
            mask.copy_(dev(cases[k]["mask"], torch.bool))
            static_g.copy_(dev(gs[k], dtype))
        graph.replay()
        torch.cuda.synchronize()
        want = checker_terms(cases[k])
        empty = {"nolow": [1], "nohigh": [2], "nomid": [6, 7]}[families[k]]
        assert not want[empty].any() and all(want[j] != 0 for j in (1, 2, 6, 7) if j not in empty)
        assert_terms(f"replay {k}", terms, want, dtype)
        for name, g in zip(INPUTS, grads):
            assert_close(f"replay {k} d {name}", g, checker_grads(cases[k], gs[k])[name], 1e-11)


def test_capture_inside_a_graphed_step(op):
    """GraphedStep over nn.Linear -> advance_gaussians -> state_loss_terms -> the TEST problem's weighted loss -> backward
    at N = 400, float64: run eagerly and replayed three times with a new state, against the torch composition
    (tests/test_advance.py's torch_forward and the recipe) in float64, 1e-11 of each tensor's scale"""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    from test_advance import make_case as advance_case
    N, c, dtype = 400, 1, torch.float64
    names = ("means", "u", "scaling", "transforms")
    cases = [advance_case(N, c, seed=190 + k, mask="prefix") for k in range(4)]
    for k, case in enumerate(cases):             # heights over all three sets
        case["means"][:, 1] = np.random.default_rng(300 + k).uniform(-1.1, 1.1, N)
    torch.manual_seed(190)
    layer = torch.nn.Linear(6, 5 + c).to("cuda", dtype)
    with torch.no_grad():
        layer.weight.mul_(0.1)
        layer.bias.mul_(0.05)
    params = (layer.weight, layer.bias)
    mask = dev(cases[0]["mask"], torch.bool)

    def step_of(advance, terms_of):
        def fn(means, u, scaling, transforms):
            deltas = layer(torch.cat((means, u, scaling, transforms), dim=-1))
            out = advance(means, u, scaling, transforms, deltas, mask)
            new_means, new_u, penalty = out[0], out[1], out[8]
            losses = compose_losses(terms_of(new_means, new_u, deltas, mask), penalty, WEIGHTS)
            loss = losses[0] + losses[1] + losses[2]
            return (loss.detach(),) + torch.autograd.grad(loss, params + (means, u))
        return fn
    ours = step_of(pigs_amd.advance_gaussians, op)
    theirs = step_of(advance_torch, state_loss_recipe)

    def inputs_of(case):
        return [dev(case[k], dtype).requires_grad_(k in ("means", "u")) for k in names]
    labels = ("loss", "d weight", "d bias", "d means", "d u")
    worst = 0.0
    for name, g, e in zip(labels, ours(*inputs_of(cases[0])), theirs(*inputs_of(cases[0]))):
        worst = max(worst, assert_close(f"eager, {name}", g, host(e), 1e-11))
    step = GraphedStep(ours, lambda: inputs_of(cases[0]), warmup=2)
    for k in (1, 2, 3):
        with torch.no_grad():
            for t, name in zip(step.inputs, names):
                t.copy_(dev(cases[k][name], dtype))
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        for name, g, e in zip(labels, got, theirs(*inputs_of(cases[k]))):
            worst = max(worst, assert_close(f"graphed step, replay {k}, {name}", g, host(e), 1e-11))
        assert float(got[0]) > 0 and got[1].abs().max() > 0
    print(f"[figure] graphed step against the float64 torch composition: worst {worst:.3g} x its bar")
