"""GPU: fused_mlp_joined (pigs_amd/mlp.py, csrc/mlp_joined.hip) against fused_mlp on the cat, bit for bit, and against the
float64 checker of tests/test_mlp_joined.py.

Bits: y, every g_W / g_b (with and without block means) and, without block means, every g_part are torch.equal to
fused_mlp(torch.cat(parts, -1)) and its gradients.  Accuracy: m, and the g_parts with g_m != 0, are held to the checker
with tests/test_mlp_gpu.py's bar,

    err_joined <= 4 err_torch32 + 1e-6 scale,      scale = the tensor's largest magnitude

where torch32 is the cat + nn.Sequential + slice / pow / mean composition in float32 on the GPU on the same tensors.
Each case prints its worst err_joined / (4 err_torch32 + 1e-6 scale).
"""
import ctypes

import numpy as np
import pytest
import torch

from test_mlp import NETS, ints, make_net, make_rows, pointers, scale_of, sequential_of
from test_mlp_gpu import dev, host, params_of
from test_mlp_joined import CASES, block_count, case_arrays, checker_joined, flat, split, torch_joined

pytestmark = pytest.mark.gpu

# the tile edge (16 rows), the workgroup edge (64), the model's size, and 4 097 = 257 tiles: more than the 256 waves of
# the backward's capped grid (the forward's 2 048: test_more_tiles_than_the_forward_has_waves)
SIZES = (1, 15, 16, 17, 65, 1600, 4097)


@pytest.fixture(scope="module")
def joined(hip_lib):
    import pigs_amd
    return pigs_amd.fused_mlp_joined


@pytest.fixture(scope="module")
def mlp(hip_lib):
    import pigs_amd
    return pigs_amd.fused_mlp


def joined_all(joined, parts, Ws, bs, blocks, g_y, g_m, requires=None):
    """(y, m, [g_part], [g_W], [g_b]) as tensors; a leaf that does not require a gradient gives None.  g_y / g_m None:
    that output is not used."""
    P, L = len(parts), len(Ws)
    requires = requires or [True] * (P + 2 * L)
    tp = [dev(t).requires_grad_(r) for t, r in zip(parts, requires)]
    W, b = params_of(Ws, bs, requires=False)
    for t, r in zip(W + b, requires[P:]):
        t.requires_grad_(r)
    out = joined(tp, W, b, block_means=blocks)
    y, m = out if blocks is not None else (out, torch.zeros(0, device="cuda"))
    outs, gouts = [], []
    if g_y is not None:
        outs.append(y)
        gouts.append(dev(g_y))
    if g_m is not None and block_count(blocks):
        outs.append(m)
        gouts.append(dev(g_m))
    leaves = [t for t in tp + W + b if t.requires_grad]
    grads = iter(torch.autograd.grad(outs, leaves, gouts))
    all_grads = [next(grads) if t.requires_grad else None for t in tp + W + b]
    return y.detach(), m.detach(), all_grads[:P], all_grads[P:P + L], all_grads[P + L:]


def cat_all(mlp, parts, Ws, bs, g_y):
    """fused_mlp on the cat: (y, g_x, [g_W], [g_b])"""
    x = torch.cat([dev(t) for t in parts], dim=-1).requires_grad_(True)
    W, b = params_of(Ws, bs)
    y = mlp(x, W, b)
    grads = torch.autograd.grad(y, [x] + W + b, dev(g_y))
    L = len(Ws)
    return y.detach(), grads[0], list(grads[1:1 + L]), list(grads[1 + L:])


_reference = {}


def reference(mlp, name, N):
    """the case's arrays, the checker's results, torch's float32 results and fused_mlp's on the cat: computed once, shared,
    never changed"""
    key = (name, N)
    if key not in _reference:
        args = case_arrays(name, N)
        _reference[key] = (args, flat(checker_joined(*args)), flat(torch_joined(*args, dtype=torch.float32, device="cuda")),
                           cat_all(mlp, args[0], args[1], args[2], args[4]))
    return _reference[key]


def equal_to_the_cat(what, got, cat, part_widths, parts_too):
    y, _, g_parts, g_W, g_b = got
    cy, cg_x, cg_W, cg_b = cat
    assert torch.equal(y, cy), f"{what}: y differs from fused_mlp on the cat"
    for l, (a, b) in enumerate(zip(g_W + g_b, cg_W + cg_b)):
        assert torch.equal(a, b), f"{what}: parameter gradient {l} differs from fused_mlp on the cat"
    if parts_too:
        edges = np.cumsum((0,) + tuple(part_widths))
        for p, g in enumerate(g_parts):
            assert g.is_contiguous() and torch.equal(g, cg_x[:, edges[p]:edges[p + 1]]), f"{what}: g_part[{p}]"


def worst_ratio(what, got, ref, want, only):
    """the bar of the module text over the named tensors; returns the worst err_joined / bound"""
    worst = 0.0
    for (name, g), (_, t), (_, w) in zip(flat(got), ref, want):
        if not name.startswith(only) or not w.size:
            continue
        assert tuple(g.shape) == w.shape, (what, name)
        scale = scale_of(w)
        err_j, err_t = np.abs(host(g) - w).max(), np.abs(host(t) - w).max()
        bound = 4.0 * err_t + 1e-6 * scale
        worst = max(worst, err_j / bound)
        assert err_j <= bound, f"{what} {name}: joined {err_j:.3g}, torch {err_t:.3g}, scale {scale:.3g}"
    return worst


# ---- bits and accuracy --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES, ids=[f"N{n}" for n in SIZES])
@pytest.mark.parametrize("name", list(CASES))
def test_every_case_at_every_size(joined, mlp, name, N):
    (parts, Ws, bs, blocks, g_y, g_m), want, ref, cat = reference(mlp, name, N)
    part_widths = CASES[name][1]
    plain = joined_all(joined, parts, Ws, bs, None, g_y, None)
    equal_to_the_cat(f"{name} N={N}, no block means", plain, cat, part_widths, parts_too=True)
    if blocks is None:
        return
    got = joined_all(joined, parts, Ws, bs, blocks, g_y, g_m)
    equal_to_the_cat(f"{name} N={N}, block means", got, cat, part_widths, parts_too=False)
    worst = worst_ratio(f"{name} N={N}", got, ref, want, ("m", "g_part"))
    print(f"{name} N={N}: worst err_joined / (4 err_torch32 + 1e-6 scale) = {worst:.3f}")


def test_more_tiles_than_the_forward_has_waves(joined, mlp):
    """the model's shape at N = 16 x 2 048 + 1, forward only: the forward's grid of 2 048 waves strides, and a wave's record
    holds the column sums of two tiles"""
    N = 16 * 2048 + 1
    parts, Ws, bs, blocks, _, _ = case_arrays("model", N)
    tp = [dev(t) for t in parts]
    W, b = params_of(Ws, bs, requires=False)
    y, m = joined(tp, W, b, block_means=blocks)
    assert torch.equal(y, mlp(torch.cat(tp, dim=-1), W, b))
    want = np.array([(parts[1][:, 16 * q:16 * (q + 1)] ** 2).mean() for q in range(2)])
    ref = torch.stack([tp[1][:, 16 * q:16 * (q + 1)].pow(2).mean() for q in range(2)])
    err_j, err_t = np.abs(host(m) - want).max(), np.abs(host(ref) - want).max()
    print(f"model N={N}: m off by {err_j:.3g}, torch32 by {err_t:.3g}, scale {scale_of(want):.3g}")
    assert err_j <= 4.0 * err_t + 1e-6 * scale_of(want)
    y2, m2 = joined(tp, W, b, block_means=blocks)
    assert torch.equal(y, y2) and torch.equal(m, m2)


# ---- exactness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 37, 4097])
def test_one_layer_with_small_integers_is_exact(joined, N):
    """tests/test_mlp_gpu.py's construction on parts (5, 3, 9): L = 1, integer x, W, b, g_y with a non-symmetric W and
    every sum below 2^24: y, the g_parts, g_W, g_b bit-equal to the integer results, and every block's sum of squares
    exact, so that m is that integer times 1 / (N columns) rounded once"""
    part_widths, blocks, w_in, w_out = (5, 3, 9), (1, 3, 3), 17, 33
    rng = np.random.default_rng(N + w_in)
    o, i = np.meshgrid(np.arange(w_out), np.arange(w_in), indexing="ij")
    W = (3 * o - 2 * i + (o * i) % 5 - 1).astype(np.float64)
    b = (np.arange(w_out) % 7 - 3).astype(np.float64)
    x = rng.integers(-4, 5, (N, w_in)).astype(np.float64)
    g_y = rng.integers(-3, 4, (N, w_out)).astype(np.float64)
    parts = split(x, part_widths)
    want = checker_joined(parts, [W], [b], blocks, g_y, None)
    assert max(np.abs(np.abs(x) @ np.abs(W).T).max() + 3, (np.abs(g_y).T @ np.abs(x)).max(),
               (np.abs(g_y) @ np.abs(W)).max(), (x ** 2).sum()) < 2 ** 24
    got = joined_all(joined, parts, [W], [b], blocks, g_y, None)
    for (name, g), (_, w) in zip(flat(got), flat(want)):
        if name != "m":
            assert np.array_equal(host(g), w), f"{name}: {np.abs(host(g) - w).max()} off an integer result"
    sums, j = [], 0
    for part, nb in zip(parts, blocks):
        cols = part.shape[1] // nb
        sums += [(part[:, q * cols:(q + 1) * cols] ** 2).sum() * (1.0 / (N * cols)) for q in range(nb)]
    assert np.array_equal(got[1].cpu().numpy(), np.array(sums).astype(np.float32)), "m"


# ---- autograd -----------------------------------------------------------------------------------------------
NEEDS = ("part0", "part1", "part2", "part3", "parameters", "m_alone", "y_alone")


@pytest.mark.parametrize("pattern", NEEDS)
def test_needs_input_grad(joined, pattern):
    """a gradient that is not asked for is None; the others are bit for bit those of the backward of the same loss with
    every leaf asking.  m_alone: y is not used (no g_y reaches the backward); y_alone: m is asked for and not used, and
    the gradients are also those of the call without block means"""
    widths, part_widths, blocks, N = NETS["48to48"], (1, 1, 45, 1), (0, 1, 3, 0), 333
    Ws, bs = make_net(widths, 41)
    parts = split(make_rows(N, widths[0], 42), part_widths)
    g_y, g_m = make_rows(N, widths[-1], 43), make_rows(1, 4, 44)[0]
    P, L = 4, 1
    if pattern == "m_alone":
        g_y = None
    if pattern == "y_alone":
        g_m = None
    full = joined_all(joined, parts, Ws, bs, blocks, g_y, g_m)
    requires = [True] * (P + 2 * L)
    if pattern.startswith("part"):
        requires = [k == int(pattern[4]) for k in range(P)] + [False] * (2 * L)
    if pattern == "parameters":
        requires = [False] * P + [True] * (2 * L)
    got = joined_all(joined, parts, Ws, bs, blocks, g_y, g_m, requires)
    asked = 0
    for (name, g), (_, f) in zip(flat(got)[2:], flat(full)[2:]):
        if g is not None:
            asked += 1
            assert torch.equal(g, f), f"{pattern}: {name} differs from the full backward"
    assert asked == sum(requires), (pattern, asked)
    want = flat(checker_joined(parts, Ws, bs, blocks, g_y, g_m))[2:]
    for (name, f), (_, w) in zip(flat(full)[2:], want):
        assert np.abs(host(f) - w).max() <= 1e-5 * max(scale_of(w), 1.0), (pattern, name)
    if pattern == "y_alone":
        for (name, g), (_, f) in zip(flat(joined_all(joined, parts, Ws, bs, None, g_y, None))[2:], flat(full)[2:]):
            assert torch.equal(g, f), f"{name}: an unused m changed the gradient's bits"
    if pattern == "m_alone":
        assert all(not t.any() for t in full[3] + full[4]), "a parameter gradient without g_y"


def test_the_forms_of_the_model(joined):
    """features [1, N, 16] and the heads' [N, H, L] as they are: y [1, N, 7], gradients in the parts' shapes, the bits of
    the flat call"""
    N = 100
    parts, Ws, bs, blocks, g_y, g_m = case_arrays("model", N)
    flat_call = joined_all(joined, parts, Ws, bs, blocks, g_y, g_m)
    features, nf = dev(parts[0])[None].requires_grad_(True), dev(parts[1]).reshape(N, 2, 16).requires_grad_(True)
    W, b = params_of(Ws, bs)
    y, m = joined((features, nf), W, b, block_means=blocks)
    assert y.shape == (1, N, 7) and m.shape == (2,)
    g_f, g_nf = torch.autograd.grad([y, m], [features, nf], [dev(g_y)[None], dev(g_m)])
    assert g_f.shape == features.shape and g_nf.shape == nf.shape and g_nf.is_contiguous()
    assert torch.equal(y[0], flat_call[0]) and torch.equal(m, flat_call[1])
    assert torch.equal(g_f[0], flat_call[2][0]) and torch.equal(g_nf.reshape(N, 32), flat_call[2][1])
    flat_y = joined((dev(parts[0]), nf.detach()), W, b)                      # part 0 without the 1: y without it
    assert flat_y.shape == (N, 7) and torch.equal(flat_y, y[0])


def test_the_module_gives_grad_to_its_own_parameters(joined):
    import pigs_amd
    N = 257
    parts, Ws, bs, blocks, g_y, g_m = case_arrays("model", N)
    seq = sequential_of(Ws, bs, dtype=torch.float32, device="cuda")
    net = pigs_amd.FusedMLP.from_sequential(seq)
    tp = [dev(t).requires_grad_(True) for t in parts]
    y, m = net.joined(tp, block_means=blocks)
    ((y * dev(g_y)).sum() + (m * dev(g_m)).sum()).backward()
    full = joined_all(joined, parts, Ws, bs, blocks, g_y, g_m)
    linears = [mod for mod in seq if isinstance(mod, torch.nn.Linear)]
    got = [y.detach(), m.detach()] + [t.grad for t in tp] + [mod.weight.grad for mod in linears] + [mod.bias.grad for mod in linears]
    for g, (name, f) in zip(got, flat(full)):
        assert g is not None and torch.equal(g, f), name


# ---- masking ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["model", "straddles", "one_column_blocks"])
@pytest.mark.parametrize("N", [17, 1611])
def test_rows_past_the_end_are_never_read_or_written(hip_lib, name, N):
    """through the C ABI with buffers of its own: every part and g_y are the heads of larger buffers whose following rows
    are NaN, N is no multiple of 16, and 64 sentinel elements stand behind y, m, every g_part, every g_W / g_b and both
    scratches"""
    net, part_widths, blocks = CASES[name]
    widths = NETS[net]
    L, P, pad, sentinel = len(widths) - 1, len(part_widths), 64, -12345.0
    parts, Ws, bs, _, g_y, g_m = case_arrays(name, N)
    want = flat(checker_joined(parts, Ws, bs, blocks, g_y, g_m))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def with_nan_rows(a):
        t = torch.full((N + 16, a.shape[1]), float("nan"), device="cuda")
        t[:N] = dev(a)
        return t

    def padded(n):
        return torch.full((n + pad,), sentinel, device="cuda")

    def ptrs(ts):
        return pointers(*[t.data_ptr() for t in ts])
    tp, tg, tm = [with_nan_rows(t) for t in parts], with_nan_rows(g_y), dev(g_m)
    W, b = params_of(Ws, bs, requires=False)
    w, pw, bl = ints(*widths), ints(*part_widths), ints(*blocks)
    y, m = padded(N * widths[-1]), padded(block_count(blocks))
    fbytes = hip_lib.pigs_mlp_joined_scratch_bytes(N, L, w, P, bl, 0)
    fscratch = padded(fbytes // 4)
    rc = hip_lib.pigs_mlp_joined_forward(0, N, L, w, P, pw, ptrs(tp), bl, ptrs(W), ptrs(b), fscratch.data_ptr(), fbytes,
                                         y.data_ptr(), m.data_ptr(), stream)
    assert rc == 0
    bbytes = hip_lib.pigs_mlp_joined_scratch_bytes(N, L, w, P, bl, 1)
    bscratch = padded(bbytes // 4)
    g_parts = [padded(N * k) for k in part_widths]
    g_W, g_b = [padded(t.numel()) for t in W], [padded(t.numel()) for t in b]
    rc = hip_lib.pigs_mlp_joined_backward(0, N, L, w, P, pw, ptrs(tp), bl, ptrs(W), ptrs(b), tg.data_ptr(), tm.data_ptr(),
                                          bscratch.data_ptr(), bbytes, ptrs(g_parts), ptrs(g_W), ptrs(g_b), stream)
    assert rc == 0
    torch.cuda.synchronize()
    outs = [y, m] + g_parts + g_W + g_b + [fscratch, bscratch]
    for (what, ref), t in zip(want + [("forward scratch", None), ("backward scratch", None)], outs):
        assert (t[-pad:] == sentinel).all(), f"{what}: written past its end"
        assert not torch.isnan(t).any(), f"{what}: a NaN of the rows past N came through"
        assert not (t[:-pad] == sentinel).any(), f"{what}: not all of it was written"
        if ref is not None:
            assert np.abs(host(t[:-pad]) - ref.reshape(-1)).max() <= 1e-4 * scale_of(ref), what


# ---- reproducibility and capture ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["model", "six_layers"])
def test_three_calls_give_the_same_bits(joined, name):
    args = case_arrays(name, 4097)
    first = flat(joined_all(joined, *args))
    for _ in range(2):
        for (what, a), (_, b) in zip(first, flat(joined_all(joined, *args))):
            assert torch.equal(a, b), f"{what} differs between two calls on the same inputs"


def test_capture_inside_a_graphed_step(joined):
    """GraphedStep over FusedMLP.joined -> the step's loss and magnitude_loss -> backward: three replays on new parts, each
    bit for bit the eager step"""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    N = 1600
    net_name, part_widths, blocks = CASES["model"]
    widths = NETS[net_name]
    Ws, bs = make_net(widths, 80)
    net = pigs_amd.FusedMLP.from_sequential(sequential_of(Ws, bs, dtype=torch.float32, device="cuda"))
    params = list(net.parameters())

    def fn(features, nf):
        deltas, mags = net.joined((features, nf), block_means=blocks)
        loss = torch.mean(deltas ** 2) + ((mags - 1.0) ** 2).mean()
        return (loss.detach(), mags.detach()) + torch.autograd.grad(loss, [features, nf] + params)

    def inputs(seed):
        f, nf = split(make_rows(N, widths[0], seed), part_widths)
        return [dev(f)[None].requires_grad_(True), dev(nf).reshape(N, 2, 16).requires_grad_(True)]
    step = GraphedStep(fn, lambda: inputs(81), warmup=2)
    for k in (1, 2, 3):
        new = inputs(81 + k)
        with torch.no_grad():
            for leaf, t in zip(step.inputs, new):
                leaf.copy_(t)
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        for a, b in zip(got, fn(*new)):
            assert torch.equal(a, b), f"replay {k} differs from the eager step"
        assert float(got[0]) > 0
