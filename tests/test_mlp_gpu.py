"""GPU: fused_mlp (pigs_amd/mlp.py, csrc/mlp.hip) against the float64 checker of tests/test_mlp.py.

The accuracy bar is measured, not fixed in advance: for every tensor the error of fused_mlp against the float64 checker
is compared with the error of torch's own float32 nn.Sequential on the GPU on the same tensors,

    err_fused <= 4 err_torch + 1e-6 scale,      scale = the tensor's largest magnitude

(the factor 4 allows for a different summation order and a different tanh, the floor covers tensors where torch happens to
be exact).  Each case prints its worst err_fused / (4 err_torch + 1e-6 scale).
"""
import ctypes

import numpy as np
import pytest
import torch

from test_mlp import (MODEL_NETS, NETS, checker_backward, checker_forward, ints, make_net, make_rows, pointers, scale_of,
                      sequential_of)

pytestmark = pytest.mark.gpu

# the tile edge (16 rows), the workgroup edge (64), the model's size, and 4 097 = 257 tiles: more than the 256 waves of
# the backward's capped grid, so that its grid-stride loop runs (the forward's: test_more_tiles_than_the_forward_has_waves)
SIZES = (1, 15, 16, 17, 63, 64, 65, 1600, 4097)


@pytest.fixture(scope="module")
def mlp(hip_lib):
    import pigs_amd
    return pigs_amd.fused_mlp


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def params_of(Ws, bs, requires=True):
    W = [dev(w).requires_grad_(requires) for w in Ws]
    b = [dev(v).requires_grad_(requires) for v in bs]
    return W, b


def names_of(L):
    return ["y", "g_x"] + [f"g_W[{l}]" for l in range(L)] + [f"g_b[{l}]" for l in range(L)]


def checker_all(x, Ws, bs, g_y):
    y, _ = checker_forward(x, Ws, bs)
    g_x, g_W, g_b = checker_backward(x, Ws, bs, g_y)
    return [y, g_x] + g_W + g_b


def fused_all(mlp, x, Ws, bs, g_y):
    tx = dev(x).requires_grad_(True)
    W, b = params_of(Ws, bs)
    y = mlp(tx, W, b)
    grads = torch.autograd.grad(y, [tx] + W + b, dev(g_y))
    return [y.detach()] + list(grads)


def torch_all(x, Ws, bs, g_y):
    """torch's own float32 nn.Sequential on the GPU, on the same tensors"""
    seq = sequential_of(Ws, bs, dtype=torch.float32, device="cuda")
    tx = dev(x).requires_grad_(True)
    y = seq(tx)
    linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
    grads = torch.autograd.grad(y, [tx] + [m.weight for m in linears] + [m.bias for m in linears], dev(g_y))
    return [y.detach()] + list(grads)


def worst_ratio(what, fused, ref, want):
    """the bar of the module text over a list of tensors; returns the worst err_fused / bound"""
    worst = 0.0
    for name, f, t, w in zip(names_of((len(want) - 2) // 2), fused, ref, want):
        assert tuple(f.shape) == w.shape, (what, name)
        scale = scale_of(w)
        err_f, err_t = np.abs(host(f) - w).max(), np.abs(host(t) - w).max()
        bound = 4.0 * err_t + 1e-6 * scale
        worst = max(worst, err_f / bound)
        assert err_f <= bound, f"{what} {name}: fused {err_f:.3g}, torch {err_t:.3g}, scale {scale:.3g}"
    return worst


_reference = {}


def reference(name, N):
    """the case's tensors, the checker's results and torch's float32 results: computed once, shared, never changed"""
    key = (name, N)
    if key not in _reference:
        widths = NETS[name]
        seed = 1000 * sorted(NETS).index(name) + N
        Ws, bs = make_net(widths, seed)
        x, g_y = make_rows(N, widths[0], seed + 1), make_rows(N, widths[-1], seed + 2)
        _reference[key] = (x, Ws, bs, g_y, checker_all(x, Ws, bs, g_y), torch_all(x, Ws, bs, g_y))
    return _reference[key]


# ---- shapes and accuracy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES, ids=[f"N{n}" for n in SIZES])
@pytest.mark.parametrize("name", list(NETS))
def test_every_net_at_every_size(mlp, name, N):
    x, Ws, bs, g_y, want, ref = reference(name, N)
    worst = worst_ratio(f"{name} N={N}", fused_all(mlp, x, Ws, bs, g_y), ref, want)
    print(f"{name} N={N}: worst err_fused / (4 err_torch + 1e-6 scale) = {worst:.3f}")


@pytest.mark.parametrize("name", ["delta_net_c2", "17_33_47_1"])
def test_more_tiles_than_the_forward_has_waves(mlp, name):
    """the forward writes no records and caps its grid at 2 048 waves: N = 16 x 2 048 + 1 makes its grid-stride loop run
    (the backward's, capped at 256 waves, runs at 4 097 already); the same bar, and the same bits twice"""
    N = 16 * 2048 + 1
    x, Ws, bs, g_y, want, ref = reference(name, N)
    got = fused_all(mlp, x, Ws, bs, g_y)
    worst = worst_ratio(f"{name} N={N}", got, ref, want)
    print(f"{name} N={N}: worst err_fused / (4 err_torch + 1e-6 scale) = {worst:.3f}")
    for what, a, b in zip(names_of(len(Ws)), got, fused_all(mlp, x, Ws, bs, g_y)):
        assert torch.equal(a, b), f"{what} differs between two calls on the same inputs"


# ---- exactness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [(48, 48), (5, 3), (17, 33), (33, 17), (1, 1)], ids=lambda w: f"{w[0]}to{w[1]}")
@pytest.mark.parametrize("N", [16, 37, 4097])
def test_one_layer_with_small_integers_is_exact(mlp, widths, N):
    """L = 1, integer x, W, b, g_y with a non-symmetric W and every sum below 2^24: y, g_x, g_W, g_b bit-equal to the
    integer results.  A permuted k index or a swapped row / column cannot pass: W[o][i] = 3 o - 2 i + (o i) % 5 - 1."""
    w_in, w_out = widths
    rng = np.random.default_rng(N + w_in)
    o, i = np.meshgrid(np.arange(w_out), np.arange(w_in), indexing="ij")
    W = (3 * o - 2 * i + (o * i) % 5 - 1).astype(np.float64)
    b = (np.arange(w_out) % 7 - 3).astype(np.float64)
    x = rng.integers(-4, 5, (N, w_in)).astype(np.float64)
    g_y = rng.integers(-3, 4, (N, w_out)).astype(np.float64)
    want = checker_all(x, [W], [b], g_y)
    assert max(np.abs(np.abs(x) @ np.abs(W).T).max() + 3, (np.abs(g_y).T @ np.abs(x)).max(),
               (np.abs(g_y) @ np.abs(W)).max()) < 2 ** 24
    got = fused_all(mlp, x, [W], [b], g_y)
    for name, g, w in zip(names_of(1), got, want):
        assert np.array_equal(host(g), w), f"{name}: {np.abs(host(g) - w).max()} off an integer result"


# ---- masking ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["delta_net_c2", "input_projection_wave", "17_33_47_1"])
@pytest.mark.parametrize("N", [1, 17, 1611])
def test_rows_past_the_end_are_never_read_or_written(hip_lib, name, N):
    """through the C ABI with buffers of its own: x and g_y are the heads of larger buffers whose following rows are NaN,
    N is no multiple of 16, and 64 sentinel elements stand behind y, g_x, every g_W / g_b and the scratch"""
    widths = NETS[name]
    L, pad, sentinel = len(widths) - 1, 64, -12345.0
    x, Ws, bs, g_y, want, _ = reference(name, N)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def with_nan_rows(a):
        t = torch.full((N + 16, a.shape[1]), float("nan"), device="cuda")
        t[:N] = dev(a)
        return t

    def padded(n):
        return torch.full((n + pad,), sentinel, device="cuda")
    tx, tg = with_nan_rows(x), with_nan_rows(g_y)
    W, b = params_of(Ws, bs, requires=False)
    w = ints(*widths)
    y = padded(N * widths[-1])
    rc = hip_lib.pigs_mlp_forward(0, N, L, w, tx.data_ptr(), pointers(*[t.data_ptr() for t in W]),
                                  pointers(*[t.data_ptr() for t in b]), y.data_ptr(), stream)
    assert rc == 0
    nbytes = hip_lib.pigs_mlp_scratch_bytes(N, L, w)
    scratch = padded(nbytes // 4)
    g_x = padded(N * widths[0])
    g_W, g_b = [padded(t.numel()) for t in W], [padded(t.numel()) for t in b]
    rc = hip_lib.pigs_mlp_backward(0, N, L, w, tx.data_ptr(), pointers(*[t.data_ptr() for t in W]),
                                   pointers(*[t.data_ptr() for t in b]), tg.data_ptr(), scratch.data_ptr(), nbytes,
                                   g_x.data_ptr(), pointers(*[t.data_ptr() for t in g_W]),
                                   pointers(*[t.data_ptr() for t in g_b]), stream)
    assert rc == 0
    torch.cuda.synchronize()
    for what, t, ref in zip(names_of(L) + ["scratch"], [y, g_x] + g_W + g_b + [scratch], want + [None]):
        assert (t[-pad:] == sentinel).all(), f"{what}: written past its end"
        assert not torch.isnan(t).any(), f"{what}: a NaN of the rows past N came through"
        assert not (t[:-pad] == sentinel).any(), f"{what}: not all of it was written"
        if ref is not None:
            assert np.abs(host(t[:-pad]) - ref.reshape(-1)).max() <= 1e-4 * scale_of(ref), what


# ---- reproducibility ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["delta_net_c2", "six_of_48", "5to3"])
def test_three_calls_give_the_same_bits(mlp, name):
    x, Ws, bs, g_y, _, _ = reference(name, 4097)
    first = fused_all(mlp, x, Ws, bs, g_y)
    for _ in range(2):
        for what, a, b in zip(names_of(len(Ws)), first, fused_all(mlp, x, Ws, bs, g_y)):
            assert torch.equal(a, b), f"{what} differs between two calls on the same inputs"


# ---- autograd -----------------------------------------------------------------------------------------------
def grads_with(mlp, x, Ws, bs, g_y, x_requires, frozen):
    """.grad of x, W, b after backward() with layers ``frozen`` (and x, unless ``x_requires``) not requiring a gradient"""
    tx = dev(x).requires_grad_(x_requires)
    W, b = params_of(Ws, bs)
    for l in frozen:
        W[l].requires_grad_(False)
        b[l].requires_grad_(False)
    y = mlp(tx, W, b)
    y.backward(dev(g_y).reshape(y.shape))
    return [tx.grad] + [t.grad for t in W] + [t.grad for t in b]


@pytest.mark.parametrize("pattern", ["x_only", "weights_only", "one_layer_frozen", "biases_only"])
def test_needs_input_grad(mlp, pattern):
    """a gradient that is not asked for is None, the others are bit for bit those of the full backward"""
    name, N = "delta_net_c1", 333
    x, Ws, bs, g_y, want, _ = reference(name, N)
    L = len(Ws)
    full = fused_all(mlp, x, Ws, bs, g_y)[1:]
    if pattern == "biases_only":
        tx = dev(x)
        W, b = params_of(Ws, bs)
        for t in W:
            t.requires_grad_(False)
        mlp(tx, W, b).backward(dev(g_y))
        got = [None] * (1 + L) + [t.grad for t in b]
    else:
        x_requires = pattern != "weights_only"
        frozen = {"x_only": range(L), "weights_only": (), "one_layer_frozen": (2,)}[pattern]
        got = grads_with(mlp, x, Ws, bs, g_y, x_requires, frozen)
    asked = 0
    for what, g, f in zip(names_of(L)[1:], got, full):
        if g is not None:
            asked += 1
            assert torch.equal(g, f), f"{pattern}: {what} differs from the full backward"
    expect = {"x_only": 1, "weights_only": 2 * L, "one_layer_frozen": 1 + 2 * (L - 1), "biases_only": L}[pattern]
    assert asked == expect, (pattern, asked)


def test_leading_one_and_nothing_requiring_grad(mlp):
    name, N = "input_projection_ns", 100
    x, Ws, bs, g_y, want, _ = reference(name, 1600)
    x, g_y = x[:N], g_y[:N]
    W, b = params_of(Ws, bs, requires=False)
    flat = mlp(dev(x), W, b)
    assert not flat.requires_grad
    tx = dev(x)[None].requires_grad_(True)
    y = mlp(tx, W, b)
    assert y.shape == (1, N, NETS[name][-1]) and torch.equal(y[0], flat)
    y.backward(dev(g_y)[None])
    assert tx.grad.shape == tx.shape
    assert np.abs(host(tx.grad[0]) - checker_backward(x, Ws, bs, g_y)[0]).max() <= 1e-5 * scale_of(want[1])
    # a gradient that arrives as a strided view
    tx2 = dev(x).requires_grad_(True)
    wide = torch.zeros(N, 2 * NETS[name][-1], device="cuda")
    wide[:, ::2] = dev(g_y)
    mlp(tx2, W, b).backward(wide[:, ::2])
    assert torch.equal(tx2.grad, tx.grad[0])


def test_from_sequential_gives_grad_to_the_shared_parameters(mlp):
    import pigs_amd
    name, N = "delta_net_c2", 257
    x, Ws, bs, g_y, want, _ = reference(name, 4097)
    x, g_y = x[:N], g_y[:N]
    want = checker_all(x, Ws, bs, g_y)
    seq = sequential_of(Ws, bs, dtype=torch.float32, device="cuda")
    net = pigs_amd.FusedMLP.from_sequential(seq)
    tx = dev(x)[None].requires_grad_(True)
    y = net(tx)
    y.backward(dev(g_y)[None])
    linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
    got = [y[0], tx.grad[0]] + [m.weight.grad for m in linears] + [m.bias.grad for m in linears]
    for what, g, w in zip(names_of(len(Ws)), got, want):
        assert g is not None, f"{what}: the wrapped nn.Sequential's parameter received no .grad"
        assert np.abs(host(g) - w).max() <= 1e-5 * scale_of(w), what
    assert torch.equal(y, net(tx.detach())) and not torch.equal(y, torch.zeros_like(y))


# ---- capture ------------------------------------------------------------------------------------------------
def test_capture_of_forward_and_backward(mlp):
    """torch.cuda.graph around fused_mlp and autograd.grad; three replays with x, the weights and g_y rewritten in place,
    each bit for bit the eager call on the same tensors"""
    name, N = "delta_net_c2", 1600
    widths = NETS[name]
    L = len(widths) - 1
    cases = []
    for k in range(4):
        Ws, bs = make_net(widths, 50 + k)
        cases.append([make_rows(N, widths[0], 60 + k)] + Ws + bs + [make_rows(N, widths[-1], 70 + k)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaves = [dev(a).requires_grad_(True) for a in cases[0][:-1]]
        g = dev(cases[0][-1])

        def step():
            y = mlp(leaves[0], leaves[1:1 + L], leaves[1 + L:])
            return (y.detach(),) + torch.autograd.grad(y, leaves, g)
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        with torch.no_grad():
            for leaf, a in zip(leaves, cases[k][:-1]):
                leaf.copy_(dev(a))
            g.copy_(dev(cases[k][-1]))
        graph.replay()
        torch.cuda.synchronize()
        eager = fused_all(mlp, cases[k][0], cases[k][1:1 + L], cases[k][1 + L:-1], cases[k][-1])
        for what, a, b in zip(names_of(L), outs, eager):
            assert torch.equal(a, b), f"replay {k}: {what} differs from the eager call"
        want = checker_all(cases[k][0], cases[k][1:1 + L], cases[k][1 + L:-1], cases[k][-1])
        assert np.abs(host(outs[0]) - want[0]).max() <= 1e-5 * scale_of(want[0])


def test_capture_inside_a_graphed_step(mlp):
    """GraphedStep over FusedMLP.from_sequential -> loss -> backward: three replays on new x against eager"""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    name, N = "input_projection_wave", 1600
    widths = NETS[name]
    Ws, bs = make_net(widths, 80)
    net = pigs_amd.FusedMLP.from_sequential(sequential_of(Ws, bs, dtype=torch.float32, device="cuda"))
    params = list(net.parameters())

    def fn(x):
        loss = torch.mean(net(x) ** 2)
        return (loss.detach(),) + torch.autograd.grad(loss, [x] + params)
    step = GraphedStep(fn, lambda: [dev(make_rows(N, widths[0], 81)).requires_grad_(True)], warmup=2)
    for k in (1, 2, 3):
        x = dev(make_rows(N, widths[0], 81 + k))
        with torch.no_grad():
            step.inputs[0].copy_(x)
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        for a, b in zip(got, fn(x.requires_grad_(True))):
            assert torch.equal(a, b), f"replay {k} differs from the eager step"
        assert float(got[0]) > 0


# ---- end to end ---------------------------------------------------------------------------------------------
def test_five_adam_steps_against_the_same_net_in_torch():
    """a small regression through FusedMLP.from_sequential(a delta_net-shaped net) and through the same nn.Sequential in
    torch, from the same weights: each side's loss curve against the float64 curve of the same five steps, with the bar of
    the module text"""
    import pigs_amd
    widths, N = MODEL_NETS["delta_net_c2"], 400
    Ws, bs = make_net(widths, 90)
    x, target = make_rows(N, widths[0], 91), 0.1 * make_rows(N, widths[-1], 92)

    def curve(net, dtype, device):
        opt = torch.optim.Adam(net.parameters(), lr=1e-2)
        tx, tt = torch.as_tensor(x, dtype=dtype, device=device), torch.as_tensor(target, dtype=dtype, device=device)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = torch.mean((net(tx) - tt) ** 2)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return np.array(losses)
    want = curve(sequential_of(Ws, bs), torch.float64, "cpu")
    ref = curve(sequential_of(Ws, bs, dtype=torch.float32, device="cuda"), torch.float32, "cuda")
    seq = sequential_of(Ws, bs, dtype=torch.float32, device="cuda")
    got = curve(pigs_amd.FusedMLP.from_sequential(seq), torch.float32, "cuda")
    assert want[-1] < want[0]
    err_f, err_t, scale = np.abs(got - want).max(), np.abs(ref - want).max(), scale_of(want)
    print(f"five Adam steps: fused {err_f:.3g}, torch {err_t:.3g} off the float64 curve of scale {scale:.3g}")
    assert err_f <= 4.0 * err_t + 1e-6 * scale
