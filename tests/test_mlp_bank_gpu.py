"""GPU: the bank of fused MLPs (pigs_amd/mlp.py fused_mlp_bank / FusedMLPBank, csrc/mlp_bank.hip) against the float64
checker of tests/test_mlp.py run per net, with g_x summed over the nets in float64.

The bar is that of tests/test_mlp_gpu.py (measured, not fixed in advance): for y and every gradient

    err_bank <= 4 err_torch + 1e-6 scale,      scale = the tensor's largest magnitude,

err_torch that of torch's own float32 nn.Sequentials with torch.stack on the same tensors.  In addition y of net b must
have the BITS of fused_mlp on that net: both run the same per-layer helper.

A result list is [y, g_x, g_W of (net 0, layer 0), (net 0, layer 1), ..., g_b in the same order]: parameter k = b L + l.

MEASURED (MI355X): the suite's largest err_bank / (4 err_torch + 1e-6 scale) is printed per case; see DESIGN.md section 21.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_mlp import checker_backward, checker_forward, ints, make_net, make_rows, pointers, scale_of, sequential_of
from test_mlp_gpu import dev, host, names_of, params_of, worst_ratio

pytestmark = pytest.mark.gpu

MODEL = (16, 16, 16, 16, 16)
BANKS = {                           # widths, B, G
    "model_b4g2": (MODEL, 4, 2),
    "model_b1g1": (MODEL, 1, 1),
    "model_b3g3": (MODEL, 3, 3),
    "model_b8g2": (MODEL, 8, 2),
    "5to3_b3g1": ((5, 3), 3, 1),
    "17_33_47_1_b2g2": ((17, 33, 47, 1), 2, 2),
    "six_of_48_b2g1": ((48,) * 7, 2, 1),
}
# the tile edge (16 rows), more than one workgroup (65), the model's size, and 4 097 = 257 tiles: more than the 256 waves
# per net of the backward's capped grid
SIZES = (1, 15, 16, 17, 65, 1600, 4097)


@pytest.fixture(scope="module")
def bank(hip_lib):
    import pigs_amd
    return pigs_amd.fused_mlp_bank


def layout(per_net, G):
    """[G][N][B / G][w] from B arrays (numpy) or tensors [N][w], as torch.stack composes queries and keys"""
    S = len(per_net) // G
    if isinstance(per_net[0], np.ndarray):
        return np.stack([np.stack(per_net[g * S:(g + 1) * S], axis=1) for g in range(G)])
    return torch.stack([torch.stack(per_net[g * S:(g + 1) * S], dim=1) for g in range(G)])


def net_slice(t, b, B, G):
    """net b's [N][w] view of a [G][N][B / G][w] array"""
    S = B // G
    return t[b // S][:, b % S]


def checker_all(x, nets, g_y, G):
    B = len(nets)
    ys, g_x, g_W, g_b = [], 0.0, [], []
    for b, (Ws, bs) in enumerate(nets):
        ys.append(checker_forward(x, Ws, bs)[0])
        gx, gW, gb = checker_backward(x, Ws, bs, net_slice(g_y, b, B, G))
        g_x = g_x + gx
        g_W += gW
        g_b += gb
    return [layout(ys, G), g_x] + g_W + g_b


def bank_all(bank, x, nets, g_y, G):
    tx = dev(x).requires_grad_(True)
    params = [params_of(Ws, bs) for Ws, bs in nets]
    y = bank(tx, [W for W, _ in params], [b for _, b in params], groups=G)
    leaves = [tx] + [t for W, _ in params for t in W] + [t for _, b in params for t in b]
    return [y.detach()] + list(torch.autograd.grad(y, leaves, dev(g_y)))


def torch_all(x, nets, g_y, G):
    """torch's own float32 nn.Sequentials and torch.stack on the GPU, on the same tensors"""
    seqs = [sequential_of(Ws, bs, dtype=torch.float32, device="cuda") for Ws, bs in nets]
    tx = dev(x).requires_grad_(True)
    y = layout([seq(tx) for seq in seqs], G)
    linears = [[m for m in seq if isinstance(m, torch.nn.Linear)] for seq in seqs]
    leaves = [tx] + [m.weight for net in linears for m in net] + [m.bias for net in linears for m in net]
    return [y.detach()] + list(torch.autograd.grad(y, leaves, dev(g_y)))


_reference = {}


def reference(name, N):
    """the case's tensors, the checker's results and torch's float32 results: computed once, shared, never changed"""
    key = (name, N)
    if key not in _reference:
        widths, B, G = BANKS[name]
        seed = 5000 * sorted(BANKS).index(name) + N
        nets = [make_net(widths, seed + 10 * b) for b in range(B)]
        x = make_rows(N, widths[0], seed + 1)
        g_y = make_rows(N * B, widths[-1], seed + 2).reshape(G, N, B // G, widths[-1])
        _reference[key] = (x, nets, g_y, G, checker_all(x, nets, g_y, G), torch_all(x, nets, g_y, G))
    return _reference[key]


# ---- shapes and accuracy ------------------------------------------------------------------------------------
def y_has_the_bits_of_fused_mlp(what, y, x, nets, G):
    import pigs_amd
    B = len(nets)
    for b, (Ws, bs) in enumerate(nets):
        W, bias = params_of(Ws, bs, requires=False)
        alone = pigs_amd.fused_mlp(dev(x), W, bias)
        assert torch.equal(net_slice(y, b, B, G), alone), f"{what}: y of net {b} differs from fused_mlp on that net"


@pytest.mark.parametrize("N", SIZES, ids=[f"N{n}" for n in SIZES])
@pytest.mark.parametrize("name", list(BANKS))
def test_every_bank_at_every_size(bank, name, N):
    x, nets, g_y, G, want, ref = reference(name, N)
    widths, B, _ = BANKS[name]
    got = bank_all(bank, x, nets, g_y, G)
    assert got[0].shape == (G, N, B // G, widths[-1]) and got[0].is_contiguous()
    worst = worst_ratio(f"{name} N={N}", got, ref, want)
    print(f"{name} N={N}: worst err_bank / (4 err_torch + 1e-6 scale) = {worst:.3f}")
    y_has_the_bits_of_fused_mlp(f"{name} N={N}", got[0], x, nets, G)


def test_more_tiles_than_the_forward_has_waves(bank):
    """the forward caps its grid at 2 048 waves per net: N = 16 x 2 048 + 1 makes its grid-stride loop run.  Forward only."""
    name, N = "model_b4g2", 16 * 2048 + 1
    widths, B, G = BANKS[name]
    nets = [make_net(widths, 77 + b) for b in range(B)]
    x = make_rows(N, widths[0], 76)
    params = [params_of(Ws, bs, requires=False) for Ws, bs in nets]
    y = bank(dev(x), [W for W, _ in params], [b for _, b in params], groups=G)
    want = layout([checker_forward(x, Ws, bs)[0] for Ws, bs in nets], G)
    seqs = [sequential_of(Ws, bs, dtype=torch.float32, device="cuda") for Ws, bs in nets]
    with torch.no_grad():
        ref = layout([seq(dev(x)) for seq in seqs], G)
    worst = worst_ratio(f"{name} N={N}", [y], [ref], [want])
    print(f"{name} N={N} forward: worst err_bank / (4 err_torch + 1e-6 scale) = {worst:.3f}")
    y_has_the_bits_of_fused_mlp(f"{name} N={N}", y, x, nets, G)


# ---- exactness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("widths", [(5, 3), (16, 16), (17, 33)], ids=lambda w: f"{w[0]}to{w[1]}")
@pytest.mark.parametrize("N", [1, 17, 65])
def test_one_layer_with_small_integers_is_exact(bank, widths, N, G):
    """L = 1, B = 3 DIFFERENT non-symmetric integer nets, integer x and g_y (different in every net's slot), every sum
    below 2^24: y, g_x, every g_W and g_b bit-equal to the integer results.  No swapped net, slot, group, row or column
    passes: W_b[o][i] = 3 o - 2 i + (o i) % 5 - 1 + b ((o + 2 i) % 3 + 1), b_b[o] = o % 7 - 3 + 2 b."""
    w_in, w_out = widths
    rng = np.random.default_rng(100 * N + w_in + G)
    o, i = np.meshgrid(np.arange(w_out), np.arange(w_in), indexing="ij")
    nets = []
    for b in range(3):
        W = (3 * o - 2 * i + (o * i) % 5 - 1 + b * ((o + 2 * i) % 3 + 1)).astype(np.float64)
        nets.append(([W], [(np.arange(w_out) % 7 - 3 + 2 * b).astype(np.float64)]))
    x = rng.integers(-4, 5, (N, w_in)).astype(np.float64)
    g_y = rng.integers(-3, 4, (G, N, 3 // G, w_out)).astype(np.float64)
    want = checker_all(x, nets, g_y, G)
    assert max(np.abs(t).max() for t in want) < 2 ** 22
    assert all((np.abs(np.abs(x) @ np.abs(W[0]).T).max() + 7) < 2 ** 24 for W, _ in nets)
    assert not np.array_equal(nets[0][0][0], nets[1][0][0].T) and not np.array_equal(nets[1][0][0], nets[2][0][0])
    got = bank_all(bank, x, nets, g_y, G)
    for name, g, w in zip(names_of(3), got, want):
        assert tuple(g.shape) == w.shape, name
        assert np.array_equal(host(g), w), f"{name}: {np.abs(host(g) - w).max()} off an integer result"


# ---- masking ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["model_b4g2", "17_33_47_1_b2g2", "5to3_b3g1"])
@pytest.mark.parametrize("N", [1, 17, 1611])
def test_rows_past_the_end_are_never_read_or_written(hip_lib, name, N):
    """through the C ABI with buffers of its own: x is the head of a larger buffer whose following rows are NaN, g_y lies
    in a buffer of NaN, N is no multiple of 16, and 64 sentinel elements stand behind y, g_x, every g_W / g_b and the
    scratch"""
    widths, B, G = BANKS[name]
    L, pad, sentinel = len(widths) - 1, 64, -12345.0
    nets = [make_net(widths, 300 + b) for b in range(B)]
    x = make_rows(N, widths[0], 299)
    g_y = make_rows(N * B, widths[-1], 298).reshape(G, N, B // G, widths[-1])
    want = checker_all(x, nets, g_y, G)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def padded(n):
        return torch.full((n + pad,), sentinel, device="cuda")
    tx = torch.full((N + 16, widths[0]), float("nan"), device="cuda")
    tx[:N] = dev(x)
    tg = torch.full((g_y.size + 16 * widths[-1],), float("nan"), device="cuda")
    tg[:g_y.size] = dev(g_y).reshape(-1)
    params = [params_of(Ws, bs, requires=False) for Ws, bs in nets]
    W, b = [t for Wn, _ in params for t in Wn], [t for _, bn in params for t in bn]
    w = ints(*widths)
    y = padded(g_y.size)
    rc = hip_lib.pigs_mlp_bank_forward(0, N, B, G, L, w, tx.data_ptr(), pointers(*[t.data_ptr() for t in W]),
                                       pointers(*[t.data_ptr() for t in b]), y.data_ptr(), stream)
    assert rc == 0
    nbytes = hip_lib.pigs_mlp_bank_scratch_bytes(N, B, L, w)
    scratch = padded(nbytes // 4)
    g_x = padded(N * widths[0])
    g_W, g_b = [padded(t.numel()) for t in W], [padded(t.numel()) for t in b]
    rc = hip_lib.pigs_mlp_bank_backward(0, N, B, G, L, w, tx.data_ptr(), pointers(*[t.data_ptr() for t in W]),
                                        pointers(*[t.data_ptr() for t in b]), tg.data_ptr(), scratch.data_ptr(), nbytes,
                                        g_x.data_ptr(), pointers(*[t.data_ptr() for t in g_W]),
                                        pointers(*[t.data_ptr() for t in g_b]), stream)
    assert rc == 0
    torch.cuda.synchronize()
    for what, t, ref in zip(names_of(B * L) + ["scratch"], [y, g_x] + g_W + g_b + [scratch], want + [None]):
        assert (t[-pad:] == sentinel).all(), f"{what}: written past its end"
        assert not torch.isnan(t).any(), f"{what}: a NaN of the rows past N came through"
        assert not (t[:-pad] == sentinel).any(), f"{what}: not all of it was written"
        if ref is not None:
            assert np.abs(host(t[:-pad]) - ref.reshape(-1)).max() <= 1e-4 * scale_of(ref), what


# ---- reproducibility ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["model_b4g2", "six_of_48_b2g1", "5to3_b3g1"])
def test_three_calls_give_the_same_bits(bank, name):
    x, nets, g_y, G, _, _ = reference(name, 4097)
    first = bank_all(bank, x, nets, g_y, G)
    for _ in range(2):
        for what, a, b in zip(names_of(len(first) // 2 - 1), first, bank_all(bank, x, nets, g_y, G)):
            assert torch.equal(a, b), f"{what} differs between two calls on the same inputs"


# ---- autograd -----------------------------------------------------------------------------------------------
PATTERNS = {            # x requires a gradient; the (net, layer) weights / biases that do not
    "x_only": (True, lambda b, l: True, lambda b, l: True),
    "parameters_only": (False, lambda b, l: False, lambda b, l: False),
    "one_net_frozen": (True, lambda b, l: b == 2, lambda b, l: b == 2),
    "one_layer_of_one_net_frozen": (True, lambda b, l: (b, l) == (1, 2), lambda b, l: (b, l) == (1, 2)),
    "biases_only": (False, lambda b, l: True, lambda b, l: False),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_needs_input_grad(bank, pattern):
    """a gradient that is not asked for is None, the others are bit for bit those of the full backward"""
    name, N = "model_b4g2", 333
    widths, B, G = BANKS[name]
    L = len(widths) - 1
    x, nets, g_y, _, _, _ = reference(name, 1600)
    x, g_y = x[:N], np.ascontiguousarray(g_y[:, :N])
    full = bank_all(bank, x, nets, g_y, G)[1:]
    x_requires, w_frozen, b_frozen = PATTERNS[pattern]
    tx = dev(x).requires_grad_(x_requires)
    params = [params_of(Ws, bs) for Ws, bs in nets]
    for b in range(B):
        for l in range(L):
            params[b][0][l].requires_grad_(not w_frozen(b, l))
            params[b][1][l].requires_grad_(not b_frozen(b, l))
    y = bank(tx, [W for W, _ in params], [bb for _, bb in params], groups=G)
    y.backward(dev(g_y))
    got = [tx.grad] + [t.grad for W, _ in params for t in W] + [t.grad for _, bb in params for t in bb]
    asked = 0
    for what, g, f in zip(names_of(B * L)[1:], got, full):
        if g is not None:
            asked += 1
            assert torch.equal(g, f), f"{pattern}: {what} differs from the full backward"
    expect = {"x_only": 1, "parameters_only": 2 * B * L, "one_net_frozen": 1 + 2 * (B - 1) * L,
              "one_layer_of_one_net_frozen": 1 + 2 * (B * L - 1), "biases_only": B * L}[pattern]
    assert asked == expect, (pattern, asked)


def test_leading_one_and_a_gradient_that_reads_one_group(bank):
    name, N = "model_b4g2", 100
    widths, B, G = BANKS[name]
    L = len(widths) - 1
    x, nets, g_y, _, want, _ = reference(name, 1600)
    x, g_y = x[:N], np.ascontiguousarray(g_y[:, :N])
    params = [params_of(Ws, bs) for Ws, bs in nets]
    W, bb = [p[0] for p in params], [p[1] for p in params]
    flat = bank(dev(x), W, bb, groups=G)
    tx = dev(x)[None].requires_grad_(True)
    y = bank(tx, W, bb, groups=G)
    assert y.shape == (G, N, B // G, widths[-1]) and torch.equal(y, flat.detach())
    # the loss reads y[0] alone: the gradient arrives as a strided view's, and group 1's nets get exactly zero
    (y[0] * dev(g_y[0])).sum().backward()
    assert tx.grad.shape == tx.shape
    zeroed = g_y.copy()
    zeroed[1] = 0.0
    expect = checker_all(x, nets, zeroed, G)
    grads = [tx.grad[0]] + [t.grad for p in params for t in p[0]] + [t.grad for p in params for t in p[1]]
    for what, g, w in zip(names_of(B * L)[1:], grads, expect[1:]):
        assert np.abs(host(g) - w).max() <= 1e-5 * max(scale_of(w), 1e-30), what
    for b in (2, 3):
        for t in params[b][0] + params[b][1]:
            assert not t.grad.any(), f"net {b} of the unused group has a gradient that is not zero"
    assert all(bool(t.grad.any()) for t in params[0][0] + params[1][1])


def test_bank_object_gives_grad_to_the_nets_parameters(bank):
    import pigs_amd
    name, N = "model_b4g2", 257
    widths, B, G = BANKS[name]
    x, nets, g_y, _, _, _ = reference(name, 1600)
    x, g_y = x[:N], np.ascontiguousarray(g_y[:, :N])
    want = checker_all(x, nets, g_y, G)
    seqs = [sequential_of(Ws, bs, dtype=torch.float32, device="cuda") for Ws, bs in nets]
    seqs[1] = pigs_amd.FusedMLP.from_sequential(seqs[1])                  # a FusedMLP among plain nn.Sequentials
    obj = pigs_amd.FusedMLPBank(seqs, groups=G)
    tx = dev(x)[None].requires_grad_(True)
    y = obj(tx)
    y.backward(dev(g_y))
    linears = [[m for m in seq if isinstance(m, torch.nn.Linear)] for seq in seqs]
    got = [y, tx.grad[0]] + [m.weight.grad for net in linears for m in net] + [m.bias.grad for net in linears for m in net]
    for what, g, w in zip(names_of(len(want) // 2 - 1), got, want):
        assert g is not None, f"{what}: the net's parameter received no .grad"
        assert np.abs(host(g) - w).max() <= 1e-5 * scale_of(w), what
    with torch.no_grad():                                                 # the next call sees a changed parameter
        linears[3][3].bias.add_(1.0)
    again, y = obj(tx).detach(), y.detach()
    assert float((again[1][:, 1] - (y[1][:, 1] + 1.0)).abs().max()) <= 1e-5 and torch.equal(again[0], y[0])
    assert torch.equal(again[1][:, 0], y[1][:, 0])


# ---- capture ------------------------------------------------------------------------------------------------
def test_capture_of_forward_and_backward(bank):
    """torch.cuda.graph around fused_mlp_bank and autograd.grad; three replays with x, the weights and g_y rewritten in
    place, each bit for bit the eager call on the same tensors"""
    name, N = "model_b4g2", 1600
    widths, B, G = BANKS[name]
    L = len(widths) - 1
    cases = []
    for k in range(4):
        nets = [make_net(widths, 50 + 10 * k + b) for b in range(B)]
        cases.append((make_rows(N, widths[0], 60 + k), nets,
                      make_rows(N * B, widths[-1], 70 + k).reshape(G, N, B // G, widths[-1])))

    def flat(nets):
        return [W for Ws, _ in nets for W in Ws] + [b for _, bs in nets for b in bs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leaves = [dev(a).requires_grad_(True) for a in [cases[0][0]] + flat(cases[0][1])]
        g = dev(cases[0][2])

        def step():
            W = [leaves[1 + b * L:1 + (b + 1) * L] for b in range(B)]
            bb = [leaves[1 + (B + b) * L:1 + (B + b + 1) * L] for b in range(B)]
            y = bank(leaves[0], W, bb, groups=G)
            return (y.detach(),) + torch.autograd.grad(y, leaves, g)
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 3):
        x, nets, g_y = cases[k]
        with torch.no_grad():
            for leaf, a in zip(leaves, [x] + flat(nets)):
                leaf.copy_(dev(a))
            g.copy_(dev(g_y))
        graph.replay()
        torch.cuda.synchronize()
        eager = bank_all(bank, x, nets, g_y, G)
        for what, a, b in zip(names_of(B * L), outs, eager):
            assert torch.equal(a, b), f"replay {k}: {what} differs from the eager call"
        want = checker_all(x, nets, g_y, G)
        assert np.abs(host(outs[0]) - want[0]).max() <= 1e-5 * scale_of(want[0])
        assert np.abs(host(outs[1]) - want[1]).max() <= 1e-5 * scale_of(want[1])


def aggregation(N, dtype=torch.float32):
    """a sampler with its neighbour lists built on N Gaussians, and the aggregation's other arguments (H = 2, L = K = 16)"""
    from test_aggregate_heads_gpu import cloud, head_arguments, sampler_on
    means, conics = cloud(N, dtype)
    _, T, _, _, freq, dist = [a.to(dtype).cuda() for a in head_arguments(N, 2, 16, 16, 6)]
    return sampler_on(means, conics, host="ctypes"), T, freq, dist


def test_capture_inside_a_graphed_step(bank):
    """GraphedStep over FusedMLPBank -> aggregate_neighbors_heads -> loss -> backward: three replays on new features
    against the eager step"""
    import pigs_amd
    from pigs_amd.graphs import GraphedStep
    N = 257
    smp, T, freq, dist = aggregation(N)
    seqs = [sequential_of(*make_net(MODEL, 80 + b), dtype=torch.float32, device="cuda") for b in range(4)]
    obj = pigs_amd.FusedMLPBank(seqs, groups=2)
    params = [p for seq in seqs for p in seq.parameters()]

    def fn(x):
        qk = obj(x)
        loss = torch.mean(smp.aggregate_neighbors_heads(x, T, qk[0], qk[1], freq, dist) ** 2)
        return (loss.detach(), qk.detach()) + torch.autograd.grad(loss, [x] + params)
    step = GraphedStep(fn, lambda: [dev(0.5 * make_rows(N, 16, 81)).requires_grad_(True)], warmup=2)
    for k in (1, 2, 3):
        x = dev(0.5 * make_rows(N, 16, 81 + k))
        with torch.no_grad():
            step.inputs[0].copy_(x)
        got = [t.clone() for t in step()]
        torch.cuda.synchronize()
        eager = fn(x.requires_grad_(True))
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1]), f"replay {k} differs from the eager step"
        for a, b in zip(got[2:], eager[2:]):
            assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-30), f"replay {k}: a gradient"
        assert float(got[0]) > 0


# ---- the seam to the aggregation ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 257])
def test_the_bank_feeds_the_aggregation_as_four_nets_and_two_stacks_do(bank, N):
    """aggregate_neighbors_heads(rows, T, qk[0], qk[1], ...) against the same call fed by four FusedMLPs and two
    torch.stacks: the outputs are bit-equal, because y is; the gradients at the nets' parameters and at the features
    differ by at most ONE allowance of the bar, 4 err_torch + 1e-6 scale, err_torch that of float32 nn.Sequentials in
    front of the same float32 aggregation against the whole composition in float64."""
    import pigs_amd
    nets = [make_net(MODEL, 90 + b) for b in range(4)]
    x, r = 0.5 * make_rows(N, 16, 95), make_rows(N * 2, 16, 96).reshape(N, 2, 16)

    def run(dtype, wrap, banked):
        smp, T, freq, dist = aggregation(N, dtype)
        seqs = [sequential_of(Ws, bs, dtype=dtype, device="cuda") for Ws, bs in nets]
        tx = dev(x, dtype).requires_grad_(True)
        if banked:
            qk = pigs_amd.FusedMLPBank(seqs, groups=2)(tx)
            q, k = qk[0], qk[1]
        else:
            mods = [wrap(s) for s in seqs]
            q, k = torch.stack([m(tx) for m in mods[:2]], dim=1), torch.stack([m(tx) for m in mods[2:]], dim=1)
        out = smp.aggregate_neighbors_heads(tx, T, q, k, freq, dist)
        leaves = [tx] + [p for s in seqs for p in s.parameters()]
        return [out.detach()] + list(torch.autograd.grad(out, leaves, dev(r, dtype)))
    want = run(torch.float64, lambda s: s, False)
    ref32 = run(torch.float32, lambda s: s, False)
    four = run(torch.float32, pigs_amd.FusedMLP.from_sequential, False)
    got = run(torch.float32, None, True)
    assert torch.equal(got[0], four[0]) and bool(got[0].any()), "the aggregation's output differs"
    worst = 0.0
    for k, (g, f, t, w) in enumerate(zip(got, four, ref32, want)):
        w = host(w)
        bound = 4.0 * np.abs(host(t) - w).max() + 1e-6 * scale_of(w)
        diff = np.abs(host(g) - host(f)).max()
        worst = max(worst, diff / bound)
        assert diff <= bound, f"tensor {k}: the two routes differ by {diff:.3g}, one allowance is {bound:.3g}"
    print(f"seam N={N}: the routes differ by at most {worst:.3f} of one allowance")
