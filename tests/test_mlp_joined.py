"""CPU: fused_mlp_joined (pigs_amd/mlp.py, csrc/mlp_joined.hip) -- its float64 numpy checker against torch autograd through
cat + nn.Sequential + the block means in float64, the C ABI (symbols, refusals, scratch size) and the wrapper's refusals.
No GPU call is made here.

The checker, shared with tests/test_mlp_joined_gpu.py, is written from the operator's statement:
    y = net(cat(parts));   m[j] = mean over the N rows and block j's w_p / b_p columns of x^2
    g_part_p[row][k] = dA_0[row][K_p + k] + g_m[block(k)] 2 x[row][k] / (N w_p / b_p)
on top of tests/test_mlp.py's checker of the net itself.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_mlp import NETS, checker_backward, checker_forward, ints, make_net, make_rows, pointers, scale_of, sequential_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (net, the parts' widths, the blocks or None)
CASES = {
    "model": ("delta_net_c2", (16, 32), (0, 2)),
    "three_parts": ("delta_net_c2", (16, 16, 16), (0, 1, 1)),
    "one_column_blocks": ("5to3", (2, 3), (2, 3)),
    "straddles": ("17_33_47_1", (13, 4), (0, 2)),
    "one_part": ("48to48", (48,), (3,)),
    "four_parts_no_blocks": ("48to48", (1, 1, 45, 1), None),
    "six_layers": ("six_of_48", (24, 24), (1, 1)),
}


def block_count(blocks):
    return sum(blocks) if blocks else 0


def split(x, part_widths):
    """the parts of a row array, as contiguous arrays"""
    edges = np.cumsum((0,) + tuple(part_widths))
    return [np.ascontiguousarray(x[:, a:b]) for a, b in zip(edges[:-1], edges[1:])]


def checker_joined(parts, Ws, bs, blocks, g_y, g_m, mistake=None):
    """(y, m, [g_part_p], [g_W_l], [g_b_l]) in float64; g_y or g_m may be None (zero); m is [0] without blocks.
    ``mistake``: "divisor_without_N" forms the block divisor from the columns alone; "g_m_on_the_wrong_part" adds the block
    means' gradient to the part after the one it belongs to."""
    x = np.concatenate(parts, axis=1)
    N = x.shape[0]
    y, _ = checker_forward(x, Ws, bs)
    g_x, g_W, g_b = checker_backward(x, Ws, bs, g_y if g_y is not None else np.zeros_like(y))
    m, extra, j, K = [], np.zeros_like(x), 0, 0
    P = len(parts)
    for p, part in enumerate(parts):
        w, nb = part.shape[1], (blocks[p] if blocks else 0)
        for q in range(nb):
            cols = w // nb
            blk = part[:, q * cols:(q + 1) * cols]
            divisor = float(cols) if mistake == "divisor_without_N" else float(N * cols)
            m.append((blk ** 2).sum() / divisor)
            if g_m is not None:
                if mistake == "g_m_on_the_wrong_part":
                    wrong = (p + 1) % P
                    Kw = sum(t.shape[1] for t in parts[:wrong])
                    c = min(cols, parts[wrong].shape[1])
                    extra[:, Kw:Kw + c] += g_m[j] * 2.0 * blk[:, :c] / divisor
                else:
                    extra[:, K + q * cols:K + (q + 1) * cols] += g_m[j] * 2.0 * blk / divisor
            j += 1
        K += w
    return y, np.array(m), split(g_x + extra, [t.shape[1] for t in parts]), g_W, g_b


def torch_joined(parts, Ws, bs, blocks, g_y, g_m, dtype=torch.float64, device="cpu"):
    """the same through torch: cat, nn.Sequential, slices, pow, mean; autograd of <g_y, y> + <g_m, m>"""
    seq = sequential_of(Ws, bs, dtype=dtype, device=device)
    tp = [torch.tensor(t, dtype=dtype, device=device, requires_grad=True) for t in parts]
    x = torch.cat(tp, dim=-1)
    y = seq(x)
    ms = []
    for p, t in enumerate(tp):
        nb = blocks[p] if blocks else 0
        for q in range(nb):
            cols = t.shape[1] // nb
            ms.append(t[:, q * cols:(q + 1) * cols].pow(2).mean())
    m = torch.stack(ms) if ms else torch.zeros(0, dtype=dtype, device=device)
    loss = (y * torch.tensor(g_y, dtype=dtype, device=device)).sum()
    if ms:
        loss = loss + (m * torch.tensor(g_m, dtype=dtype, device=device)).sum()
    linears = [mod for mod in seq if isinstance(mod, torch.nn.Linear)]
    grads = torch.autograd.grad(loss, tp + [mod.weight for mod in linears] + [mod.bias for mod in linears])
    P, L = len(tp), len(linears)
    return y.detach(), m.detach(), list(grads[:P]), list(grads[P:P + L]), list(grads[P + L:])


def flat(result):
    """[(name, array)] of a checker_joined / torch_joined result"""
    y, m, g_parts, g_W, g_b = result
    out = [("y", y), ("m", m)] + [(f"g_part[{p}]", g) for p, g in enumerate(g_parts)]
    return out + [(f"g_W[{l}]", g) for l, g in enumerate(g_W)] + [(f"g_b[{l}]", g) for l, g in enumerate(g_b)]


def case_arrays(name, N, dtype=np.float32):
    net, part_widths, blocks = CASES[name]
    widths = NETS[net]
    seed = 7000 + 100 * sorted(CASES).index(name) + N
    Ws, bs = make_net(widths, seed, dtype)
    parts = split(make_rows(N, widths[0], seed + 1, dtype), part_widths)
    g_y = make_rows(N, widths[-1], seed + 2, dtype)
    g_m = make_rows(1, max(block_count(blocks), 1), seed + 3, dtype)[0][:block_count(blocks)]
    return parts, Ws, bs, blocks, g_y, g_m


def worst_difference(got, want):
    worst = 0.0
    for (name, a), (_, b) in zip(got, want):
        b = b.numpy() if isinstance(b, torch.Tensor) else b
        assert a.shape == b.shape, name
        if b.size:
            worst = max(worst, float(np.abs(a - b).max()) / scale_of(b))
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_checker_agrees_with_torch_autograd(name):
    """float64 on the CPU, N = 37: y, m and every gradient at 1e-12 of each tensor's scale"""
    args = case_arrays(name, 37, np.float64)
    worst = worst_difference(flat(checker_joined(*args)), flat(torch_joined(*args)))
    print(f"joined checker vs torch autograd, {name}: worst {worst:.3g} of a tensor's scale")
    assert worst <= 1e-12


@pytest.mark.parametrize("mistake", ["divisor_without_N", "g_m_on_the_wrong_part"])
def test_a_planted_mistake_fails_that_comparison(mistake):
    args = case_arrays("model", 37, np.float64)
    worst = worst_difference(flat(checker_joined(*args, mistake=mistake)), flat(torch_joined(*args)))
    print(f"{mistake}: {worst:.3g} of a tensor's scale off torch autograd")
    assert worst > 1e-3


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_mlp_joined_scratch_bytes", "pigs_mlp_joined_forward", "pigs_mlp_joined_backward")


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
    assert _lib.SIGNATURES["pigs_mlp_joined_scratch_bytes"][0] is ctypes.c_size_t
    assert "#define PIGS_MLP_JOINED_MAX_PARTS 4" in header


def test_scratch_is_nothing_without_block_means_and_monotone_in_n(hip_lib):
    """forward: one record of w_0 column sums per wave, one wave per 16 rows, at most 2 048 waves, and only with a block
    wanted; backward: pigs_mlp_scratch_bytes, which a caller needs only with a weight or bias gradient wanted"""
    size = hip_lib.pigs_mlp_joined_scratch_bytes
    for net, part_widths, blocks in CASES.values():
        widths = NETS[net]
        w, L, P = ints(*widths), len(widths) - 1, len(part_widths)
        b = ints(*blocks) if blocks else None
        last_f = last_b = 0
        for N in (1, 15, 16, 17, 1600, 4097, 32768, 32769, 65536, 1 << 30):
            fwd, bwd = size(N, L, w, P, b, 0), size(N, L, w, P, b, 1)
            assert fwd == (min((N + 15) // 16, 2048) * widths[0] * 4 if block_count(blocks) else 0), (net, N)
            assert bwd == hip_lib.pigs_mlp_scratch_bytes(N, L, w)
            assert fwd >= last_f and bwd >= last_b
            last_f, last_b = fwd, bwd
        assert size(1600, L, w, P, None, 0) == 0 and size(1600, L, w, P, ints(*[0] * P), 0) == 0
        assert size(0, L, w, P, b, 0) == 0 and size(-1, L, w, P, b, 1) == 0
        assert size(16, L, w, 0, b, 0) == 0 and size(16, L, w, 5, b, 1) == 0
    assert size(16, 1, ints(4, 49), 1, ints(1), 0) == 0 and size(16, 1, None, 1, ints(1), 1) == 0


def test_abi_refusals_come_before_any_pointer_is_read(hip_lib):
    """device pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some = None, 1 << 12
    fwd, bwd = hip_lib.pigs_mlp_joined_forward, hip_lib.pigs_mlp_joined_backward
    UNSUPPORTED, INVALID = 2, 1

    def forward(dtype=0, N=4, widths=(5, 7, 3), pw=(2, 3), parts=(some, some), blocks=(1, 3), W=True, b=True,
                scratch=some, nbytes=1 << 20, y=some, m=some, P=None, hole=None, no_widths=False, no_pw=False):
        L = len(widths) - 1
        Wp, bp = [some] * L, [some] * L
        if hole == "W":
            Wp[-1] = null
        if hole == "b":
            bp[0] = null
        return fwd(dtype, N, L, None if no_widths else ints(*widths), len(pw) if P is None else P,
                   None if no_pw else ints(*pw), pointers(*parts) if parts else None, ints(*blocks) if blocks else None,
                   pointers(*Wp) if W else None, pointers(*bp) if b else None, scratch, nbytes, y, m, None)
    assert forward(dtype=1) == UNSUPPORTED and forward(dtype=7) == UNSUPPORTED               # float64, no such dtype
    assert forward(P=0) == UNSUPPORTED and forward(P=5) == UNSUPPORTED
    assert forward(pw=(1,) * 5, parts=(some,) * 5, blocks=None) == UNSUPPORTED
    assert forward(pw=(0, 5)) == UNSUPPORTED and forward(widths=(49, 3), pw=(49,), parts=(some,), blocks=None) == UNSUPPORTED
    assert forward(widths=(48, 3), pw=(49,), parts=(some,), blocks=None) == UNSUPPORTED      # a part too wide
    assert forward(widths=(5, 49, 3)) == UNSUPPORTED and forward(widths=(5, 0)) == UNSUPPORTED
    assert forward(widths=(5,) * 8) == UNSUPPORTED                                            # L = 7
    assert fwd(0, 4, 0, ints(5), 2, ints(2, 3), pointers(some, some), None, pointers(some), pointers(some), null, 0, some,
               null, None) == UNSUPPORTED                                                     # L = 0
    assert forward(widths=(48, 3), pw=(24, 24), blocks=(6, 3)) == UNSUPPORTED                 # nine blocks
    assert forward(widths=(48, 3), pw=(24, 24), blocks=(6, 2), y=null) == INVALID             # eight pass the size checks
    assert forward(N=0) == INVALID and forward(N=-3) == INVALID
    assert forward(pw=(2, 2)) == INVALID and forward(pw=(3, 3)) == INVALID                    # do not add up to w_0
    assert forward(blocks=(1, 2)) == INVALID and forward(blocks=(-1, 3)) == INVALID           # 2 does not divide 3
    assert forward(no_widths=True) == INVALID and forward(no_pw=True) == INVALID
    assert forward(parts=None) == INVALID and forward(parts=(some, null)) == INVALID
    assert forward(W=False) == INVALID and forward(b=False) == INVALID and forward(y=null) == INVALID
    assert forward(hole="W") == INVALID and forward(hole="b") == INVALID
    assert forward(m=null) == INVALID                                                         # blocks wanted, nowhere to go
    need = hip_lib.pigs_mlp_joined_scratch_bytes(4, 2, ints(5, 7, 3), 2, ints(1, 3), 0)
    assert need == 4 * 5
    assert forward(scratch=null) == INVALID and forward(scratch=some + 2) == INVALID and forward(nbytes=need - 1) == INVALID
    assert forward(N=1 << 20, nbytes=2048 * 20 - 1) == INVALID

    def backward(dtype=0, N=4, widths=(5, 7, 3), pw=(2, 3), parts=(some, some), blocks=(1, 3), g_y=some, g_m=some,
                 scratch=some, nbytes=1 << 20, g_parts=(some, some), gW=True, gb=True, P=None, hole=None):
        L = len(widths) - 1
        Wp = [some] * L
        if hole == "W":
            Wp[0] = null
        return bwd(dtype, N, L, ints(*widths), len(pw) if P is None else P, ints(*pw), pointers(*parts) if parts else None,
                   ints(*blocks) if blocks else None, pointers(*Wp), pointers(*[some] * L), g_y, g_m, scratch, nbytes,
                   pointers(*g_parts) if g_parts else None, pointers(*[some] * L) if gW else None,
                   pointers(*[some] * L) if gb else None, None)
    assert backward(dtype=1) == UNSUPPORTED and backward(widths=(5, 49, 3)) == UNSUPPORTED and backward(P=5) == UNSUPPORTED
    assert backward(widths=(48, 3), pw=(24, 24), blocks=(8, 1)) == UNSUPPORTED
    assert backward(N=0) == INVALID and backward(pw=(2, 4)) == INVALID and backward(blocks=(1, 2)) == INVALID
    assert backward(parts=(null, some)) == INVALID and backward(hole="W") == INVALID
    assert backward(g_y=null, g_m=null) == INVALID                                            # nothing comes in
    assert backward(blocks=None, g_m=some) == INVALID                                         # g_m of no block
    assert backward(g_parts=None, gW=False, gb=False) == INVALID                              # nothing wanted
    assert backward(g_parts=(null, null), gW=False, gb=False) == INVALID
    need = hip_lib.pigs_mlp_joined_scratch_bytes(4, 2, ints(5, 7, 3), 2, ints(1, 3), 1)
    assert need == 4 * (7 * 6 + 3 * 8)
    assert backward(nbytes=need - 1) == INVALID and backward(scratch=null) == INVALID
    assert backward(scratch=some + 2) == INVALID and backward(scratch=null, gW=False) == INVALID
    assert backward(N=4097, nbytes=256 * need - 1) == INVALID


# ---- the Python surface -------------------------------------------------------------------------------------
def test_fused_mlp_joined_refuses_by_part(hip_lib):
    import pigs_amd
    f = pigs_amd.fused_mlp_joined
    a, b, W, bias = torch.zeros(4, 2), torch.zeros(4, 3), [torch.zeros(3, 5)], [torch.zeros(3)]
    with pytest.raises(RuntimeError, match=r"parts\[0\].*no CPU fallback"):
        f((a, b), W, bias)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f((a[None], b.reshape(4, 3, 1)), W, bias, block_means=(0, 3))
    with pytest.raises(ValueError, match=r"parts\[1\].*rows"):
        f((a, torch.zeros(5, 3)), W, bias)                                     # mismatched N
    with pytest.raises(ValueError, match=r"parts\[1\] must be contiguous"):
        f((a, torch.zeros(4, 6)[:, ::2]), W, bias)
    with pytest.raises(ValueError, match="add up to 4"):
        f((a, a), W, bias)                                                     # 2 + 2 columns, weights[0] takes 5
    with pytest.raises(ValueError, match="block_means has 1 entries for 2 parts"):
        f((a, b), W, bias, block_means=(1,))
    with pytest.raises(ValueError, match=r"block_means\[1\] = 2 does not divide parts\[1\]'s 3 columns"):
        f((a, b), W, bias, block_means=(1, 2))
    with pytest.raises(ValueError, match=r"block_means\[0\]"):
        f((a, b), W, bias, block_means=(-1, 3))
    with pytest.raises(NotImplementedError, match="9 blocks"):
        f((torch.zeros(4, 24), torch.zeros(4, 24)), [torch.zeros(3, 48)], bias, block_means=(6, 3))
    with pytest.raises(TypeError, match=r"parts\[0\].*float32 only"):
        f((a.double(), b.double()), [W[0].double()], [bias[0].double()])       # float64 is not built
    with pytest.raises(TypeError, match=r"parts\[1\].*float32 only"):
        f((a, b.double()), W, bias)
    with pytest.raises(TypeError, match="float32 only"):
        f((a, b), [W[0].double()], bias)
    with pytest.raises(TypeError, match=r"parts\[1\]"):
        f((a, b.numpy()), W, bias)
    with pytest.raises(NotImplementedError, match="5 parts"):
        f((a[:, :1],) * 5, W, bias)
    with pytest.raises(NotImplementedError, match="0 parts"):
        f((), W, bias)
    with pytest.raises(NotImplementedError, match=r"parts\[0\].*49 columns"):
        f((torch.zeros(4, 49),), [torch.zeros(3, 49)], bias)
    with pytest.raises(ValueError, match=r"parts\[0\]"):
        f((torch.zeros(4), b), W, bias)                                        # no columns
    with pytest.raises(NotImplementedError):
        f((a, b), [torch.zeros(5, 5)] * 7, [torch.zeros(5)] * 7)               # seven layers


def test_joined_leaves_the_module_as_it_is(hip_lib):
    import pigs_amd
    nn = torch.nn
    seq = nn.Sequential(nn.Linear(48, 32), nn.Tanh(), nn.Linear(32, 7))
    keys, params = list(seq.state_dict()), list(seq.parameters())
    net = pigs_amd.FusedMLP.from_sequential(seq)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.joined((torch.zeros(1, 4, 16), torch.zeros(4, 2, 16)), block_means=(0, 2))
    with pytest.raises(ValueError, match="add up to 32"):
        net.joined((torch.zeros(4, 16), torch.zeros(4, 16)))
    assert list(net.state_dict()) == keys
    assert len(list(net.parameters())) == len(params) and all(a is b for a, b in zip(net.parameters(), params))
    assert pigs_amd.fused_mlp_joined is pigs_amd.mlp.fused_mlp_joined
