"""CPU: the bank of fused MLPs (pigs_amd/mlp.py fused_mlp_bank / FusedMLPBank, csrc/mlp_bank.hip) -- the C ABI (symbols,
refusals, scratch size) and the Python surface's refusals and bookkeeping.  No GPU call is made here; the checker and the
helpers are those of tests/test_mlp.py.
"""
import ctypes
import os
import re

import pytest
import torch

from test_mlp import NETS, ROOT, UNSUPPORTED, ints, pointers

NAMES = ("pigs_mlp_bank_scratch_bytes", "pigs_mlp_bank_forward", "pigs_mlp_bank_backward")
MAX_NETS = 8


def test_symbols_declared_exported_and_bound(hip_lib):
    from pigs_amd import _lib
    text = open(os.path.join(ROOT, "include", "pigs_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name       # one ctypes type per parameter
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"#define\s+PIGS_MLP_BANK_MAX_NETS\s+%d\b" % MAX_NETS, header)
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION                       # additive: no number change
    assert _lib.SIGNATURES["pigs_mlp_bank_scratch_bytes"][0] is ctypes.c_size_t


def test_scratch_size(hip_lib):
    """B times the records of pigs_mlp_scratch_bytes (at most 256 waves PER NET), then B - 1 parts of g_x [N][w_0]:
    monotone in N (the records up to their cap), monotone in B, 0 when unsupported"""
    size, one = hip_lib.pigs_mlp_bank_scratch_bytes, hip_lib.pigs_mlp_scratch_bytes
    for widths in NETS.values():
        w, L = ints(*widths), len(widths) - 1
        for B in range(1, MAX_NETS + 1):
            last = 0
            for N in (1, 15, 16, 17, 1600, 4095, 4096, 4097, 65536, 1 << 24):
                got = size(N, B, L, w)
                assert got == B * one(N, L, w) + (B - 1) * N * widths[0] * 4, (widths, B, N)
                assert got >= last and got >= size(N, max(B - 1, 1), L, w)
                last = got
            assert size(0, B, L, w) == 0 and size(-5, B, L, w) == 0
        # B = 1: the records alone, capped as one net's
        assert size(4096, 1, L, w) == size(1 << 30, 1, L, w) == one(4096, L, w)
        for N in (1, 1600, 4097):
            assert size(N, 1, L, w) >= one(N, L, w)
        assert size(16, 0, L, w) == 0 and size(16, MAX_NETS + 1, L, w) == 0 and size(16, -1, L, w) == 0
    assert size(16, 2, 0, ints(4)) == 0 and size(16, 2, 7, ints(*[4] * 8)) == 0
    assert size(16, 2, 1, ints(0, 4)) == 0 and size(16, 2, 1, ints(4, 49)) == 0 and size(16, 2, 1, None) == 0


def test_abi_refusals_come_before_any_hip_call(hip_lib):
    """device pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some = None, 1 << 12
    fwd, bwd = hip_lib.pigs_mlp_bank_forward, hip_lib.pigs_mlp_bank_backward

    def arrays(B, L, W=True, b=True, hole=None):
        Wp, bp = [some] * (B * L), [some] * (B * L)
        if hole == "W":
            Wp[-1] = null
        if hole == "b":
            bp[L] = null                                   # net 1's first layer
        return (pointers(*Wp) if W else None), (pointers(*bp) if b else None)

    def forward(dtype=0, N=4, B=4, G=2, widths=(5, 7, 3), x=some, W=True, b=True, y=some, hole=None):
        L = len(widths) - 1
        Wp, bp = arrays(max(B, 0), L, W, b, hole)
        return fwd(dtype, N, B, G, L, ints(*widths) if widths else None, x, Wp, bp, y, None)
    assert forward(dtype=1) == 2 and forward(dtype=7) == 2                         # float64, no such dtype
    assert forward(B=0) == 2 and forward(B=9, G=1) == 2 and forward(B=-1, G=1) == 2
    assert forward(G=0) == 1 and forward(G=3) == 1 and forward(G=-2) == 1 and forward(G=8) == 1
    assert forward(widths=(0, 4)) == 2 and forward(widths=(4, 49)) == 2 and forward(widths=(4, 0, 4)) == 2
    assert forward(widths=(49, 4)) == 2
    assert fwd(0, 4, 4, 2, 0, ints(4), some, pointers(*[some] * 4), pointers(*[some] * 4), some, None) == 2      # L = 0
    assert forward(widths=(4,) * 8) == 2                                           # L = 7
    assert forward(widths=(4,) * 7, x=null) == 1                                   # L = 6 passes the size checks
    assert forward(B=8, G=8, x=null) == 1 and forward(B=1, G=1, x=null) == 1       # B = 1 and 8 pass them too
    assert forward(N=0) == 1 and forward(N=-3) == 1
    assert fwd(0, 4, 2, 1, 1, None, some, pointers(some, some), pointers(some, some), some, None) == 1           # no widths
    assert forward(x=null) == 1 and forward(W=False) == 1 and forward(b=False) == 1 and forward(y=null) == 1
    assert forward(hole="W") == 1 and forward(hole="b") == 1                       # a null entry

    def backward(dtype=0, N=4, B=4, G=2, widths=(5, 7, 3), x=some, g_y=some, scratch=some, nbytes=1 << 24, g_x=some,
                 gW=True, gb=True, hole=None):
        L = len(widths) - 1
        Wp, bp = arrays(max(B, 0), L, hole=hole)
        k = max(B, 0) * L
        return bwd(dtype, N, B, G, L, ints(*widths), x, Wp, bp, g_y, scratch, nbytes, g_x,
                   pointers(*[some] * k) if gW else None, pointers(*[some] * k) if gb else None, None)
    assert backward(dtype=1) == 2 and backward(widths=(5, 49, 3)) == 2 and backward(widths=(4,) * 8) == 2
    assert backward(B=0) == 2 and backward(B=9, G=1) == 2 and backward(G=0) == 1 and backward(G=3) == 1
    assert backward(N=0) == 1 and backward(x=null) == 1 and backward(g_y=null) == 1
    assert backward(hole="W") == 1 and backward(hole="b") == 1
    assert backward(g_x=null, gW=False, gb=False) == 1                             # no gradient wanted
    nulls = pointers(*[null] * 8)
    assert bwd(0, 4, 4, 2, 2, ints(5, 7, 3), some, *arrays(4, 2), some, some, 1 << 24, null, nulls, nulls, None) == 1
    need = hip_lib.pigs_mlp_bank_scratch_bytes(4, 4, 2, ints(5, 7, 3))
    assert need == 4 * 4 * (7 * 6 + 3 * 8) + 3 * 4 * 5 * 4
    assert backward(nbytes=need - 1) == 1 and backward(nbytes=0) == 1              # a short scratch
    assert backward(scratch=null) == 1 and backward(scratch=some + 2) == 1         # none, or off its alignment
    assert backward(scratch=null, gW=False) == 1                                   # a bias gradient alone needs it too
    assert backward(scratch=null, gW=False, gb=False) == 1                         # and so does g_x of more than one net
    assert backward(nbytes=need - 1, gW=False, gb=False) == 1
    for N, records in ((4097, 256), (1600, 100)):
        assert backward(N=N, nbytes=4 * records * 4 * (7 * 6 + 3 * 8) + 3 * N * 5 * 4 - 1) == 1


# ---- the Python surface -------------------------------------------------------------------------------------
def test_fused_mlp_bank_refuses_cpu_tensors_and_bad_arguments(hip_lib):
    import pigs_amd
    f = pigs_amd.fused_mlp_bank

    def net(w_in=5, w_mid=6, w_out=3):
        return [torch.zeros(w_mid, w_in), torch.zeros(w_out, w_mid)], [torch.zeros(w_mid), torch.zeros(w_out)]
    x = torch.zeros(4, 5)
    W, b = zip(*[net() for _ in range(4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, W, b, groups=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x[None], W, b)
    with pytest.raises(TypeError):
        f(x.numpy(), W, b)
    with pytest.raises(TypeError):
        f(x.double(), W, b)
    for groups in (0, 3, 8, -1, 2.0):
        with pytest.raises(ValueError, match="groups"):
            f(x, W, b, groups=groups)
    W9, b9 = zip(*[net() for _ in range(9)])
    with pytest.raises(NotImplementedError, match="9 nets"):
        f(x, W9, b9)
    with pytest.raises(NotImplementedError, match="0 nets"):
        f(x, [], [])
    with pytest.raises(ValueError):
        f(x, W, b[:3])
    # nets whose shapes differ: the first differing net and layer are named
    odd = net(w_out=4)
    with pytest.raises(ValueError, match=r"net 2, layer 1\b"):
        f(x, [W[0], W[1], odd[0], net(w_mid=7)[0]], [b[0], b[1], odd[1], net(w_mid=7)[1]])
    with pytest.raises(ValueError, match=r"net 1, layer 0\b"):
        f(x, [W[0], net(w_mid=7)[0]], [b[0], net(w_mid=7)[1]])
    with pytest.raises(ValueError, match="net 3 has 1 weights"):
        f(x, [W[0], W[1], W[2], W[3][:1]], [b[0], b[1], b[2], b[3][:1]])
    with pytest.raises(ValueError, match="net 0 has 2 weights and 1 biases"):
        f(x, [W[0], W[1]], [b[0][:1], b[1]])
    with pytest.raises(ValueError, match=r"net 1, layer 1\b"):                      # the weights agree, a bias does not
        f(x, [W[0], W[1]], [b[0], [b[1][0], torch.zeros(4)]])
    with pytest.raises(NotImplementedError):                                        # the refusals of one net hold per net
        wide = ([torch.zeros(49, 5)], [torch.zeros(49)])
        f(x, [wide[0]] * 2, [wide[1]] * 2)
    with pytest.raises(ValueError):
        f(torch.zeros(0, 5), W, b)
    with pytest.raises(ValueError):
        f(torch.zeros(2, 4, 5), W, b)


class TwoLists(torch.nn.Module):
    """the model's way of keeping the nets: two nn.ParameterLists of nn.Sequentials (model_pn.py:203-226)"""

    def __init__(self, heads=2, width=16, layers=4):
        super().__init__()
        nn = torch.nn

        def net():
            mods = []
            for l in range(layers):
                mods += [nn.Linear(width, width)] + ([nn.Tanh()] if l + 1 < layers else [])
            return nn.Sequential(*mods)
        self.query_transform = nn.ParameterList([net() for _ in range(heads)])
        self.key_transform = nn.ParameterList([net() for _ in range(heads)])


def test_bank_registers_nothing_and_reads_the_parameters_at_call_time(hip_lib):
    import pigs_amd
    model = TwoLists()
    keys, params = list(model.state_dict()), list(model.parameters())
    assert len(keys) == 32
    model.qk_bank = pigs_amd.FusedMLPBank([*model.query_transform, *model.key_transform], groups=2)
    assert not isinstance(model.qk_bank, torch.nn.Module)
    assert list(model.state_dict()) == keys                                         # keys and order
    after = list(model.parameters())
    assert len(after) == len(params) and all(a is b for a, b in zip(after, params))          # the same objects, no duplicate
    assert [n for n, _ in model.named_modules() if "qk_bank" in n] == []

    nets = [*model.query_transform, *model.key_transform]
    W, b = model.qk_bank.arguments()
    assert len(W) == len(b) == 4 and all(len(w) == 4 for w in W)
    for n in range(4):
        for l in range(4):
            assert W[n][l] is nets[n][2 * l].weight and b[n][l] is nets[n][2 * l].bias
    # load_state_dict and an in-place step are seen by the next call's arguments
    model.load_state_dict({k: torch.full_like(v, 0.25) for k, v in model.state_dict().items()})
    W, b = model.qk_bank.arguments()
    assert all(bool((t == 0.25).all()) for net in W + b for t in net)
    with torch.no_grad():
        model.key_transform[1][6].bias.add_(1.0)
    assert bool((model.qk_bank.arguments()[1][3][3] == 1.25).all())
    # a replaced Parameter object is seen too
    model.query_transform[0][0].weight = torch.nn.Parameter(torch.ones(16, 16))
    assert model.qk_bank.arguments()[0][0][0] is model.query_transform[0][0].weight
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.qk_bank(torch.zeros(4, 16))
    # FusedMLP-wrapped nets are taken as well, and from_sequentials is the same constructor
    fused = [pigs_amd.FusedMLP.from_sequential(n) for n in nets]
    bank = pigs_amd.FusedMLPBank.from_sequentials(fused, groups=1)
    assert bank.groups == 1 and bank.arguments()[0][2][1] is nets[2][2].weight


def test_bank_refusals(hip_lib):
    import pigs_amd
    nn = torch.nn
    Bank = pigs_amd.FusedMLPBank

    def good():
        return nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 4))
    with pytest.raises(TypeError, match="net 1.*Linear"):
        Bank([good(), nn.Linear(4, 4)])
    with pytest.raises(TypeError, match="net 0"):
        Bank([[nn.Linear(4, 4)]])
    with pytest.raises(NotImplementedError, match="0 nets"):
        Bank([])
    with pytest.raises(NotImplementedError, match="9 nets"):
        Bank([good() for _ in range(9)])
    for groups in (0, 3, 5, -1):
        with pytest.raises(ValueError, match="groups"):
            Bank([good() for _ in range(4)], groups=groups)
    with pytest.raises(ValueError, match=r"net 2, layer 1\b"):
        Bank([good(), good(), nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 5)), good()])
    with pytest.raises(ValueError, match="net 1 has 1 nn.Linear"):
        Bank([good(), nn.Sequential(nn.Linear(4, 4))])


@pytest.mark.parametrize("what", list(UNSUPPORTED), ids=[k.replace(" ", "_").replace("=", "_") for k in UNSUPPORTED])
def test_bank_refuses_unsupported_nets_by_name(hip_lib, what):
    import pigs_amd
    good = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Tanh(), torch.nn.Linear(4, 4))
    with pytest.raises(NotImplementedError, match="net 1: .*" + re.escape(what)):
        pigs_amd.FusedMLPBank([good, UNSUPPORTED[what](torch.nn)])
