"""CPU: fused_mlp (pigs_amd/mlp.py, csrc/mlp.hip) -- its float64 numpy checker against torch autograd through an
nn.Sequential in float64, the C ABI (symbols, refusals, scratch size) and the wrapper's refusals.  No GPU call is made here.

The checker, shared with tests/test_mlp_gpu.py:
    make_net()           weights and biases with nn.Linear's initialisation range, float64 numpy holding float32 values
    checker_forward()    y and the activations a_0 .. a_{L-1}
    checker_backward()   g_x, [g_W_l], [g_b_l] in closed form
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the dynamics network's per-Gaussian nets (model_pn.py:154-174, 187-198, 203-226; d = 2)
MODEL_NETS = {
    "input_projection_c1": (12, 16, 32, 48, 16),
    "input_projection_ns": (18, 16, 32, 48, 16),
    "input_projection_wave": (19, 16, 32, 48, 16),
    "query_key": (16, 16, 16, 16, 16),
    "delta_net_c1": (48, 32, 16, 16, 48, 32, 6),
    "delta_net_c2": (48, 32, 16, 16, 48, 32, 7),
}
EDGE_NETS = {
    "1to1": (1, 1),
    "5to3": (5, 3),
    "17_33_47_1": (17, 33, 47, 1),
    "48to48": (48, 48),
    "six_of_48": (48,) * 7,
}
NETS = {**MODEL_NETS, **EDGE_NETS}


def make_net(widths, seed, dtype=np.float32):
    """W_l, b_l uniform in +-1 / sqrt(w_l), nn.Linear's own range; values of ``dtype`` held in float64"""
    rng = np.random.default_rng(seed)
    Ws, bs = [], []
    for w_in, w_out in zip(widths[:-1], widths[1:]):
        k = 1.0 / np.sqrt(w_in)
        Ws.append(rng.uniform(-k, k, (w_out, w_in)).astype(dtype).astype(np.float64))
        bs.append(rng.uniform(-k, k, (w_out,)).astype(dtype).astype(np.float64))
    return Ws, bs


def make_rows(N, width, seed, dtype=np.float32):
    return np.random.default_rng(seed).standard_normal((N, width)).astype(dtype).astype(np.float64)


def checker_forward(x, Ws, bs):
    """(y, [a_0 .. a_{L-1}]): tanh after every layer but the last"""
    acts, a = [], x
    for l, (W, b) in enumerate(zip(Ws, bs)):
        acts.append(a)
        z = a @ W.T + b
        a = np.tanh(z) if l + 1 < len(Ws) else z
    return a, acts


def checker_backward(x, Ws, bs, g_y):
    """(g_x, [g_W_l], [g_b_l]) of <g_y, y>"""
    _, acts = checker_forward(x, Ws, bs)
    L = len(Ws)
    g_W, g_b = [None] * L, [None] * L
    dz = g_y
    for l in range(L - 1, -1, -1):
        g_W[l] = dz.T @ acts[l]
        g_b[l] = dz.sum(axis=0)
        da = dz @ Ws[l]
        if l:
            dz = da * (1.0 - acts[l] ** 2)          # a_l = tanh(z_{l-1})
    return da, g_W, g_b


def scale_of(a):
    a = np.asarray(a)
    return max(float(np.abs(a).max()), 1e-300) if a.size else 1e-300


def sequential_of(Ws, bs, dtype=torch.float64, device="cpu"):
    """the nn.Sequential of the same net: Linear, Tanh, ..., Linear"""
    mods = []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        lin = torch.nn.Linear(W.shape[1], W.shape[0], dtype=dtype, device=device)
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(W, dtype=dtype))
            lin.bias.copy_(torch.as_tensor(b, dtype=dtype))
        mods.append(lin)
        if l + 1 < len(Ws):
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("name", list(NETS))
def test_checker_agrees_with_torch_autograd(name):
    """float64 on the CPU, N = 37: y and every gradient at 1e-12 of each tensor's scale"""
    widths = NETS[name]
    Ws, bs = make_net(widths, seed=1, dtype=np.float64)
    x, g_y = make_rows(37, widths[0], 2, np.float64), make_rows(37, widths[-1], 3, np.float64)
    y, _ = checker_forward(x, Ws, bs)
    g_x, g_W, g_b = checker_backward(x, Ws, bs, g_y)
    seq = sequential_of(Ws, bs)
    tx = torch.tensor(x, requires_grad=True)
    ty = seq(tx)
    (ty * torch.tensor(g_y)).sum().backward()
    linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
    pairs = [("y", y, ty.detach()), ("g_x", g_x, tx.grad)]
    pairs += [(f"g_W[{l}]", g_W[l], m.weight.grad) for l, m in enumerate(linears)]
    pairs += [(f"g_b[{l}]", g_b[l], m.bias.grad) for l, m in enumerate(linears)]
    worst = 0.0
    for what, got, want in pairs:
        want = want.numpy()
        assert got.shape == want.shape, what
        err = np.abs(got - want).max() / scale_of(want)
        worst = max(worst, err)
        assert err <= 1e-12, f"{what}: {err:.3g} of its scale"
    print(f"checker vs torch autograd, {name}: worst {worst:.3g} of a tensor's scale")


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_mlp_scratch_bytes", "pigs_mlp_forward", "pigs_mlp_backward")


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


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
    assert _lib.SIGNATURES["pigs_mlp_scratch_bytes"][0] is ctypes.c_size_t


def test_scratch_size_is_monotone_up_to_its_cap(hip_lib):
    """one record of sum_l w_{l+1} (w_l + 1) floats per wave, one wave per 16 rows, at most 256 waves"""
    size = hip_lib.pigs_mlp_scratch_bytes
    for widths in NETS.values():
        w = ints(*widths)
        L = len(widths) - 1
        record = 4 * sum(o * (i + 1) for i, o in zip(widths[:-1], widths[1:]))
        last = 0
        for N in (1, 15, 16, 17, 1600, 4095, 4096, 4097, 65536, 1 << 30):
            got = size(N, L, w)
            assert got == min((N + 15) // 16, 256) * record, (widths, N)
            assert got >= last
            last = got
        assert size(4096, L, w) == size(1 << 30, L, w)                   # the cap
        assert size(0, L, w) == 0 and size(-5, L, w) == 0
    assert size(16, 0, ints(4)) == 0 and size(16, 7, ints(*[4] * 8)) == 0
    assert size(16, 1, ints(0, 4)) == 0 and size(16, 1, ints(4, 49)) == 0 and size(16, 2, ints(4, -1, 4)) == 0
    assert size(16, 1, None) == 0


def test_abi_refusals_come_before_any_hip_call(hip_lib):
    """device pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some = None, 1 << 12
    fwd, bwd = hip_lib.pigs_mlp_forward, hip_lib.pigs_mlp_backward

    def forward(dtype=0, N=4, widths=(5, 7, 3), x=some, W=True, b=True, y=some, hole=None):
        L = len(widths) - 1
        Wp, bp = [some] * L, [some] * L
        if hole == "W":
            Wp[-1] = null
        if hole == "b":
            bp[0] = null
        return fwd(dtype, N, L, ints(*widths) if widths else None, x, pointers(*Wp) if W else None,
                   pointers(*bp) if b else None, y, None)
    assert forward(dtype=1) == 2 and forward(dtype=7) == 2                         # float64, no such dtype
    assert forward(widths=(0, 4)) == 2 and forward(widths=(4, 49)) == 2 and forward(widths=(4, 0, 4)) == 2
    assert forward(widths=(49, 4)) == 2 and forward(widths=(4, 4, -1)) == 2
    assert fwd(0, 4, 0, ints(4), some, pointers(some), pointers(some), some, None) == 2              # L = 0
    assert forward(widths=(4,) * 8) == 2                                           # L = 7
    assert forward(widths=(4,) * 7, x=null) == 1                                   # L = 6 passes the size checks
    assert forward(N=0) == 1 and forward(N=-3) == 1
    assert fwd(0, 4, 2, None, some, pointers(some, some), pointers(some, some), some, None) == 1     # no widths
    assert forward(x=null) == 1 and forward(W=False) == 1 and forward(b=False) == 1 and forward(y=null) == 1
    assert forward(hole="W") == 1 and forward(hole="b") == 1                       # a null entry

    def backward(dtype=0, N=4, widths=(5, 7, 3), x=some, g_y=some, scratch=some, nbytes=1 << 20, g_x=some, gW=True,
                 gb=True, hole=None):
        L = len(widths) - 1
        Wp = [some] * L
        if hole == "W":
            Wp[0] = null
        return bwd(dtype, N, L, ints(*widths), x, pointers(*Wp), pointers(*[some] * L), g_y, scratch, nbytes, g_x,
                   pointers(*[some] * L) if gW else None, pointers(*[some] * L) if gb else None, None)
    assert backward(dtype=1) == 2 and backward(widths=(5, 49, 3)) == 2 and backward(widths=(4,) * 8) == 2
    assert backward(N=0) == 1 and backward(x=null) == 1 and backward(g_y=null) == 1 and backward(hole="W") == 1
    assert backward(g_x=null, gW=False, gb=False) == 1                             # no gradient wanted
    need = hip_lib.pigs_mlp_scratch_bytes(4, 2, ints(5, 7, 3))
    assert need == 4 * (7 * 6 + 3 * 8)
    assert backward(nbytes=need - 1) == 1 and backward(nbytes=0) == 1              # a short scratch
    assert backward(scratch=null) == 1 and backward(scratch=some + 2) == 1         # none, or off its alignment
    assert backward(scratch=null, gW=False) == 1                                   # a bias gradient alone needs it too
    assert backward(N=4097, nbytes=256 * need - 1) == 1 and backward(N=1600, nbytes=100 * need - 1) == 1


# ---- the Python surface -------------------------------------------------------------------------------------
def test_fused_mlp_refuses_cpu_tensors_and_bad_arguments(hip_lib):
    import pigs_amd
    f = pigs_amd.fused_mlp
    x, W, b = torch.zeros(4, 5), [torch.zeros(3, 5)], [torch.zeros(3)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, W, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x[None], W, b)
    with pytest.raises(TypeError):
        f(x.numpy(), W, b)
    with pytest.raises(TypeError):
        f(x, W, [None])
    with pytest.raises(TypeError):
        f(x.double(), [W[0].double()], [b[0].double()])                       # float64 is not built
    with pytest.raises(TypeError):
        f(x, W, [b[0].double()])
    with pytest.raises(NotImplementedError):
        f(x, [], [])
    with pytest.raises(NotImplementedError):
        f(torch.zeros(4, 4), [torch.zeros(4, 4)] * 7, [torch.zeros(4)] * 7)    # seven layers
    with pytest.raises(NotImplementedError):
        f(torch.zeros(4, 49), [torch.zeros(3, 49)], b)
    with pytest.raises(NotImplementedError):
        f(x, [torch.zeros(49, 5)], [torch.zeros(49)])
    with pytest.raises(ValueError):
        f(torch.zeros(0, 5), W, b)                                            # N = 0
    with pytest.raises(ValueError):
        f(torch.zeros(2, 4, 5), W, b)                                         # a leading 2
    with pytest.raises(ValueError):
        f(x, [torch.zeros(3, 6)], b)                                          # the widths do not chain
    with pytest.raises(ValueError):
        f(x, W, [torch.zeros(4)])
    with pytest.raises(ValueError):
        f(x, W, b + b)
    with pytest.raises(ValueError, match="contiguous"):
        f(torch.zeros(4, 10)[:, ::2], W, b)
    with pytest.raises(ValueError, match="contiguous"):
        f(x, [torch.zeros(5, 3).t()], b)


def test_from_sequential_shares_parameters_and_keeps_the_state_dict(hip_lib):
    import pigs_amd
    nn = torch.nn
    seq = nn.Sequential(nn.Linear(48, 32), nn.Tanh(), nn.Linear(32, 16), nn.Tanh(), nn.Linear(16, 6))
    keys, params = list(seq.state_dict()), list(seq.parameters())
    net = pigs_amd.FusedMLP.from_sequential(seq)
    assert isinstance(net, nn.Module)
    assert len(list(net.parameters())) == len(params) and all(a is b for a, b in zip(net.parameters(), params))
    assert list(net.state_dict()) == keys

    class Holder(nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.delta_net = inner
    before = {k: v.clone() for k, v in Holder(seq).state_dict().items()}
    after = Holder(net)
    assert list(after.state_dict()) == list(before)                 # "delta_net.0.weight", ...: checkpoints stay valid
    after.load_state_dict({k: v + 1 for k, v in before.items()})
    assert torch.equal(seq[0].weight, before["delta_net.0.weight"] + 1)      # the same storage was loaded into
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(4, 48))


UNSUPPORTED = {                     # the words the refusal must hold: the net that makes it
    "ReLU": lambda nn: nn.Sequential(nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 4)),
    "Sigmoid": lambda nn: nn.Sequential(nn.Linear(4, 4), nn.Sigmoid(), nn.Linear(4, 4)),
    "Conv1d": lambda nn: nn.Sequential(nn.Conv1d(4, 4, 1), nn.Tanh(), nn.Linear(4, 4)),
    "bias=False": lambda nn: nn.Sequential(nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 4, bias=False)),
    "width 49": lambda nn: nn.Sequential(nn.Linear(4, 49), nn.Tanh(), nn.Linear(49, 4)),
    "width 64": lambda nn: nn.Sequential(nn.Linear(64, 4)),
    "7 nn.Linear": lambda nn: nn.Sequential(*([nn.Linear(4, 4), nn.Tanh()] * 6 + [nn.Linear(4, 4)])),
    "ends with Tanh": lambda nn: nn.Sequential(nn.Linear(4, 4), nn.Tanh()),
    "is Linear": lambda nn: nn.Sequential(nn.Linear(4, 4), nn.Linear(4, 4)),
}


@pytest.mark.parametrize("what", list(UNSUPPORTED), ids=[k.replace(" ", "_").replace("=", "_") for k in UNSUPPORTED])
def test_from_sequential_refuses_by_name(hip_lib, what):
    import pigs_amd
    with pytest.raises(NotImplementedError, match=re.escape(what)):
        pigs_amd.FusedMLP.from_sequential(UNSUPPORTED[what](torch.nn))


def test_from_sequential_takes_a_sequential_only(hip_lib):
    import pigs_amd
    with pytest.raises(TypeError, match="Linear"):
        pigs_amd.FusedMLP.from_sequential(torch.nn.Linear(4, 4))
