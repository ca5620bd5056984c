"""CPU: NetworkAdam (pigs_amd/network_adam.py, csrc/network_adam.hip) -- its float64 checker against torch.optim.Adam, the
packing between the flat moments and torch's state dict, the C ABI's refusals and the Python refusals.  No GPU call is
made here.

The checker, shared with tests/test_network_adam_gpu.py:
    make_state()     a starting state over a list of shapes: parameters, moments, per-tensor step counts (float64 numpy)
    make_grads()     one gradient per tensor, None where the tensor sits the step out
    checker_step()   ONE step from a given state, per tensor, with the presence mask and per-tensor step counts
As in tests/test_optim.py every comparison is one step from a given state.
"""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_optim import BETAS, EPS, scale_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3


# ---- the checker --------------------------------------------------------------------------------------------
def make_state(shapes, seed, steps=0, moments=False):
    """parameters N(0, 1); moments zero or random (exp_avg N(0, 1), exp_avg_sq chi^2); ``steps``: an int or a list"""
    rng = np.random.default_rng(seed)
    p = [rng.standard_normal(s) for s in shapes]
    if moments:
        m = [rng.standard_normal(s) for s in shapes]
        v = [rng.standard_normal(s) ** 2 for s in shapes]
    else:
        m, v = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    steps = list(steps) if isinstance(steps, (list, tuple)) else [int(steps)] * len(shapes)
    return {"p": p, "m": m, "v": v, "steps": steps}


def make_grads(shapes, seed, absent=()):
    rng = np.random.default_rng(seed + 7919)
    grads = [rng.standard_normal(s) for s in shapes]
    return [None if k in absent else g for k, g in enumerate(grads)]


def as_dtype(state, dtype):
    """the state rounded to ``dtype`` and promoted back to float64: what a float32 run starts from"""
    out = copy.deepcopy(state)
    for k in ("p", "m", "v"):
        out[k] = [a.astype(dtype).astype(np.float64) for a in state[k]]
    return out


def checker_step(state, grads, lr=LR, betas=BETAS, eps=EPS):
    """ONE step of Adam as torch.optim.Adam defines it; a tensor whose gradient is None keeps everything"""
    new = copy.deepcopy(state)
    b1, b2 = betas
    for s, g in enumerate(grads):
        if g is None:
            continue
        t = new["steps"][s] = state["steps"][s] + 1
        m = new["m"][s] = b1 * state["m"][s] + (1.0 - b1) * g
        v = new["v"][s] = b2 * state["v"][s] + (1.0 - b2) * g ** 2
        new["p"][s] = state["p"][s] - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return new


def torch_adam(state, dtype=torch.float64, device="cpu", lr=LR, **kw):
    """leaves and a torch.optim.Adam(foreach=False) over them carrying the state's moments and counts"""
    params = [torch.tensor(a, dtype=dtype, device=device, requires_grad=True) for a in state["p"]]
    optim = torch.optim.Adam(params, lr=lr, betas=BETAS, eps=EPS, foreach=False, **kw)
    for s, p in enumerate(params):
        if state["steps"][s] > 0:
            optim.state[p] = {"step": torch.tensor(float(state["steps"][s])),
                              "exp_avg": torch.tensor(state["m"][s], dtype=dtype, device=device),
                              "exp_avg_sq": torch.tensor(state["v"][s], dtype=dtype, device=device)}
    return params, optim


def torch_step(params, optim, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else torch.as_tensor(g, dtype=p.dtype, device=p.device).clone()
    optim.step()


def read_torch(params, optim, like):
    out = copy.deepcopy(like)
    for s, p in enumerate(params):
        out["p"][s] = p.detach().cpu().double().numpy().copy()
        st = optim.state.get(p)
        if st:
            out["m"][s] = st["exp_avg"].cpu().double().numpy().copy()
            out["v"][s] = st["exp_avg_sq"].cpu().double().numpy().copy()
            out["steps"][s] = int(st["step"])
        else:
            out["steps"][s] = 0
    return out


SHAPES = [(1,), (3,), (4, 1), (5,), (31, 33), (1024,), (1025,), (16, 16), (7, 32)]


def test_checker_agrees_with_torch_adam():
    """float64 on the CPU, three steps, each compared as ONE step from torch's state before it; tensor 4 has no gradient
    at step 2, so the step counts differ at step 3.  The project's float64 bar, 1e-12 of each tensor's scale"""
    state = make_state(SHAPES, seed=1)
    params, optim = torch_adam(state)
    worst = 0.0
    for it in range(3):
        grads = make_grads(SHAPES, seed=10 + it, absent=(4,) if it == 1 else ())
        before = read_torch(params, optim, state)
        torch_step(params, optim, grads)
        want = read_torch(params, optim, state)
        got = checker_step(before, grads)
        assert got["steps"] == want["steps"]
        for k in ("p", "m", "v"):
            for s in range(len(SHAPES)):
                err = float(np.abs(got[k][s] - want[k][s]).max()) / scale_of(want[k][s])
                worst = max(worst, err)
                assert err <= 1e-12, f"step {it} {k}[{s}]: {err:.3g} of its scale"
        if it == 1:
            assert np.array_equal(got["p"][4], before["p"][4]) and got["steps"][4] == before["steps"][4] == 1
    assert want["steps"] == [3, 3, 3, 3, 2, 3, 3, 3, 3]
    print(f"checker vs torch.optim.Adam, float64: worst {worst:.3g} of a tensor's scale")


# ---- the packing --------------------------------------------------------------------------------------------
def test_segments_start_at_multiples_of_four():
    from pigs_amd.network_adam import segment_offsets
    offsets, total = segment_offsets([1, 3, 4, 5, 1023, 1024, 1025])
    assert offsets == [0, 4, 8, 12, 20, 1044, 2068] and total == 3096
    assert segment_offsets([4]) == ([0], 4) and segment_offsets([]) == ([], 0)


def test_running_products_are_repeated_multiplications():
    from pigs_amd.network_adam import running_products
    steps = [0, 3, 1, 1000, 3]
    for beta in BETAS:
        want = []
        for t in steps:
            p = 1.0
            for _ in range(t):
                p *= beta
            want.append(p)
        assert running_products(beta, steps) == want


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_state_dict_packing_round_trip(dtype):
    """a real torch.optim.Adam on CPU tensors: parameter 2 is frozen (no slot), parameter 4 never has a gradient (no
    state), parameter 1 misses a step.  torch's state dict -> the flat arrays -> the per-tensor layout -> a fresh
    torch.optim.Adam: the same keys, the same steps, the same moments bit for bit, and the same third step"""
    from pigs_amd.network_adam import pack_moments, segment_offsets, unpack_moments
    shapes = [(3,), (5, 7), (2, 2), (1,), (6,), (1025,)]
    state = make_state(shapes, seed=3)
    params = [torch.tensor(a, dtype=dtype, requires_grad=k != 2) for k, a in enumerate(state["p"])]
    adam = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    for it in range(2):
        torch_step(params, adam, make_grads(shapes, seed=20 + it, absent=(2, 4) + ((1,) if it == 0 else ())))
    sd = adam.state_dict()
    assert sorted(sd["state"]) == [0, 1, 3, 5]
    positions = [k for k in range(len(shapes)) if k != 2]
    slot_shapes = [shapes[k] for k in positions]
    _, total = segment_offsets([int(np.prod(s)) for s in slot_shapes])
    flat_m, flat_v = torch.full((total,), 9.0, dtype=dtype), torch.full((total,), 9.0, dtype=dtype)
    steps = pack_moments(sd["state"], positions, slot_shapes, flat_m, flat_v)          # torch's loads into ours
    assert steps == [2, 1, 2, 0, 2]
    ours = {"state": unpack_moments(flat_m, flat_v, steps, positions, slot_shapes), "param_groups": sd["param_groups"]}
    assert sorted(ours["state"]) == sorted(sd["state"])
    for k, entry in sd["state"].items():
        mine = ours["state"][k]
        assert sorted(mine) == sorted(entry) == ["exp_avg", "exp_avg_sq", "step"]
        assert mine["step"].dtype == entry["step"].dtype == torch.float32 and mine["step"].dim() == 0
        assert float(mine["step"]) == float(entry["step"])
        for key in ("exp_avg", "exp_avg_sq"):
            assert mine[key].shape == entry[key].shape and torch.equal(mine[key], entry[key]), (k, key)
            assert mine[key].untyped_storage().data_ptr() == (flat_m if key == "exp_avg" else flat_v).untyped_storage().data_ptr()
    at = segment_offsets([int(np.prod(s)) for s in slot_shapes])[0][3]
    assert not flat_m[at:at + 6].any() and not flat_v[at:at + 6].any()               # no entry: zeros
    fresh = [p.detach().clone().requires_grad_(p.requires_grad) for p in params]
    other = torch.optim.Adam(fresh, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    other.load_state_dict(ours)                                                      # ours loads into torch's
    grads = make_grads(shapes, seed=22, absent=(2,))
    torch_step(params, adam, grads)
    torch_step(fresh, other, grads)
    for a, b in zip(params, fresh):
        assert torch.equal(a, b)
    assert [int(other.state[p]["step"]) for k, p in enumerate(fresh) if k != 2] == [3, 2, 3, 1, 3]
    with pytest.raises(ValueError):
        pack_moments({0: {"step": torch.tensor(1.0), "exp_avg": torch.zeros(4), "exp_avg_sq": torch.zeros(4)}}, positions,
                     slot_shapes, flat_m, flat_v)


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_network_adam_state_doubles", "pigs_network_adam_step")


def test_symbols_declared_exported_and_bound(hip_lib):
    import pigs_amd
    from pigs_amd import _lib, network_adam
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION
    assert pigs_amd.NetworkAdam is network_adam.NetworkAdam
    assert issubclass(pigs_amd.NetworkAdam, torch.optim.Optimizer)
    # struct PigsNetworkAdam: the binding's layout is the header's (an int, 128 counts, 2 x 128 pointers, 5 doubles, a pointer)
    assert ctypes.sizeof(_lib.PigsNetworkAdam) == 8 + 3 * 128 * 8 + 5 * 8 + 8
    assert _lib.PigsNetworkAdam.dev_lr.offset == 8 + 3 * 128 * 8 + 5 * 8
    assert [hip_lib.pigs_network_adam_state_doubles(s) for s in (0, 1, 90, 128, 129)] == [0, 9, 454, 644, 0]


def block_of(counts, grads=True):
    from pigs_amd import _lib
    b = _lib.PigsNetworkAdam()
    b.tensors = len(counts)
    for s, n in enumerate(counts[:128]):
        b.counts[s], b.params[s], b.grads[s] = n, 1 << 12, (1 << 16) if grads else None
    b.lr, b.beta1, b.beta2, b.eps = LR, BETAS[0], BETAS[1], EPS
    return b


def test_refusals_come_before_any_hip_call(hip_lib):
    """pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    null, some, odd = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)
    step = hip_lib.pigs_network_adam_step
    ok = block_of([5, 7])
    tail = (some, some, some, null, 0, null)
    assert step(7, ctypes.byref(ok), *tail) == 2                                         # dtype
    assert step(0, ctypes.byref(ok), some, some, some, some, 5, null) == 2               # the loss's dtype
    assert step(0, None, *tail) == 1                                                     # no block
    for S in (0, -1, 129):
        b = block_of([5, 7])
        b.tensors = S
        assert step(0, ctypes.byref(b), *tail) == 1, S                                   # S < 1, S > 128
    b = block_of([5, 7])
    b.params[1] = None
    assert step(0, ctypes.byref(b), *tail) == 1                                          # a NULL parameter
    for n in (0, -3):
        assert step(0, ctypes.byref(block_of([5, n])), *tail) == 1                       # a count that is not positive
    assert step(0, ctypes.byref(block_of([1 << 30, 1 << 30])), *tail) == 1               # 2^31 elements
    assert step(1, ctypes.byref(block_of([(1 << 31) - 5, 1, 1])), *tail) == 1            # the same through the padding
    assert step(0, ctypes.byref(block_of([5, 7], grads=False)), *tail) == 1              # no gradient anywhere
    b = block_of([5, 7])
    b.grads[0] = (1 << 16) + 4
    assert step(1, ctypes.byref(b), *tail) == 1                                          # a double off its alignment
    assert step(0, ctypes.byref(ok), null, some, some, null, 0, null) == 1               # no state
    assert step(0, ctypes.byref(ok), ctypes.c_void_p((1 << 20) + 4), some, some, null, 0, null) == 1     # a state off 8 bytes
    for k in (1, 2):                                                                     # the moments: NULL, off 16 bytes
        for bad in (null, odd):
            args = [some, some, some, null, 0, null]
            args[k] = bad
            assert step(0, ctypes.byref(ok), *args) == 1, (k, bad)
    b = block_of([5, 7])
    b.dev_lr = (1 << 16) + 4
    assert step(0, ctypes.byref(b), *tail) == 1                                          # the device rate off 8 bytes
    assert step(0, ctypes.byref(ok), some, some, some, ctypes.c_void_p((1 << 20) + 4), 1, null) == 1     # a double loss off 8


# ---- the Python surface -------------------------------------------------------------------------------------
def leaves(*shapes, dtype=torch.float32):
    return [torch.zeros(s, dtype=dtype, requires_grad=True) for s in shapes]


def test_network_adam_refuses_cpu_tensors_and_bad_arguments(hip_lib):
    from pigs_amd import NetworkAdam
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NetworkAdam(leaves((4, 2), (3,)))
    with pytest.raises(ValueError, match="ONE parameter group"):
        NetworkAdam([{"params": leaves((4,))}, {"params": leaves((3,)), "lr": 1e-2}])
    with pytest.raises(ValueError, match="at most 128"):
        NetworkAdam(leaves(*[(2,)] * 129))
    with pytest.raises(TypeError, match="all alike"):
        NetworkAdam(leaves((4,)) + leaves((3,), dtype=torch.float64))
    with pytest.raises(TypeError):
        NetworkAdam(leaves((4,), dtype=torch.float16))
    with pytest.raises(ValueError, match="contiguous"):
        NetworkAdam(leaves((4,)) + [torch.zeros(4, 6).t().requires_grad_(True)])
    with pytest.raises(ValueError):
        NetworkAdam([torch.zeros(3)])                                            # nothing requires grad
    with pytest.raises(ValueError):
        NetworkAdam(leaves((4,)), lr=-1.0)                                       # torch's own checks of lr, betas, eps
    with pytest.raises(ValueError):
        NetworkAdam(leaves((4,)), betas=(0.9, 1.0))
    for kw in ({"weight_decay": 0.1}, {"amsgrad": True}, {"maximize": True}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            NetworkAdam(leaves((4,)), **kw)
    # 128 tensors that require grad beside frozen ones are not refused for their number: the device comes last
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NetworkAdam(leaves(*[(2,)] * 128) + [torch.zeros(6)])
