"""CPU: the optimiser's gradient statistics (GaussianAdam(grad_stats=True), pigs_optim_step_stats) -- a float64 checker
against torch.optim.Adam plus autograd plus the reference's literal statistic lines (test_no_mlp.py:149-155), the planted
mistakes the checker must see, the presence patterns, ``shift_means`` against test_no_mlp_1d.py:204-256, the C ABI's new
symbols and refusals, and the recorded loops of tests/golden/grad_stats/*.npz.  No GPU call is made here.

Shared with tests/test_optim_stats_gpu.py and the 1-D modules:
    make_stats()     a starting statistics state: random NON-zero sums, counts 3
    stats_step()     ONE step of the statistics from a given state, for any chain rule (d = 2: test_optim.chain_rule)
    TorchChain       the reference's step behind GaussianAdam's interface: tanh / exp / covariances_from_raw, autograd,
                     torch.optim.Adam, and the four statistic lines after every backward
    loop_2d()        tests/test_training_gpu.py::run_loop restated over that interface (tools/gen_grad_stats.py records it
                     with the reference's sampling functions; the GPU tests drive it with GaussianAdam)
"""
import collections
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_optim import (BETAS, EPS, GROUPS, RATES, chain_rule, checker_step, make_grads, make_state, read_torch, scale_of,
                        torch_state, torch_step)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = ("mean_grad", "mean_grad_norm", "scale_grad", "scale_grad_norm")
STATS = SUMS + ("last_mean_grad", "last_scale_grad")
STAT_GROUPS = {"means": ("mean_grad", "mean_grad_norm", "last_mean_grad"),
               "scaling": ("scale_grad", "scale_grad_norm", "last_scale_grad")}


# ---- the checker --------------------------------------------------------------------------------------------
def make_stats(N, seed, d=2, counts=3):
    """random NON-zero sums N(0, 1), norms at least those of the sums (they are sums of norms), last gradients N(0, 1)"""
    rng = np.random.default_rng(seed + 7919)
    out = {"mean_grad": rng.standard_normal((N, d)), "scale_grad": rng.standard_normal((N, d)),
           "last_mean_grad": rng.standard_normal((N, d)), "last_scale_grad": rng.standard_normal((N, d))}
    out["mean_grad_norm"] = np.linalg.norm(out["mean_grad"], axis=-1) + rng.uniform(0.0, 2.0, N)
    out["scale_grad_norm"] = np.linalg.norm(out["scale_grad"], axis=-1) + rng.uniform(0.0, 2.0, N)
    out["counts"] = {"means": counts, "scaling": counts}
    return out


def stats_as_dtype(stats, dtype):
    return {k: (dict(v) if k == "counts" else v.astype(dtype).astype(np.float64)) for k, v in stats.items()}


def stats_step(p, stats, grads, means_map="tanh", scale=1.0, chain=chain_rule, mistake=None):
    """ONE step of the statistics from ``stats``, with G the raw parameters' gradients of ``chain``:
    last = G, sum += G, norm += ||sum|| (the sum AFTER adding).  ``mistake`` plants one of three wrong readings."""
    raw = chain(p, grads, means_map, scale)
    new = copy.deepcopy(stats)
    for g, (s, n, last) in STAT_GROUPS.items():
        G = raw[g]
        if G is None:
            continue
        if mistake == "d_mu" and g == "means":
            G = grads[0]                                          # the leaf's gradient, not the raw parameter's
        new[last] = G.copy()
        new[s] = stats[s] + G
        normed = {None: new[s], "d_mu": new[s], "step_norm": G, "norm_before": stats[s]}[mistake]
        new[n] = stats[n] + np.sqrt((normed ** 2).sum(-1))
        new["counts"][g] = stats["counts"][g] + 1
    return new


def torch_stats(stats, dtype=torch.float64, device="cpu"):
    return {k: torch.tensor(stats[k], dtype=dtype, device=device) for k in STATS}


def reference_lines(t, raw_means, scaling):
    """test_no_mlp.py:149-155 / test_no_mlp_1d.py:156-162, on the gradients a backward left; a parameter without one is
    skipped, as its group is; the last step's gradients as test_initialize.py:156-158 reads them"""
    if raw_means.grad is not None:
        t["mean_grad"] += raw_means.grad
        t["mean_grad_norm"] += torch.norm(t["mean_grad"], dim=-1)
        t["last_mean_grad"] = raw_means.grad.detach().clone()
    if scaling.grad is not None:
        t["scale_grad"] += scaling.grad
        t["scale_grad_norm"] += torch.norm(t["scale_grad"], dim=-1)
        t["last_scale_grad"] = scaling.grad.detach().clone()


def assert_stats_agree(got, want, bar, what=""):
    worst = 0.0
    for k in STATS:
        w = want[k].detach().cpu().double().numpy() if isinstance(want[k], torch.Tensor) else want[k]
        err = float(np.abs(got[k] - w).max()) / scale_of(w)
        worst = max(worst, err)
        assert err <= bar, f"{what} {k}: {err:.3g} of its scale > {bar:.3g}"
    return worst


def test_checker_agrees_with_torch_and_the_reference_lines():
    """float64 on the CPU, five consecutive steps, each compared as ONE step from torch's state before it; starting from
    non-zero sums; the covariances' gradient comes and goes; 1e-12 of each tensor's scale"""
    N, c = 257, 2
    state = make_state(N, c, seed=1, t_max=3.0)
    stats = make_stats(N, seed=1)
    params, optim = torch_state(state)
    t = torch_stats(stats)
    worst = 0.0
    for it in range(5):
        grads = make_grads(N, c, seed=10 + it, present=(True, True, it % 2 == 1, True))
        before = read_torch(params, optim, state)
        stats_before = dict({k: t[k].numpy().copy() for k in STATS}, counts=dict(stats["counts"]))
        torch_step(params, optim, grads, "tanh", 2.5)             # leaves the gradients on the parameters
        reference_lines(t, params["means"], params["scaling"])
        got = stats_step(before["p"], stats_before, grads, "tanh", 2.5)
        worst = max(worst, assert_stats_agree(got, t, 1e-12, f"step {it}"))
        assert got["counts"] == {"means": 3 + 1, "scaling": 3 + 1}
    print(f"statistics checker vs torch + the reference's lines, float64: worst {worst:.3g} of a tensor's scale")


@pytest.mark.parametrize("mistake", ["step_norm", "norm_before", "d_mu"])
def test_checker_sees_a_planted_mistake(mistake):
    """from NON-zero sums each wrong reading moves a statistic by far more than any bar of the GPU tests allows (the
    loosest is 2e-3 of an array's scale, float64's 1e-11): at least 1e-2 of the array's scale is asked"""
    N, c = 257, 2
    state, stats = make_state(N, c, seed=2), make_stats(N, seed=2)
    grads = make_grads(N, c, seed=3, present=(True, True, True, True))
    want = stats_step(state["p"], stats, grads, "tanh", 2.5)
    wrong = stats_step(state["p"], stats, grads, "tanh", 2.5, mistake=mistake)
    moved = max(float(np.abs(wrong[k] - want[k]).max()) / scale_of(want[k]) for k in STATS)
    print(f"planted mistake {mistake}: moves a statistic by {moved:.3g} of its scale, {moved / 1e-11:.3g} x the float64 "
          f"bar, {moved / 2e-3:.3g} x the loop bar")
    assert moved >= 1e-2


PATTERNS = [(a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)
            if a or b or c or d]


@pytest.mark.parametrize("present", PATTERNS, ids=["".join("mvcq"[i] if on else "-" for i, on in enumerate(p)) for p in PATTERNS])
def test_absent_groups_keep_their_statistics(present):
    N, c = 65, 2
    state, stats = make_state(N, c, seed=4, moments=True, steps=3), make_stats(N, seed=4)
    grads = make_grads(N, c, seed=5, present=present)
    params, optim = torch_state(state)
    t = torch_stats(stats)
    torch_step(params, optim, grads, "identity")
    reference_lines(t, params["means"], params["scaling"])
    got = stats_step(state["p"], stats, grads, "identity")
    assert_stats_agree(got, t, 1e-12, str(present))
    on = {"means": present[0], "scaling": present[2] or present[3]}
    for g, names in STAT_GROUPS.items():
        assert got["counts"][g] == 3 + int(on[g])
        if not on[g]:
            assert all(np.array_equal(got[k], stats[k]) for k in names), g
        else:
            assert not np.array_equal(got[names[0]], stats[names[0]])


# ---- refine with shift_means --------------------------------------------------------------------------------
def clone_maps(keep, split):
    """``refine_index(keep, split, mode="clone")``: the kept rows, then the split ones again (child 0)"""
    kept, again = np.nonzero(keep)[0], np.nonzero(split & keep)[0]
    return (torch.as_tensor(np.concatenate((kept, again))),
            torch.as_tensor(np.concatenate((np.full(len(kept), -1), np.zeros(len(again), dtype=np.int64)))))


@pytest.mark.parametrize("d", [1, 2])
def test_shift_means_is_the_reference_densification(d):
    """pigs_amd.optim.follow_maps with a shift (what ``opt.refine(source, child, shift_means)`` applies to the means)
    against test_no_mlp_1d.py:219-251 line for line on a real torch.optim.Adam state: bitwise"""
    from pigs_amd.optim import follow_maps
    N, c = 40, 1
    rng = np.random.default_rng(11 + d)
    raw_means = torch.nn.Parameter(torch.tensor(rng.standard_normal((N, d))))
    values = torch.nn.Parameter(torch.tensor(rng.standard_normal((N, c))))
    scaling = torch.nn.Parameter(torch.tensor(rng.uniform(-4.0, -1.0, (N, d))))
    parameters = [{"name": "means", "params": raw_means, "lr": 1e-2}, {"name": "values", "params": values, "lr": 1e-2},
                  {"name": "scaling", "params": scaling, "lr": 1e-2}]
    optim = torch.optim.Adam(parameters)
    for _ in range(3):
        ((torch.tanh(raw_means) ** 2).sum() + (values ** 3).sum() + torch.exp(scaling).sum()).backward()
        optim.step()
        optim.zero_grad()
    mean_grad = torch.tensor(rng.standard_normal((N, d)))
    keep_mask = torch.tensor(rng.random(N) > 0.2)
    split_indices = torch.logical_and(torch.tensor(rng.random(N) > 0.6), keep_mask)
    old = {"means": raw_means.detach().clone(), "values": values.detach().clone(), "scaling": scaling.detach().clone()}
    old_m = {g["name"]: optim.state[g["params"][0]]["exp_avg"].clone() for g in optim.param_groups}
    old_v = {g["name"]: optim.state[g["params"][0]]["exp_avg_sq"].clone() for g in optim.param_groups}
    with torch.no_grad():                                         # test_no_mlp_1d.py:219-251
        split_dir = mean_grad[split_indices]
        extensions = {"means": raw_means.data[split_indices] + split_dir, "values": values.data[split_indices],
                      "scaling": scaling.data[split_indices]}
        new_tensors = {}
        for group in optim.param_groups:
            extension = extensions[group["name"]]
            stored_state = optim.state.get(group["params"][0], None)
            stored_state["exp_avg"] = torch.cat((stored_state["exp_avg"][keep_mask], torch.zeros_like(extension)), dim=0)
            stored_state["exp_avg_sq"] = torch.cat((stored_state["exp_avg_sq"][keep_mask], torch.zeros_like(extension)), dim=0)
            del optim.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0][keep_mask], extension), dim=0).requires_grad_(True))
            optim.state[group["params"][0]] = stored_state
            new_tensors[group["name"]] = group["params"][0]
    source, child = clone_maps(keep_mask.numpy(), split_indices.numpy())
    assert int(split_indices.sum()) > 0 and int((~keep_mask).sum()) > 0
    for name in ("means", "values", "scaling"):
        p, m, v = follow_maps(old[name], old_m[name], old_v[name], source, child,
                              shift=mean_grad if name == "means" else None)
        want = new_tensors[name]
        assert torch.equal(p, want.detach()), name
        assert torch.equal(m, optim.state[want]["exp_avg"]) and torch.equal(v, optim.state[want]["exp_avg_sq"]), name
    plain, _, _ = follow_maps(old["means"], old_m["means"], old_v["means"], source, child)
    assert torch.equal(plain, old["means"].index_select(0, source))          # the default: today's behaviour


# ---- the C ABI ----------------------------------------------------------------------------------------------
NAMES = ("pigs_optim_step_stats", "pigs_optim1d_materialize", "pigs_optim1d_step")


def test_symbols_declared_exported_and_bound(hip_lib):
    import pigs_amd
    from pigs_amd import _lib, optim
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("pigs_optim_materialize", "pigs_optim_step"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert hip_lib.pigs_abi_version() == 10 == _lib.ABI_VERSION
    assert pigs_amd.GaussianAdam is optim.GaussianAdam and pigs_amd.GaussianAdam1D is optim.GaussianAdam1D
    # struct PigsGradStats: six array pointers and the device counts; PigsAdamStep as it was
    assert ctypes.sizeof(_lib.PigsGradStats) == 7 * 8 and _lib.PigsGradStats.device_counts.offset == 6 * 8
    assert [f[0] for f in _lib.PigsGradStats._fields_][:6] == list(optim.GradStats._fields)
    fields = re.search(r"typedef struct PigsGradStats \{(.*?)\} PigsGradStats;", header, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", fields) == [f[0] for f in _lib.PigsGradStats._fields_]
    assert ctypes.sizeof(_lib.PigsAdamStep) == 18 * 8 + 2 * 4 + 2 * 8
    assert _lib.PigsAdamStep.device_state.offset == 18 * 8 + 8 + 8


def filled_stats(value=1 << 12):
    from pigs_amd import _lib
    s = _lib.PigsGradStats()
    for name, _ in _lib.PigsGradStats._fields_[:6]:
        setattr(s, name, value)
    return s


def test_stats_step_refusals_come_before_any_hip_call(hip_lib):
    """pointers that are never dereferenced: a call that got as far as a launch would fault; none does"""
    from pigs_amd import _lib
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(1 << 12)
    odd = ctypes.c_void_p((1 << 12) + 4)
    step = hip_lib.pigs_optim_step_stats
    h = _lib.PigsAdamStep()
    h.means_map = 0
    s = filled_stats()
    ok = [some] * 19
    assert step(0, 1, 4, ctypes.byref(h), *ok, None, null) == 1                  # no statistics
    assert step(0, 1, 4, None, *ok, ctypes.byref(s), null) == 1                  # null hyper
    assert step(7, 1, 4, ctypes.byref(h), *ok, ctypes.byref(s), null) == 2       # dtype
    assert step(0, 0, 4, ctypes.byref(h), *ok, ctypes.byref(s), null) == 2       # c outside 1..4
    assert step(0, 5, 4, ctypes.byref(h), *ok, ctypes.byref(s), null) == 2
    assert step(0, 1, 0, ctypes.byref(h), *ok, ctypes.byref(s), null) == 1       # N <= 0
    h.means_map = 3
    assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(s), null) == 2       # map
    h.means_map = 1
    for k in list(range(12)) + [16, 17, 18]:                                     # parameters, moments, outputs
        args = list(ok)
        args[k] = null
        assert step(0, 1, 4, ctypes.byref(h), *args, ctypes.byref(s), null) == 1, k
    args = list(ok)
    args[12:16] = [null] * 4
    assert step(0, 1, 4, ctypes.byref(h), *args, ctypes.byref(s), null) == 1     # no gradient at all
    for k in (0, 2, 4, 6, 8, 10, 12, 16):                                        # the rows of two: off their alignment
        args = list(ok)
        args[k] = odd
        assert step(0, 1, 4, ctypes.byref(h), *args, ctypes.byref(s), null) == 1, k
    for name, _ in _lib.PigsGradStats._fields_[:6]:                              # a null statistics array
        bad = filled_stats()
        setattr(bad, name, None)
        assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1, name
    for name in ("mean_grad", "scale_grad", "last_mean_grad", "last_scale_grad"):  # [N][2]: off their alignment
        bad = filled_stats()
        setattr(bad, name, (1 << 12) + 4)
        assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1, name
        setattr(bad, name, (1 << 12) + 8)
        assert step(1, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1, name
    bad = filled_stats()
    bad.device_counts = 1 << 12                                                  # device counts without a device state
    assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1
    h.device_state = 1 << 12
    bad.device_counts = (1 << 12) + 4                                            # off 8 bytes
    assert step(0, 1, 4, ctypes.byref(h), *ok, ctypes.byref(bad), null) == 1


def test_grad_stats_off_raises_and_bad_arguments(hip_lib):
    from pigs_amd.optim import GaussianAdam
    rm, u, rs, t = torch.zeros(4, 2), torch.ones(4, 3), torch.zeros(4, 2), torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianAdam(rm, u, rs, t, grad_stats=True)
    opt = GaussianAdam.__new__(GaussianAdam)                      # the attributes' refusal needs no GPU
    opt._stats = None
    for read in (lambda: opt.grad_stats, lambda: opt.grad_counts, opt.reset_grad_stats):
        with pytest.raises(RuntimeError, match="grad_stats=True"):
            read()


# ---- the recorded loops -------------------------------------------------------------------------------------
Gaussians = collections.namedtuple("Gaussians", "means values covariances conics")


class TorchChain:
    """The reference's MLP-free step behind GaussianAdam's interface, any device: ``gaussians()`` is tanh / exp /
    covariances_from_raw with autograd, ``step()`` the four statistic lines (test_no_mlp.py:149-155), the last gradients,
    torch.optim.Adam and zero_grad."""

    def __init__(self, raw_means, values, raw_scaling, transform, lr, scale):
        self.p = [t.detach().clone().requires_grad_(True) for t in (raw_means, values, raw_scaling, transform)]
        self.scale = scale
        self.optim = torch.optim.Adam(self.p, lr=lr)
        rm = self.p[0]
        self.stats = {"mean_grad": torch.zeros_like(rm), "mean_grad_norm": torch.zeros(rm.shape[0], dtype=rm.dtype, device=rm.device),
                      "scale_grad": torch.zeros_like(rm), "scale_grad_norm": torch.zeros(rm.shape[0], dtype=rm.dtype, device=rm.device)}

    def gaussians(self):
        from pigs_amd import synthetic
        raw_means, values, raw_scaling, transform = self.p
        cov, con = synthetic.covariances_from_raw(torch.exp(raw_scaling), transform)
        return Gaussians(torch.tanh(raw_means) * self.scale, values, cov, con)

    def step(self):
        reference_lines(self.stats, self.p[0], self.p[2])
        self.optim.step()
        self.optim.zero_grad()

    def read_stats(self):
        return {k: self.stats[k].detach().cpu().double().numpy() for k in STATS}


def read_grad_stats(opt):
    """the six arrays of a GaussianAdam / GaussianAdam1D as float64 numpy"""
    return {k: t.detach().cpu().double().numpy() for k, t in opt.grad_stats._asdict().items()}


def init_2d(device, dtype, n=16):
    """tests/test_training_gpu.py::run_loop's start; returns the four raw parameters and the generator"""
    g = torch.Generator(device="cpu").manual_seed(7)
    tx = torch.linspace(-1, 1, n) * 0.6
    gx, gy = torch.meshgrid((tx, tx), indexing="ij")
    raw_means = torch.atanh(torch.stack((gx, gy), dim=-1).reshape(n * n, 2)).to(device=device, dtype=dtype)
    raw_scaling = torch.full((n * n, 2), -3.0, device=device, dtype=dtype)
    transform = torch.zeros((n * n, 1), device=device, dtype=dtype)
    values = (0.1 * torch.rand((n * n, 1), generator=g)).to(device=device, dtype=dtype)
    return (raw_means, values, raw_scaling, transform), g


def loop_2d(opt, g, new_sampler, device, dtype, steps=30, scale=2.5, dt=0.1):
    """tests/test_training_gpu.py::run_loop over ``opt.gaussians()`` / ``opt.step()``: 1 024 points per step (drawn in
    float32 as there), 10 steps fitting the initial condition, then the diffusion residual against the state frozen at
    step 10.  Returns the losses."""
    sampler = new_sampler()
    losses, prev = [], None
    for it in range(steps):
        samples = ((torch.rand((1024, 2), generator=g) * 2 - 1) * scale).to(device=device, dtype=dtype)
        gs = opt.gaussians()
        if it == 10:
            prev = tuple(t.detach().clone() for t in gs)
        sampler.preprocess(gs.means, gs.values, gs.covariances, gs.conics, samples)
        u = sampler.sample_gaussians()
        if it < 10:
            desired = torch.exp(-0.5 * (samples ** 2).sum(-1) / (0.1 * scale))
            loss = torch.mean((u[:, 0] - desired) ** 2)
        else:
            uxx = sampler.sample_gaussians_laplacian()
            ux = sampler.sample_gaussians_derivative()
            with torch.no_grad():
                sampler2 = new_sampler()
                sampler2.preprocess(*prev, samples)
                u_prev = sampler2.sample_gaussians()
            ut = (u - u_prev) / dt
            loss = torch.mean((ut[:, 0] - (uxx[:, 0, 0, 0] + uxx[:, 1, 1, 0])) ** 2) + 1e-3 * torch.mean(ux ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


def check_fixture(path, n_rows, d):
    f = np.load(path)
    assert int(f["steps"]) == 30 and f["losses"].shape == (30,) and np.isfinite(f["losses"]).all()
    for k in STATS:
        for tag in ("", "_f64"):
            a = f[k + tag]
            assert a.shape == ((n_rows,) if k.endswith("norm") else (n_rows, d)) and np.isfinite(a).all(), k + tag
    # what the norms are sums of: at least the norm of the sum, and not zero
    for s, n in (("mean_grad", "mean_grad_norm"), ("scale_grad", "scale_grad_norm")):
        assert (f[n] >= np.linalg.norm(f[s], axis=-1) * (1 - 1e-5)).all() and f[n].max() > 0
    return f


def test_the_2d_fixture_is_the_recorded_loss_curve():
    """the restated loop with the statistic lines computes what run_loop computed: its float32 losses against
    ref_loss_curve_no_mlp.npz within 1e-6 relative; float32 against float64 as the generator measured them"""
    f = check_fixture(os.path.join(GOLDEN, "grad_stats", "no_mlp_2d.npz"), 256, 2)
    ref = np.load(os.path.join(GOLDEN, "ref_loss_curve_no_mlp.npz"))["losses"]
    rel = np.abs(f["losses"] - ref) / np.abs(ref)
    print(f"2-D fixture vs ref_loss_curve_no_mlp.npz: worst {rel.max():.3g}")
    assert rel.max() <= 1e-6
    worst = max(float(np.abs(f[k] - f[k + "_f64"]).max()) / scale_of(f[k + "_f64"]) for k in STATS)
    loss = float((np.abs(f["losses"] - f["losses_f64"]) / np.abs(f["losses_f64"])).max())
    print(f"2-D fixture, float32 vs float64: losses {loss:.3g}, statistics {worst:.3g} of an array's scale")
    assert loss < 2e-3 / 70 and worst < 2e-3 / 70                 # precision alone leaves the 2e-3 bar 70 x of room
