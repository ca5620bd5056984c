"""GPU: the two cores behind GaussianSampler -- _pigs_host.SamplerCore and host_ctypes.SamplerCore -- take the same
decisions on a sequence of calls.  A seeded walk of 40 calls is played on a ``host="native"`` and a ``host="ctypes"``
sampler in step; after every call both must show the same plans (present, rebuilt, forward-only, recorded-only), the
same cached orders, the same remembered sample plans and the same number of pooled workspaces, and must have returned
the same tensors.  Captures are not part of the walk (tests/test_host_gpu.py has them)."""
import random

import pytest
import torch

from pigs_amd import synthetic

STEPS = 40
ORDERS = (0, 1, 2, 3, "lap")
GETTERS = ("sample_gaussians", "sample_gaussians_derivative", "sample_gaussians_laplacian",
           "sample_gaussians_third_derivative")
WALKS = ((4, 1), (7, 1), (15, 2))      # (seed, channels): seeds whose walks have all four features()


def walk(seed, c):
    """The calls of one walk: ("preprocess", point set, requires_grad, no_grad), ("get", order), ("sample", orders),
    ("residual", with_target), ("vorticity",), ("backward",).  The first call binds something."""
    rng = random.Random(seed)
    kinds = ["preprocess"] * 5 + ["get"] * 4 + ["sample"] * 5 + ["residual"] * 2 + ["backward"] * 3 + ["vorticity"] * (c == 2)
    steps = []
    while len(steps) < STEPS:
        kind = rng.choice(kinds) if steps else "preprocess"
        if kind == "preprocess":
            steps.append((kind, rng.randrange(2), rng.random() < 0.7, rng.random() < 0.4))
        elif kind == "get":
            steps.append((kind, rng.randrange(4)))
        elif kind == "sample":
            orders = [o for o in ORDERS if rng.random() < 0.5] or [rng.choice(ORDERS)]
            rng.shuffle(orders)
            steps.append((kind, tuple(orders)))
        elif kind == "residual":
            steps.append((kind, rng.random() < 0.5))
        else:
            steps.append((kind,))
    return steps


def features(steps):
    """What a walk must contain to be worth playing: (1) a no_grad preprocess followed by a differentiable call -- the
    forward-only rebuild; (2) an order-3 call -- plan3; (3) a point set bound again -- a sample plan reused; (4) a
    request for "lap" and 3 without 2 on an empty cache -- two launches."""
    found, seen, bound, sampled = set(), set(), None, False
    for s in steps:
        if s[0] == "preprocess":
            found |= {3} if s[1] in seen else set()
            seen.add(s[1])
            bound, sampled = s, False
        elif s[0] in ("get", "sample", "residual", "vorticity"):
            if bound[3] and (bound[2] or (s[0] == "residual" and s[1])):
                found.add(1)
            orders = () if s[0] in ("residual", "vorticity") else (s[1],) if s[0] == "get" else s[1]
            if 3 in orders:
                found.add(2)
            if "lap" in orders and 3 in orders and 2 not in orders and not sampled:
                found.add(4)
            sampled = sampled or bool(orders)
    return found


def test_every_walk_has_the_four_features():
    for seed, c in WALKS:
        steps = walk(seed, c)
        assert len(steps) == STEPS and features(steps) == {1, 2, 3, 4}, (seed, c, features(steps))
        assert c == 1 or ("vorticity",) in steps
    assert sorted(c for _, c in WALKS) == [1, 1, 2]


class Player:
    """One sampler playing a walk; after each call: what it returned (detached) and the record of its core."""

    def __init__(self, host, backend, leaves, point_sets, targets):
        from diff_gaussian_sampling import GaussianSampler
        self.s = GaussianSampler(False, backend=backend, host=host)
        self.leaves, self.point_sets, self.targets = leaves, point_sets, targets
        self.target = None               # the target that goes with the bound points
        self.last = None                 # the last differentiable output
        self.plans = (None, None)

    def play(self, k, step):
        s, kind = self.s, step[0]
        outs = ()
        if kind == "preprocess":
            m, v, con = (t if step[2] else t.detach() for t in self.leaves)
            with torch.no_grad() if step[3] else torch.enable_grad():
                s.preprocess(m, v, None, con, self.point_sets[step[1]])
            self.target = self.targets[step[1]]
        elif kind == "get":
            outs = (getattr(s, GETTERS[step[1]])(),)
        elif kind == "sample":
            outs = s.sample(step[1])
        elif kind == "residual":
            outs = (s.residual(1.5, None, -0.3, self.target if step[1] else None),)
        elif kind == "vorticity":
            outs = (s.vorticity_terms(),)
        elif self.last is not None:
            gen = torch.Generator().manual_seed(k)
            w = torch.rand(self.last.shape, generator=gen).to(self.last.device)
            outs = torch.autograd.grad((self.last * w).sum(), (*self.leaves, *self.targets), retain_graph=True,
                                       allow_unused=True)
        if kind != "backward":
            self.last = next((o for o in reversed(outs) if o.requires_grad), self.last)
        core = s._core
        plans = (core.plan, core.plan3)
        record = [(p is not None, p is not None and p is not old, p is not None and p.forward_only,
                   p is not None and p.recorded_only) for p, old in zip(plans, self.plans)]
        self.plans = plans
        record += [list(core.cached_orders()), [p.built for p in core.sample_plans], core.pool_size]
        return [None if o is None else o.detach() for o in outs], record


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["binned", "auto"])
@pytest.mark.parametrize("seed, c", WALKS)
def test_hosts_take_the_same_decisions(hip_lib, seed, c, backend):
    steps = walk(seed, c)
    assert features(steps) == {1, 2, 3, 4}
    gs = synthetic.lattice_gaussians(16, 16, 0.8, seed=3, c=c)
    leaves = [gs[k].float().cuda().requires_grad_(True) for k in ("means", "values", "conics")]
    point_sets = [synthetic.grid_samples(res).float().cuda() for res in (48, 40)]
    gen = torch.Generator().manual_seed(seed)
    targets = [torch.rand((p.shape[0], c), generator=gen).cuda().requires_grad_(True) for p in point_sets]
    players = [Player(host, backend, leaves, point_sets, targets) for host in ("native", "ctypes")]
    built3 = rebuilt = False
    bound = set()
    for k, step in enumerate(steps):
        (outs_n, rec_n), (outs_c, rec_c) = (p.play(k, step) for p in players)
        bound |= {step[1]} if step[0] == "preprocess" else set()
        assert rec_n == rec_c, (k, step, rec_n, rec_c)
        assert len(outs_n) == len(outs_c)
        for a, b in zip(outs_n, outs_c):
            assert (a is None) == (b is None), (k, step)
            if a is None:
                continue
            assert a.shape == b.shape
            if backend == "auto" and step[0] != "backward":
                assert torch.equal(a, b), (k, step)          # dense forward: same kernel, same launch geometry
            else:
                err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                assert err < 2e-6, (k, step, err)
        built3 = built3 or rec_n[1][1]
        rebuilt = rebuilt or (step[0] != "preprocess" and rec_n[0][1])
        if backend == "binned":                 # a point set bound again reuses its sample plan: none is added
            assert len(rec_n[3]) == len(bound), (k, step, rec_n)
    assert all(p.s._plan is None for p in players) == (backend == "auto")      # at these sizes ``auto`` is dense
    if backend == "binned":                     # the walk did reach the policy's corners
        assert built3 and rebuilt
