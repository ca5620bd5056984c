"""GPU: the five fused outputs -- residual() in its linear, general and coupled form, vorticity_terms() and
vorticity_residual() -- share ONE autograd node and ONE call path per host (pigs_host.cpp FusedBackward / fused_apply,
host_ctypes.py _FusedFunction / _fused_call).  What that could break is state leaking from one operator's node into
another's: the wrong entry point, coefficient block, record (aux) or target edge.

All five are created after one preprocess and differentiated in reverse order of creation with all five nodes alive;
each must give the gradients that the same operator gives on a fresh sampler where it is the only call.  The two runs
launch the same kernels on the same data; the backward combines with float atomics, so the bar is the one between any
two float32 runs of a backward (tests/test_vorticity_residual_gpu.py): 1e-5 of the tensor's largest entry.  The
target's gradient is -gout, formed without atomics: exact.

Sizes: dense 40 Gaussians x 700 points, binned 32 Gaussians x 3 000 points (points, weights, tau and the previous
level from small() of tests/test_vorticity_residual_gpu.py, the Gaussians from the lattice generator under it)."""
import pytest
import torch

from pigs_amd import synthetic
from test_residual_coupled_gpu import QA, QB
from test_vorticity_gpu import HOSTS, rel
from test_vorticity_residual_gpu import DT, NU, small

pytestmark = pytest.mark.gpu

NODES = {      # creation order; (ctypes host, native host)
    "linear": ("_ResidualFunctionBackward", "PigsResidualBackward"),
    "general": ("_ResidualTermsFunctionBackward", "PigsResidualTermsBackward"),
    "coupled": ("_ResidualCoupledFunctionBackward", "PigsResidualCoupledBackward"),
    "vorticity_terms": ("_VorticityFunctionBackward", "PigsVorticityBackward"),
    "vorticity_residual": ("_VorticityResidualFunctionBackward", "PigsVorticityResidualBackward"),
}
SHAPES = {"dense": (5, 8, 700), "binned": (4, 8, 3000)}


def problem(backend):
    nx, ny, M = SHAPES[backend]
    gs = synthetic.lattice_gaussians(nx, ny, 1.0, seed=4, c=2)
    base = [gs[k].float().cuda() for k in ("means", "values", "conics")]
    _, pts, _, tau, prev = small(M=M, grad=False)
    gen = torch.Generator().manual_seed(11)
    target = torch.rand((M, 2), generator=gen).cuda()
    weights = {k: (torch.rand((M, 7 if k == "vorticity_terms" else 2), generator=gen) * 2 - 1).cuda() for k in NODES}
    return base, pts, tau, prev, target, weights


def bound_sampler(host, backend, base, pts):
    from diff_gaussian_sampling import GaussianSampler
    t = [x.clone().requires_grad_(True) for x in base]
    s = GaussianSampler(False, backend=backend, host=host)
    s.preprocess(t[0], t[1], None, t[2], pts)
    assert (s._plan is not None) == (backend == "binned")
    return s, t


def call(s, name, tau, prev, target):
    if name == "linear":
        return s.residual(a0=1.7, lap=-0.01, target=target)
    if name == "general":
        return s.residual(a0=tau, lap=-0.01, advect=0.5)
    if name == "coupled":
        return s.residual(a0=1.7, lap=-0.01, couple_weight=tau, couple0=QA, couple_lap=QB)
    if name == "vorticity_terms":
        return s.vorticity_terms()
    return s.vorticity_residual(NU, DT, prev, tau)


@pytest.mark.parametrize("host", HOSTS)
@pytest.mark.parametrize("backend", ["dense", "binned"])
def test_merged_node_keeps_the_operators_apart(hip_lib, host, backend):
    base, pts, tau, prev, target, weights = problem(backend)

    def leaves(name, t, tgt):
        return t + [tgt] if name == "linear" else t

    alone = {}
    for name in NODES:
        s, t = bound_sampler(host, backend, base, pts)
        tgt = target.clone().requires_grad_(True)
        alone[name] = torch.autograd.grad((call(s, name, tau, prev, tgt) * weights[name]).sum(), leaves(name, t, tgt))

    s, t = bound_sampler(host, backend, base, pts)
    tgt = target.clone().requires_grad_(True)
    outs = {name: call(s, name, tau, prev, tgt) for name in NODES}
    for name, out in outs.items():
        assert out.grad_fn.name() == NODES[name][host == "native"], (name, out.grad_fn.name())
    for name in reversed(list(NODES)):
        got = torch.autograd.grad((outs[name] * weights[name]).sum(), leaves(name, t, tgt))
        errs = [rel(g, a) for g, a in zip(got[:3], alone[name][:3])]
        print(backend, host, name, "gradients (means, values, conics) against the operator alone:", errs)
        assert all(torch.isfinite(g).all() for g in got) and max(errs) < 1e-5, (name, errs)
        if name == "linear":
            assert torch.equal(got[3], -weights[name]) and torch.equal(alone[name][3], -weights[name])
