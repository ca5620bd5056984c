"""GPU: every instantiation of the dense kernels (pigs_amd/csrc/dense.hip: 2 dtypes x 2 dimensions x 4 channel counts x
10 covering masks) through every launch variant it can take, against the float64 oracle.

The shapes S1..S7 are the smallest that put a launch on an edge of its selection (tests/test_dense_matrix.py asks the
launchers' own choice functions and asserts, without a GPU, that the case list below covers the table); STORE_N x STORE_M is the smallest
problem whose backward stores its sums directly (gridDim.y == 1) instead of adding them into zeroed buffers.

Expectations: oracle/c_oracle.py in float64 on the inputs as the kernel saw them (rounded to the test's dtype).  The
oracle's VJP is linear in the incoming gradients, so it runs once per order (and once for the trace) with one random
r_k each, and an order set's expected gradient is the sum over its orders.

Bars, each the project's own:
  float64          outputs and gradients within 1e-11 of the largest entry (tests/test_residual_terms_gpu.py)
  float32 outputs  within 1e-5 of the largest output (F32_TOL of tests/test_parity_gpu.py)
  float32 grads    every entry within conftest.grads_within_accumulation_bound's bound (ulps = floor = 1e-6), the
                   magnitudes being the sum over the set's orders of the oracle's absolute sums -- never below the
                   magnitude of the combined call (triangle inequality)
  float32 general residual with advection: tests/test_residual_terms_gpu.py's check_against_own_composition
  the far Gaussian (width 1e-5, at least 0.6 from every point: its weight is exactly 0 and p^4 overflows in float32):
                   all its gradients are exactly 0; every output and gradient is finite

Measured on an MI355X, the worst error as a fraction of its bar over all 116 tests (the forward variants carry the
outputs, the backward variants the gradients); no case needed another bar:
                 rows     w16      w4       staged32  staged64  split_atomic  split_store
  float32        0.076    0.026    0.038    0.66      0.18      0.058         0.060
  float64        1.9e-4   1.3e-4   1.7e-4   2.6e-4    8.9e-4    2.4e-3        2.1e-5
  float32 general residual with advection against its own composition: forward 7.1e-7 of the term scale (bar 2e-6),
  gradients 1.1e-6 of the largest entry (bar 5e-6)
The matrix catches what it is for: with the rows forward reading its second chunk of conics one record early, all 16
S1 tests fail and nothing else; with the direct-store backward adding into its buffers instead of storing, all four
direct-store tests fail (NaN: the buffers were handed back dirty) and nothing else.
"""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# ---- the case list: plain data (tests/test_dense_matrix.py reads it without a GPU)
SHAPES = (("S1", None, 81),         # N = rows chunk + 33: a second LDS chunk of 33 Gaussians; last 16-point workgroup holds one point
          ("S2", 128, 1),           # rows at its smallest N; one point
          ("S3", 127, 97),          # one Gaussian short of rows: w16 where it exists; last backward slice holds one point
          ("S4", 63, 130),          # one Gaussian short of w16: w4 for everyone, a partly filled wave of Gaussians
          ("S5", 300, 16350),       # 256 blocks: the last that take rows; staged backward of 64-point slices at its threshold
          ("S6", 130, 16445),       # 257 blocks: w16 / w4; split backward, 65 slices of 253 points
          ("S7", 70, 65473))        # 1 024 blocks: w4 also where w16 exists; split backward, 256 slices
INSTANCES = [(t, d, c) for t in ("float32", "float64") for d in (1, 2) for c in (1, 2, 3, 4)]
# S1's N, the instantiation's rows chunk + 33 (tests/test_dense_matrix.py holds each to the library's chunk)
S1_N = {("float32", 1): (3105, 2337, 1876, 1569), ("float32", 2): (1569, 1349, 1185, 1057),
        ("float64", 1): (1569, 1185, 954, 801), ("float64", 2): (801, 691, 609, 545)}       # c = 1 .. 4
CASES = [(t, d, c, name, N if N is not None else S1_N[t, d][c - 1], M) for t, d, c in INSTANCES for name, N, M in SHAPES]
# (orders of one sample() call, the outputs its loss reads: None = all of them)
ORDER_SETS = [((0,), None), ((1,), None), ((2,), None), ((3,), None), (("lap",), None), ((0, 1, 2), None),
              ((0, 1, 2, 3), None), ((0, 1, "lap"), None),
              ((0, 2), None), ((1, 2), None), ((0, 3), None), ((1, 3), None), ((0, "lap"), None), ((1, "lap"), None),
              ((0, 1, 2, 3), (1, 3))]
RESIDUAL_MASKS = (32, 64)      # residual() with float coefficients / with per-point fields
STORE_N, STORE_M = 65537, 16385
STORE_CASES = [("float32", 2, 1, (0, 1, 2)), ("float32", 2, 2, (0, 1, "lap")), ("float64", 1, 1, (0, 1, 2, 3)),
               ("float32", 2, 1, "advect")]

F64_TOL, F32_TOL, ULPS, FLOOR = 1e-11, 1e-5, 1e-6, 1e-6
FAR_AT, FAR_CONIC = 1.7, 1e10       # points live in [-1.1, 1.1]^d
A0, A1, AL = 1.25, (0.5, -0.25), -0.0078125      # the linear residual's coefficients: exact in float32


def np64(x):
    return x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def problem(rng, d, c, N, M):
    """means [N, d], values [N, c], flat conics, points [M, d] in float64, and the index of the far Gaussian."""
    n = N - 1
    means = rng.uniform(-1, 1, (n, d))
    pts = 1.1 * rng.uniform(-1, 1, (M, d))
    sig = 2.0 / n ** (1.0 / d) * np.exp(rng.normal(0, 0.35, (n, d)))
    if d == 2:
        rho = rng.uniform(-0.9, 0.9, n)
        s0, s1 = sig[:, 0], sig[:, 1]
        det = (s0 * s1) ** 2 * (1 - rho ** 2)
        con = np.stack((s1 ** 2 / det, -rho * s0 * s1 / det, s0 ** 2 / det), -1)
    else:
        con = 1.0 / sig ** 2
    values = rng.uniform(-1, 1, (n, c))
    far = int(rng.integers(0, N))
    means = np.insert(means, far, np.full(d, FAR_AT), axis=0)
    con = np.insert(con, far, (FAR_CONIC, 0.0, FAR_CONIC) if d == 2 else (FAR_CONIC,), axis=0)
    values = np.insert(values, far, rng.uniform(-1, 1, c), axis=0)
    assert np.abs(pts - FAR_AT).max(-1).min() >= 0.5
    return means, values, con, pts, far


def out_shape(o, M, d, c):
    return (M, c) if o == "lap" else (M,) + (d,) * o + (c,)


def as_order_grads(o, r, d):
    """The incoming gradient of output ``o`` as the oracle's {order: array} (the trace arrives on the diagonal)."""
    if o != "lap":
        return {o: r}
    g2 = np.zeros((r.shape[0], d, d, r.shape[1]))
    for i in range(d):
        g2[:, i, i] = r
    return {2: g2}


class Worst:
    """The worst error / bar per (dtype, launch variant), and the checks that failed."""

    def __init__(self, dtype):
        self.dtype, self.worst, self.failed = dtype, {}, []

    def note(self, variant, what, ratio):
        ratio = float(ratio)
        self.worst[variant] = max(self.worst.get(variant, 0.0), ratio)
        if not ratio <= 1.0:
            self.failed.append((variant, what, ratio))

    def require(self, ok, what):
        if not ok:
            self.failed.append(what)

    def report(self):
        for variant in sorted(self.worst):
            print(f"worst of the bar: {self.dtype} {variant} {self.worst[variant]:.3g}")
        assert not self.failed, self.failed


class Case:
    """One problem on the device, its oracle outputs and the per-order oracle gradients (each computed once)."""

    def __init__(self, dtype, d, c, N, M, key):
        from oracle import c_oracle
        self.dtype, self.tdt, self.d, self.c, self.N, self.M = dtype, getattr(torch, dtype), d, c, N, M
        self.f32 = dtype == "float32"
        self.rng = np.random.default_rng(seed_of(key))
        means, values, con, pts, self.far = problem(self.rng, d, c, N, M)
        self.t = [self.dev(a) for a in (means, values, con, pts)]
        for x in self.t[:3]:
            x.requires_grad_(True)
        self.leaves = (self.t[0], self.t[2], self.t[1])                      # means, conics, values: the oracle's order
        self.args = [np64(x) for x in (self.t[0], self.t[2], self.t[1], self.t[3])]
        self.oracle = c_oracle
        self.w = Worst(dtype)

    def dev(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.tdt, device="cuda")

    def sampler(self):
        from diff_gaussian_sampling import GaussianSampler
        s = GaussianSampler(True, backend="dense")
        s.preprocess(self.t[0], self.t[1], None, self.t[2], self.t[3])
        assert s._plan is None
        return s

    def draw(self, shape):
        """uniform in [-1, 1], rounded to the dtype: (device tensor, float64 array)"""
        r = self.dev(self.rng.uniform(-1, 1, shape))
        return r, np64(r)

    def piece(self, o, r64, sel=None):
        """(gradient, absolute sums or None) of the oracle for r64 arriving at output o alone"""
        a = self.args if sel is None else [x[sel] for x in self.args[:3]] + [self.args[3]]
        g = as_order_grads(o, r64, self.d)
        return (self.oracle.backward(*a, g), self.oracle.backward(*a, g, absolute=True) if self.f32 else None)

    # ---- the bars
    def check_output(self, variant, what, got, want, scale=None):
        got = np64(got).reshape(want.shape)
        self.w.require(np.isfinite(got).all(), (what, "not finite"))
        scale = np.abs(want).max() if scale is None else scale
        err = np.abs(got - want).max() / max(scale, 1e-300)
        self.w.note(variant, what, err / (F32_TOL if self.f32 else F64_TOL))

    def check_grads(self, variant, what, got, want, mags, far=None, floor_scale=None):
        """got, want, mags: (means, conics, values) triples; mags: the absolute sums (float32)"""
        for name, g, w, k in zip(("means", "conics", "values"), got, want, range(3)):
            g = np64(g).reshape(w.shape)
            self.w.require(np.isfinite(g).all(), (what, name, "not finite"))
            top = max(np.abs(w).max() if floor_scale is None else floor_scale[k], 1e-300)
            if self.f32:
                ratio = (np.abs(g - w) / (ULPS * mags[k] + FLOOR * top)).max()
            else:
                ratio = np.abs(g - w).max() / top / F64_TOL
            self.w.note(variant, (what, name), ratio)
            if far is not None:
                self.w.require((g[far] == 0).all(), (what, name, "the far Gaussian's gradient is not 0", g[far].tolist()))


def run_matrix_case(dtype, d, c, name, N, M):
    import test_dense_matrix as table        # the variants' names: asked of the launchers' choice functions
    import test_residual_terms_gpu as R
    cs = Case(dtype, d, c, N, M, (dtype, d, c, name))
    oracle, rng, args = cs.oracle, cs.rng, cs.args
    exp = oracle.forward(*args, orders=(0, 1, 2, 3))
    exp["lap"] = sum(exp[2][:, i, i] for i in range(d))
    r = {o: cs.draw(out_shape(o, M, d, c)) for o in (0, 1, 2, 3, "lap")}
    pieces = {o: cs.piece(o, r[o][1]) for o in r}
    bvar = table.choice(dtype, d, c, 1, N, M).backward
    s = cs.sampler()

    # ---- sample(): every covering mask alone, requests with holes, a backward with holes the forward did not have
    for orders, reads in ORDER_SETS:
        reads = orders if reads is None else reads
        fmask, _ = table.masks_of(orders, reads)
        fvar = table.choice(dtype, d, c, fmask, N, M).forward
        s.preprocess(cs.t[0], cs.t[1], None, cs.t[2], cs.t[3])          # forget the outputs of the previous set
        outs = s.sample(orders)
        for o, out in zip(orders, outs):
            assert tuple(out.shape) == out_shape(o, M, d, c) and out.dtype == cs.tdt
            cs.check_output(fvar, (orders, "output", o), out, exp[o])
        loss = sum((out * r[o][0]).sum() for o, out in zip(orders, outs) if o in reads)
        got = torch.autograd.grad(loss, cs.leaves)
        want = [sum(pieces[o][0][k] for o in reads) for k in range(3)]
        mags = [sum(pieces[o][1][k] for o in reads) for k in range(3)] if cs.f32 else None
        cs.check_grads(bvar, (orders, reads, "gradient"), got, want, mags, far=cs.far)

    # ---- residual(): float coefficients (mask 32), per-point fields without and with advection (mask 64)
    tgt, tgt64 = cs.draw((M, c))
    w, w64 = cs.draw((M, c))
    B64 = np64(cs.dev(rng.uniform(-1, 1, (d, c))))                      # a non-identity advect_by, as the kernel sees it
    B = tuple(tuple(float(x) for x in row) for row in B64)
    consts = (np.full(M, A0), np.tile(np.asarray(A1[:d]), (M, 1)), np.full(M, AL), None)
    Fn = tuple(cs.dev(a) for a in R.fields(rng, M, d, advect=False)[:3]) + (None,)
    Fa = tuple(cs.dev(a) for a in R.fields(rng, M, d))
    for mask, what, F, call in (
            (32, "linear residual", consts, lambda t_: s.residual(a0=A0, a1=A1[:d], lap=AL, target=t_)),
            (64, "fields", Fn, lambda t_: R.call(s, Fn, B, t_)),
            (64, "fields + advection", Fa, lambda t_: R.call(s, Fa, B, t_))):
        F64 = tuple(None if a is None else np64(a) for a in F)
        fvar = table.choice(dtype, d, c, mask, N, M).forward
        want_r = R.compose(exp, F64, B64, tgt64, d)
        t_ = tgt.clone().requires_grad_(True)
        res = call(t_)
        assert tuple(res.shape) == (M, c) and res.dtype == cs.tdt
        cs.check_output(fvar, (what, "output"), res, want_r)
        got = torch.autograd.grad((res * w).sum(), cs.leaves + (t_,))
        cs.w.require(torch.equal(got[3], -w), (what, "the target's gradient is not -w"))
        inc = R.incoming(w64, exp, F64, B64, d, c)
        if cs.f32 and F[3] is not None:
            # the kernel forms the incoming gradients from its own float32 u and grad u: against torch.autograd through
            # the same expression on the sampler's own outputs; what the oracle still says: finite, and 0 for the far one
            R.check_against_own_composition(s, (cs.t[0], cs.t[1], cs.t[2]), F, B, tgt, d, w)
            for g in got[:3]:
                cs.w.require(bool(torch.isfinite(g).all()) and bool((g[cs.far] == 0).all()), (what, "far / finite"))
            continue
        want = oracle.backward(*args, inc)
        mags = oracle.backward(*args, inc, absolute=True) if cs.f32 else None
        cs.check_grads(bvar, (what, "gradient"), got[:3], want, mags, far=cs.far)
    cs.w.report()


@pytest.mark.parametrize("dtype,d,c,name,N,M", CASES, ids=[f"{t}-d{d}-c{c}-{n}" for t, d, c, n, _, _ in CASES])
def test_matrix(hip_lib, dtype, d, c, name, N, M):
    run_matrix_case(dtype, d, c, name, N, M)


# ------------------------------------------------------------------------------------------
# the backward that stores directly
# ------------------------------------------------------------------------------------------
def dirty_the_allocator(cs):
    """Blocks full of NaN go back to the caching allocator: one of the gradient buffer's own size (the sampler's three
    gradients are views of one allocation) and a large one, so that the backward's torch.empty is no fresh zero page."""
    nf = cs.d * (cs.d + 1) // 2
    junk = [torch.empty(cs.N * (cs.d + nf + cs.c), dtype=cs.tdt, device="cuda").fill_(float("nan")),
            torch.empty(1 << 26, dtype=torch.float32, device="cuda").fill_(float("nan"))]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("dtype,d,c,what", STORE_CASES, ids=[f"{t}-d{d}-c{c}-{'-'.join(map(str, w)) if w != 'advect' else w}"
                                                             for t, d, c, w in STORE_CASES])
def test_direct_store_backward(hip_lib, dtype, d, c, what):
    """N = 65 537 Gaussians give 1 025 workgroups, so the split backward keeps one slice of the points and stores its
    sums without atomics, into buffers nobody zeroed.  The oracle takes 512 points for the outputs and 512 Gaussians
    (the first and the last workgroup and a random rest; a Gaussian's gradient needs no other Gaussian) against all
    points for the gradients; every entry must be finite."""
    import test_dense_matrix as table
    import test_residual_terms_gpu as R
    N, M = STORE_N, STORE_M
    assert table.choice(dtype, d, c, 1, N, M).backward == "split_store"
    cs = Case(dtype, d, c, N, M, (dtype, d, c, what, "store"))
    oracle, rng, args = cs.oracle, cs.rng, cs.args
    psel = np.unique(np.concatenate((np.arange(64), np.arange(M - 64, M), rng.choice(M, 384, replace=False))))
    gsel = np.unique(np.concatenate((np.arange(64), np.arange(N - 64, N), [cs.far], rng.choice(N, 383, replace=False))))
    far_in_sel = int(np.searchsorted(gsel, cs.far))
    s = cs.sampler()
    if what == "advect":
        exp = oracle.forward(*args[:3], args[3][psel], orders=(0, 1, 2))
        F = tuple(cs.dev(a) for a in R.fields(rng, M, d))
        B64 = np64(cs.dev(rng.uniform(-1, 1, (d, c))))
        B = tuple(tuple(float(x) for x in row) for row in B64)
        tgt, tgt64 = cs.draw((M, c))
        w, _ = cs.draw((M, c))
        res = R.call(s, F, B, tgt)
        want = R.compose(exp, tuple(np64(a)[psel] for a in F), B64, tgt64[psel], d)
        cs.w.require(bool(torch.isfinite(res).all()), "output not finite")
        cs.check_output(table.choice(dtype, d, c, 64, N, M).forward, "output", res[psel], want,
                        scale=float(res.detach().abs().max()))
        dirty_the_allocator(cs)
        got = torch.autograd.grad((res * w).sum(), (cs.t[0], cs.t[1], cs.t[2]))
        for g in got:
            cs.w.require(bool(torch.isfinite(g).all()) and bool((g[cs.far] == 0).all()), "far / finite")
        dirty_the_allocator(cs)
        R.check_against_own_composition(s, (cs.t[0], cs.t[1], cs.t[2]), F, B, tgt, d, w)
        cs.w.report()
        return
    fmask, _ = table.masks_of(what)
    exp = oracle.forward(*args[:3], args[3][psel], orders=tuple(o for o in what if o != "lap") + ((2,) if "lap" in what else ()))
    if "lap" in what:
        exp["lap"] = sum(exp[2][:, i, i] for i in range(d))
    outs = s.sample(what)
    r = {o: cs.draw(out_shape(o, M, d, c)) for o in what}
    for o, out in zip(what, outs):
        cs.w.require(bool(torch.isfinite(out).all()), (o, "output not finite"))
        cs.check_output(table.choice(dtype, d, c, fmask, N, M).forward, ("output", o), out[psel], exp[o],
                        scale=float(out.detach().abs().max()))
    loss = sum((out * r[o][0]).sum() for o, out in zip(what, outs))
    dirty_the_allocator(cs)
    got = torch.autograd.grad(loss, cs.leaves)
    for g in got:
        cs.w.require(bool(torch.isfinite(g).all()) and bool((g[cs.far] == 0).all()), "far / finite")
    pieces = [cs.piece(o, r[o][1], gsel) for o in what]
    want = [sum(p[0][k] for p in pieces) for k in range(3)]
    mags = [sum(p[1][k] for p in pieces) for k in range(3)] if cs.f32 else None
    cs.check_grads("split_store", "gradient", [g[gsel] for g in got], want, mags, far=far_in_sel,
                   floor_scale=[float(g.detach().double().abs().max()) for g in got])
    cs.w.report()
