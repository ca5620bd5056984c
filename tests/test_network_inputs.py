"""CPU: GaussianSampler.network_inputs() -- the four arrays of the reference's Model.forward (model_pn.py:645-664) --
without a GPU: the float64 recipe that the GPU tests (tests/test_network_inputs_gpu.py) take their expectations from,
held to the reference's own recordings; the planted mistakes that the bars must see; the C symbol, its ctypes signature
and its refusals; and what the dense launchers' choice functions say about the two new masks.

  recipe(out, pde, nu, wave)        the four arrays from orders 0..3 ({order: array} as oracle/dense_numpy.forward
                                    returns them), numpy or torch, with the five pde_rhs lines of :612-631 restated
  scales(mag, pde, nu, wave)        the same compositions over magnitudes (the oracle's absolute=True pair sums): what a
                                    float32 error is measured against where a sum cancels
"""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PDES = ("zero", "diffusion", "burgers", "wave", "navier_stokes")
NAMES = ("sample_u", "sample_ux", "sample_uxx", "sample_pde")
ORDI, ORDJ = 1024, 2048
BAR64 = 1e-12
FLOOR32 = 1e-5          # the float32 bar of the GPU file: err <= 4 err_torch32 + FLOOR32 x scale


def _lib_of(a):
    if isinstance(a, np.ndarray):
        return np, dict(axis=-1)
    import torch
    return torch, dict(dim=-1)


def pde_rhs(pde, u, ux, uxx, wx=None, wxx=None, nu=0.0, wave=(10.0, 0.1)):
    """model_pn.py:612-631 with its index expressions; ``zero`` is Problem.TEST"""
    xp, last = _lib_of(u)
    if pde == "diffusion":
        return uxx[:, 0, 0] + uxx[:, 1, 1]
    if pde == "burgers":
        return nu * (uxx[:, 0, 0] + uxx[:, 1, 1]) - u * ux[:, 0]
    if pde == "wave":
        return xp.stack((u[..., 1], wave[0] * (uxx[..., 0, 0, 0] + uxx[..., 1, 1, 0]) - wave[1] * u[..., 1]), **last)
    if pde == "navier_stokes":
        return nu * (wxx[:, 0, 0] + wxx[:, 1, 1]) - (u[:, 0] * wx[:, 0] + u[:, 1] * wx[:, 1])
    assert pde == "zero"
    return xp.zeros_like(u)


def recipe(out, pde, nu=0.0, wave=(10.0, 0.1)):
    """model_pn.py:650-664 on the outputs of orders 0, 1, 2 (and 3 for Navier-Stokes)"""
    xp, last = _lib_of(out[0])
    n = out[0].shape[0]
    sample_u, sample_ux, sample_uxx = out[0], out[1], out[2]
    if pde == "navier_stokes":
        sample_uxxx = out[3]
        sample_wx = sample_uxx[..., 0, 1] - sample_uxx[..., 1, 0]
        sample_wxx = sample_uxxx[..., 0, 1] - sample_uxxx[..., 1, 0]
        sample_pde = pde_rhs(pde, sample_u, sample_ux, sample_uxx, sample_wx, sample_wxx, nu=nu, wave=wave).reshape(n, -1)
    else:
        sample_pde = pde_rhs(pde, sample_u, sample_ux, sample_uxx, nu=nu, wave=wave).reshape(n, -1)
    cat = np.concatenate if xp is np else xp.cat
    return {"sample_u": sample_u, "sample_ux": sample_ux.reshape(n, -1),
            "sample_uxx": cat((sample_uxx[:, 0, 0], sample_uxx[:, 1, 1]), **last).reshape(n, -1), "sample_pde": sample_pde}


def scales(mag, pde, nu=0.0, wave=(10.0, 0.1)):
    """The sum of the absolute terms of every composed value, per entry, with each sampled quantity replaced by its
    magnitude ``mag`` = the oracle's absolute=True pair sums: the recipe with every minus turned into a plus."""
    n = mag[0].shape[0]
    lap = mag[2][:, 0, 0] + mag[2][:, 1, 1]
    if pde == "zero":
        s_pde = np.zeros_like(mag[0])
    elif pde == "diffusion":
        s_pde = lap
    elif pde == "burgers":
        s_pde = abs(nu) * lap + mag[0] * mag[1][:, 0]
    elif pde == "wave":
        s_pde = np.stack((mag[0][:, 1], abs(wave[0]) * lap[:, 0] + abs(wave[1]) * mag[0][:, 1]), -1)
    else:
        wx = mag[2][..., 0, 1] + mag[2][..., 1, 0]
        wxx = mag[3][..., 0, 1] + mag[3][..., 1, 0]
        s_pde = abs(nu) * (wxx[:, 0, 0] + wxx[:, 1, 1]) + mag[0][:, 0] * wx[:, 0] + mag[0][:, 1] * wx[:, 1]
    return {"sample_u": mag[0], "sample_ux": mag[1].reshape(n, -1),
            "sample_uxx": np.concatenate((mag[2][:, 0, 0], mag[2][:, 1, 1]), -1).reshape(n, -1), "sample_pde": s_pde.reshape(n, -1)}


def full_conics(flat):
    flat = np.asarray(flat, dtype=np.float64)
    return np.stack((np.stack((flat[:, 0], flat[:, 1]), -1), np.stack((flat[:, 1], flat[:, 2]), -1)), -2)


def flat_conics(full):
    return np.stack((full[:, 0, 0], full[:, 0, 1], full[:, 1, 1]), -1)


def oracle_outputs(means, conics_full, values, samples, absolute=False):
    """{order: array} of orders 0..3 from oracle/dense_numpy.forward; ``absolute``: every pair's term in absolute value"""
    from oracle import dense_numpy
    if absolute:
        mask = np.ones((len(samples), len(means)), dtype=bool)
        return dense_numpy.forward(means, conics_full, values, samples, orders=(0, 1, 2, 3), pair_mask=mask, absolute=True)
    return dense_numpy.forward(means, conics_full, values, samples, orders=(0, 1, 2, 3))


# ---- the recordings -----------------------------------------------------------------------------------------
FIXTURES = {"diffusion": ("diffusion", 0.0), "navier_stokes": ("navier_stokes", 1e-3)}      # file: (pde, nu)
TRACES = {"burgers": ("burgers", 0.01), "wave": ("wave", 0.0), "test": ("zero", 0.0)}       # file: (pde, nu)
WAVE = (10.0, 0.1)


def load_recorded(name):
    """(means, full conics, u, {name: recorded array}) of tests/golden/input_transform/<name>.npz, float64"""
    fx = np.load(os.path.join(GOLDEN, "input_transform", name + ".npz"))
    conics = np.linalg.inv(fx["in/full_covariances"])
    conics = 0.5 * (conics + conics.transpose(0, 2, 1))
    return fx["in/means"], conics, fx["in/u"], {k: fx["in/" + k] for k in NAMES}


def load_trace_records(name):
    """The M = N records with three calls of tests/golden/model_pn_trace_<name>.npz (Model.forward's sampling at the
    means): [(means, full conics, values, {0, 1, 2: recorded output})], float64"""
    z = np.load(os.path.join(GOLDEN, f"model_pn_trace_{name}.npz"))
    out = []
    for k in range(int(z["n_records"])):
        means, samples = z[f"r{k}_means"], z[f"r{k}_samples"]
        if list(z[f"r{k}_calls"]) == [0, 1, 2] and means.shape == samples.shape and np.array_equal(means, samples):
            out.append((means.astype(np.float64), full_conics(z[f"r{k}_conics"]), z[f"r{k}_values"].astype(np.float64),
                        {o: z[f"r{k}_out{o}"] for o in range(3)}))
    return out


def worst_relative(got, want):
    """{name: max |got - want| / max |want|}"""
    return {k: float(np.abs(got[k] - want[k]).max() / max(np.abs(want[k]).max(), 1e-300)) for k in NAMES}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_recipe_reproduces_the_recorded_forward(name):
    pde, nu = FIXTURES[name]
    means, conics, u, rec = load_recorded(name)
    got = recipe(oracle_outputs(means, conics, u, means), pde, nu=nu, wave=WAVE)
    for k in NAMES:
        assert got[k].shape == rec[k].shape, (k, got[k].shape, rec[k].shape)
    e = worst_relative(got, rec)
    print(f"[figure] {name}: worst error of the recipe relative to each recorded array's maximum {max(e.values()):.3g}")
    assert max(e.values()) <= BAR64, e


@pytest.mark.parametrize("name", sorted(TRACES))
def test_the_recipe_reproduces_the_recorded_traces(name):
    pde, nu = TRACES[name]
    records = load_trace_records(name)
    assert records, "no M = N record with three calls"
    worst = 0.0
    for means, conics, values, outs in records:
        want = recipe(outs, pde, nu=nu, wave=WAVE)
        got = recipe(oracle_outputs(means, conics, values, means), pde, nu=nu, wave=WAVE)
        for k in NAMES:
            scale = max(np.abs(want[k]).max(), 1e-300)
            worst = max(worst, float(np.abs(got[k] - want[k]).max() / scale))
            assert got[k].shape == want[k].shape
    print(f"[figure] {name}: {len(records)} records, worst error relative to each array's maximum {worst:.3g}")
    assert worst <= BAR64


# ---- the planted mistakes -----------------------------------------------------------------------------------
def _swap_halves(a):
    h = a.shape[1] // 2
    return np.concatenate((a[:, h:], a[:, :h]), -1)


def _interleave(a):          # planar (xx of every channel, then yy) -> per channel (xx, yy)
    h = a.shape[1] // 2
    return np.stack((a[:, :h], a[:, h:]), -1).reshape(a.shape[0], -1)


def mistakes(out, pde, nu, wave):
    """{name: (array it shows in, the four arrays with the mistake)} for the mistakes this right-hand side can show"""
    right = recipe(out, pde, nu=nu, wave=wave)
    c = out[0].shape[1]
    m = {}
    m["u_xx and u_yy exchanged"] = ("sample_uxx", dict(right, sample_uxx=_swap_halves(right["sample_uxx"])))
    if c > 1:
        m["the diagonal interleaved per channel"] = ("sample_uxx", dict(right, sample_uxx=_interleave(right["sample_uxx"])))
        m["sample_ux as [c][d]"] = ("sample_ux", dict(right, sample_ux=out[1].transpose(0, 2, 1).reshape(len(out[0]), -1)))
    if pde in ("burgers", "navier_stokes"):
        m["nu dropped"] = ("sample_pde", recipe(out, pde, nu=0.0, wave=wave))
        flipped = {0: -out[0], 1: out[1], 2: out[2], 3: out.get(3)}      # - u . grad: the advection's sign
        adv = recipe(flipped, pde, nu=nu, wave=wave)["sample_pde"]
        m["the advection's sign"] = ("sample_pde", dict(right, sample_pde=adv))
    if pde == "navier_stokes":
        o2 = out[2][:, ::-1]              # d_x and d_y of the first derivative index exchanged: w_x <-> w_y
        sw = recipe({0: out[0], 1: out[1], 2: o2, 3: out[3]}, pde, nu=nu, wave=wave)["sample_pde"]
        m["w_x and w_y exchanged"] = ("sample_pde", dict(right, sample_pde=sw))
        m["w with the wrong sign"] = ("sample_pde", dict(right, sample_pde=-right["sample_pde"]))
    if pde == "wave":
        m["the wave's two outputs exchanged"] = ("sample_pde", dict(right, sample_pde=right["sample_pde"][:, ::-1]))
    return right, m


def seeded_scene(c, N=97, seed=5):
    """Gaussians on a jittered lattice with anisotropic, correlated covariances and values of both signs, sampled at
    their means: a scene in which no two of the checked quantities coincide"""
    rng = np.random.default_rng(seed + 10 * c)
    means = rng.uniform(-1, 1, (N, 2))
    sig = 0.25 * np.exp(rng.normal(0, 0.3, (N, 2)))
    rho = rng.uniform(-0.7, 0.7, N)
    cov = np.stack((np.stack((sig[:, 0] ** 2, rho * sig[:, 0] * sig[:, 1]), -1),
                    np.stack((rho * sig[:, 0] * sig[:, 1], sig[:, 1] ** 2), -1)), -2)
    conics = np.linalg.inv(cov)
    return means, 0.5 * (conics + conics.transpose(0, 2, 1)), rng.uniform(-1, 1, (N, c))


def _scenes_for_mistakes():
    """(label, pde, nu, means, conics, values): the recorded scenes, and a seeded one per right-hand side"""
    for name, (pde, nu) in FIXTURES.items():
        means, conics, u, _ = load_recorded(name)
        yield "recorded " + name, pde, nu, means, conics, u
    for name, (pde, nu) in TRACES.items():
        means, conics, values, _ = load_trace_records(name)[0]
        yield "trace " + name, pde, nu, means, conics, values
    for pde, c, nu in (("diffusion", 2, 0.0), ("burgers", 2, 0.05), ("wave", 2, 0.0), ("navier_stokes", 2, 0.05), ("zero", 3, 0.0)):
        yield "seeded " + pde, pde, nu, *seeded_scene(c)


def test_the_bar_sees_every_planted_mistake():
    """Each mistake moves the array it shows in by at least 100 x the float32 allowance's floor, FLOOR32 x scale, in at
    least one scene; a scene that cannot see a mistake is named, and every mistake is seen by a seeded scene."""
    seen, blind = {}, []
    for label, pde, nu, means, conics, values in _scenes_for_mistakes():
        out = oracle_outputs(means, conics, values, means)
        mag = oracle_outputs(means, conics, values, means, absolute=True)
        right, wrong = mistakes(out, pde, nu, WAVE)
        sc = scales(mag, pde, nu=nu, wave=WAVE)
        for what, (k, arrays) in wrong.items():
            moved = float(np.abs(arrays[k] - right[k]).max())
            floor = FLOOR32 * float(sc[k].max())
            ok = moved >= 100 * floor
            seen.setdefault(what, []).append((label, ok))
            if not ok:
                blind.append(f"{label} does not see '{what}': moved {moved:.3g}, 100 x floor {100 * floor:.3g}")
    for line in blind:
        print("[figure]", line)
    expected = {"u_xx and u_yy exchanged", "the diagonal interleaved per channel", "sample_ux as [c][d]", "nu dropped",
                "the advection's sign", "w_x and w_y exchanged", "w with the wrong sign", "the wave's two outputs exchanged"}
    assert set(seen) == expected
    for what, where in seen.items():
        assert any(ok for label, ok in where if label.startswith("seeded")), (what, where)


# ---- the symbol ---------------------------------------------------------------------------------------------
def test_the_public_names():
    import pigs_amd
    from pigs_amd import sampler
    assert pigs_amd.NETWORK_PDES == PDES and pigs_amd.NETWORK_PDES is sampler.NETWORK_PDES
    assert sampler.NetworkInputs._fields == NAMES
    assert callable(sampler.GaussianSampler.network_inputs)
    assert "model_pn.py:645-664" in sampler.GaussianSampler.network_inputs.__doc__


def test_both_cores_have_the_method(hip_lib):
    import inspect
    from pigs_amd import _pigs_host, host_ctypes
    native = _pigs_host.SamplerCore._network_inputs.__doc__.splitlines()[0]
    import re
    assert re.findall(r"[(,] ?(\w+): ", native)[1:] == ["kind", "nu", "wave0", "wave1"], native
    assert list(inspect.signature(host_ctypes.SamplerCore._network_inputs).parameters) == ["self", "kind", "nu", "wave0", "wave1"]


def test_lib_binds_the_symbol_with_the_documented_arguments(hip_lib):
    """dtype, d, c, N, M, means, conics, values, samples, params, the four outputs, plan_ws, bytes, samples_ws, bytes,
    stream (19)"""
    from pigs_amd import _lib
    res, sig = _lib.SIGNATURES["pigs_network_inputs_forward"]
    assert res is ctypes.c_int and len(sig) == 19
    assert sig[:5] == [ctypes.c_int] * 3 + [ctypes.c_int64] * 2
    assert sig[9] is ctypes.POINTER(_lib.PigsNetworkInputs)
    assert all(a is ctypes.c_void_p for a in sig[5:9] + sig[10:14])
    assert sig[-5:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert [n for n, _ in _lib.PigsNetworkInputs._fields_] == ["kind", "nu", "wave"]
    assert ctypes.sizeof(_lib.PigsNetworkInputs) == 32
    assert hip_lib.pigs_network_inputs_forward.argtypes == sig
    assert hip_lib.pigs_abi_version() == 10              # additive: no version bump
    assert "pigs_network_inputs_backward" not in _lib.SIGNATURES and not hasattr(hip_lib, "pigs_network_inputs_backward")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pigs_amd.h")).read()
    assert "int pigs_network_inputs_forward(" in header and "} PigsNetworkInputs;" in header


def test_argument_validation_needs_no_gpu(hip_lib):
    """Bad arguments are rejected before any HIP call (1 = invalid, 2 = unsupported)."""
    from pigs_amd import _lib
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below returns before a launch
    f = hip_lib.pigs_network_inputs_forward

    def call(dtype=0, d=2, c=2, kind=1, params=True, outs=(one,) * 4, means=one, plan=(null, 0, null, 0)):
        pz = ctypes.byref(_lib.PigsNetworkInputs(kind, 0.05, WAVE)) if params else None
        return f(dtype, d, c, 4, 4, means, one, one, one, pz, *outs, *plan, null)
    assert call(d=1) == 2                                                            # the model is two-dimensional
    assert call(d=1, c=1, kind=0) == 2
    for kind in (PDES.index("wave"), PDES.index("navier_stokes")):
        for c in (1, 3, 4):
            assert call(c=c, kind=kind) == 2, (kind, c)                              # two channels only
    assert call(kind=5) == 1 and call(kind=-1) == 1                                  # an unknown kind
    for k in range(4):                                                               # a null output with M > 0
        assert call(outs=tuple(null if i == k else one for i in range(4))) == 1, k
    assert call(params=False) == 1
    assert call(means=null) == 1
    assert call(dtype=7) == 2
    assert call(c=5) == 2 and call(d=3) == 2
    assert call(dtype=1, plan=(one, 64, one, 64)) == 2                               # binned float64


# ---- the choice functions -----------------------------------------------------------------------------------
def instantiations():
    """(dtype, c, mask) of every dense instantiation of the two masks"""
    return [(dt, c, ORDI) for dt in ("float32", "float64") for c in (1, 2, 3, 4)] + [(dt, 2, ORDJ) for dt in ("float32", "float64")]


# the forward variants every dense instantiation can take: the case list of tests/test_network_inputs_gpu.py, held to the
# choice functions' own answers below
VARIANTS = {("float32", 1, ORDI): ("rows", "w16", "w4"), ("float32", 2, ORDI): ("rows", "w4"), ("float32", 3, ORDI): ("rows", "w4"),
            ("float32", 4, ORDI): ("rows", "w4"), ("float64", 1, ORDI): ("rows", "w4"), ("float64", 2, ORDI): ("rows", "w4"),
            ("float64", 3, ORDI): ("w4",), ("float64", 4, ORDI): ("w4",), ("float32", 2, ORDJ): ("rows", "w4"),
            ("float64", 2, ORDJ): ("rows", "w4")}


def variants_of(dtype, c, mask):
    """the forward variants that choose_dense_forward can hand this instantiation, from its own flags"""
    import host_program as hp
    probe = hp.dense(dtype, 2, c, mask, 1600, 1600)
    return (("rows",) if probe.can_rows else ()) + (("w16",) if probe.can_w16 else ()) + ("w4",)


def test_the_choice_functions_know_both_masks():
    import host_program as hp
    table = {}
    for dtype, c, mask in instantiations():
        probe = hp.dense(dtype, 2, c, mask, 1600, 1600)
        assert probe.accumulators == (5 * c if mask == ORDI else 13), (dtype, c, mask, probe.accumulators)
        words = probe.accumulators * (2 if dtype == "float64" else 1)
        assert bool(probe.can_rows) == (words <= hp.constants()["ROWS_MAX_WORDS"])
        assert bool(probe.can_w16) == (words <= hp.constants()["W16_MAX_WORDS"])
        table[(dtype, c, mask)] = variants_of(dtype, c, mask)
        # every variant it can take is reached at some shape, and none it cannot
        reached = {hp.dense(dtype, 2, c, mask, N, M).forward for N, M in ((1600, 1600), (1600, 20000), (1600, 70000), (8, 8))}
        assert reached == set(table[(dtype, c, mask)]), (dtype, c, mask, reached)
    for key, v in sorted(table.items()):
        print("[figure] dense instantiation", key, "takes", v)
    assert table == VARIANTS
    assert hp.covering(ORDI) == ORDI and hp.covering(ORDJ) == ORDJ
    # the existing instantiation lists do not hold the new masks: they live in forward-only lists of their own
    for which in (("dense", 2, 2), ("binned", 2), ("fused", 2)):
        assert ORDI not in hp.instances(*which) and ORDJ not in hp.instances(*which)
