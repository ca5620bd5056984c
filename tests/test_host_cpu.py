"""CPU: host-side bookkeeping of the sampler that needs no device."""


def test_plan_pool_is_bounded_and_keyed():
    from pigs_amd.host_ctypes import _PlanPool
    pool = _PlanPool()
    for k in range(10):                                  # ten problem sizes, one dead plan each
        pool.give(("sizes", k), object())
    assert sum(len(v) for v in pool.free.values()) == pool.KEEP_TOTAL
    assert pool.take(("sizes", 0)) is None               # the oldest went back to the allocator
    a, b, c = object(), object(), object()
    for ws in (a, b, c):
        pool.give(("sizes", 9), ws)
    assert len(pool.free[("sizes", 9)]) == pool.KEEP     # per key
    assert sum(len(v) for v in pool.free.values()) <= pool.KEEP_TOTAL
    got = pool.take(("sizes", 9))
    assert got is not None and pool.take(("other", 9)) is None


def test_native_host_extension_loads_and_rejects_cpu_tensors(hip_lib):
    """The native host side (pigs_amd/_pigs_host.so) is built by build(), imports without a GPU, was
    compiled against the ABI the library reports, and has no CPU path: same errors as the ctypes host."""
    import pytest
    import torch
    from pigs_amd import _lib, _pigs_host
    from pigs_amd.sampler import GaussianSampler
    assert _pigs_host.ABI_VERSION == _lib.ABI_VERSION == _lib.load().pigs_abi_version()
    for name in ("SamplerCore", "Plan", "SamplePlan", "forward_raw", "backward_raw"):
        assert hasattr(_pigs_host, name)
    means = torch.zeros(4, 2); values = torch.ones(4, 1); con = torch.ones(4, 3); pts = torch.zeros(8, 2)
    for host in ("native", "ctypes"):
        s = GaussianSampler(True, host=host)
        assert isinstance(s._core, _pigs_host.SamplerCore) == (host == "native")
        with pytest.raises(RuntimeError, match="preprocess"):
            s.sample_gaussians()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.preprocess(means, values, con, con, pts)
        with pytest.raises(NotImplementedError):
            s.preprocess(torch.zeros(4, 3), values, con, con, pts)
        with pytest.raises(ValueError):
            s.preprocess(torch.zeros(4), values, con, con, pts)
        with pytest.raises(TypeError):
            s.preprocess(means, values, con, con, [0.0, 1.0])
        assert s._inputs is None and s._plan is None
    with pytest.raises(ValueError):
        GaussianSampler(True, host="jit")


def test_the_two_cores_have_one_interface(hip_lib):
    """What GaussianSampler drives is written down twice, in the pybind class at the end of pigs_host.cpp and in
    host_ctypes.SamplerCore: the same constructor, the same public names, and the Python methods take every argument
    the native ones take, under the native keyword names where pybind declares any."""
    import inspect
    import re
    import torch  # noqa: F401  (the extension links against it)
    from pigs_amd import _pigs_host, host_ctypes
    args = dict(debug=False, fuse=0, backend=2, q_max=36.0, q_max_order3=44.0, q_max_backward=40.0, reuse_samples=4)
    native, python = _pigs_host.SamplerCore(**args), host_ctypes.SamplerCore(**args)
    names = {n for n in dir(native) if not n.startswith("_")}
    assert names == {n for n in dir(python) if not n.startswith("_")}
    methods = {n for n in names if callable(getattr(native, n))}
    assert methods == {n for n in names if callable(getattr(python, n))}
    assert {"preprocess", "get", "sample", "inputs", "residual", "residual_terms", "residual_coupled", "vorticity_terms",
            "vorticity_residual", "preprocess_aggregate", "aggregate_neighbors", "aggregate_neighbors_heads",
            "cached_orders"} == methods
    for n in sorted(methods):
        declared = re.findall(r"[(,] ?(\w+): ", getattr(native, n).__doc__.splitlines()[0])[1:]      # without self
        params = inspect.signature(getattr(python, n)).parameters
        assert len(params) == len(declared), n
        keywords = [a for a in declared if not re.fullmatch(r"arg\d+", a)]
        assert keywords == list(params)[len(declared) - len(keywords):], n
        defaults = len(re.findall(r" = ", getattr(native, n).__doc__.splitlines()[0]))
        assert sum(p.default is not p.empty for p in params.values()) == defaults, n
    for n in sorted(names - methods):                    # the attributes start out equal, and the four settable ones are
        assert getattr(native, n) == getattr(python, n), n
    for n, v in (("defer_lists", True), ("static_samples", True), ("periodic", (0.0, 3.0)), ("periodic_aggregate", True)):
        for core in (native, python):
            setattr(core, n, v)
            assert getattr(core, n) == v


def test_host_selection_by_environment(hip_lib, monkeypatch):
    from pigs_amd.sampler import GaussianSampler
    monkeypatch.setenv("PIGS_AMD_HOST", "ctypes")
    assert GaussianSampler(False).host == "ctypes"
    monkeypatch.delenv("PIGS_AMD_HOST")
    assert GaussianSampler(False).host == "native"
