"""The small stand-alone programs that put the library's host-side choice functions in front of the tests
(tests/build_choice_main.cpp, tests/launch_choice_main.cpp): compile one with hipcc as host code only, once per process,
and ask it lines.  Plain functions, no fixture: a GPU test that needs a launch variant's name or a list slab's size asks
from inside its body.

``ask`` is the protocol; the functions below it word single questions to launch_choice_main and name the answers'
fields.  They hold no rule of their own."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "float64")          # enum pigs_dtype
_built = {}


def program(name):
    """Path of tests/<name>.cpp compiled (host code only; once per process)."""
    if name not in _built:
        hipcc = os.environ.get("HIPCC", "hipcc")      # as pigs_amd/build.py
        tmp = tempfile.mkdtemp(prefix=name + "_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        exe = os.path.join(tmp, name)
        subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-Wall", "-o", exe,
                        os.path.join(ROOT, "tests", name + ".cpp")], check=True)
        _built[name] = exe
    return _built[name]


def ask(name, lines):
    """One answer line per question line."""
    lines = list(lines)
    out = subprocess.run([program(name)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


# ---- launch_choice_main
Dense = namedtuple("Dense", "forward grid block accumulators can_rows can_w16 rows_chunk backward zeroed gx gy slice")
Aggregate = namedtuple("Aggregate", "regions lds waves grids splits zero_grid outer_grid components_ok admitted lds_bytes "
                                    "heads_lds_bytes scratch_bytes")
KERNELS = ("forward", "rows", "cols")


def _number(s):
    return int(s) if s.lstrip("-").isdigit() else s


_dense, _aggregate = {}, {}


def dense_many(keys):
    """[Dense] for keys (dtype, d, c, mask, N, M): one run of the program for those not asked before"""
    new = [k for k in dict.fromkeys(keys) if k not in _dense]
    lines = ["D %d %d %d %d %d %d" % ((DTYPES.index(k[0]),) + tuple(k[1:])) for k in new]
    for k, line in zip(new, ask("launch_choice_main", lines) if new else ()):
        _dense[k] = Dense(*map(_number, line.split()))
    return [_dense[k] for k in keys]


def dense(dtype, d, c, mask, N, M):
    return dense_many([(dtype, d, c, mask, N, M)])[0]


def aggregate_many(keys):
    """[Aggregate] for keys (dtype, H, N, L, K, F); regions, lds, waves and grids are {kernel: value}"""
    new = [k for k in dict.fromkeys(keys) if k not in _aggregate]
    lines = ["A %d %d %d %d %d %d" % ((DTYPES.index(k[0]),) + tuple(k[1:])) for k in new]
    for k, line in zip(new, ask("launch_choice_main", lines) if new else ()):
        v = list(map(int, line.split()))
        four = [dict(zip(KERNELS, v[3 * i:3 * i + 3])) for i in range(4)]
        _aggregate[k] = Aggregate(*four, v[12], v[13], v[14], bool(v[15]), bool(v[16]), v[17], v[18], v[19])
    return [_aggregate[k] for k in keys]


def aggregate(dtype, H, N, L, K, F):
    return aggregate_many([(dtype, H, N, L, K, F)])[0]


@functools.lru_cache(maxsize=None)
def heads_waves(N, lds):
    """heads_waves_per_gaussian of a kernel that asks for ``lds`` bytes"""
    return int(ask("launch_choice_main", [f"W {N} {lds}"])[0])


@functools.lru_cache(maxsize=None)
def covering(mask):
    """covering_mask_of (instances.h): the compiled mask that serves a request (0: none)."""
    return int(ask("launch_choice_main", [f"V {mask}"])[0])


@functools.lru_cache(maxsize=None)
def instances(*which):
    """The compiled masks of ("dense", d, c), ("binned", c) or ("fused", c), in the order of instances.h's lists."""
    return tuple(map(int, ask("launch_choice_main", ["I " + " ".join(map(str, which))])[0].split()))


@functools.lru_cache(maxsize=None)
def list_build(N):
    """"all-pairs" or "grid": the aggregation's list build at N Gaussians"""
    return ask("launch_choice_main", [f"B {N}"])[0]


@functools.lru_cache(maxsize=None)
def plan_sizes(N):
    """(list_cap_for(N), the finest grid G0 of make_plan_layout)"""
    return tuple(map(int, ask("launch_choice_main", [f"P {N}"])[0].split()))


@functools.lru_cache(maxsize=None)
def constants():
    return {k: float(v) if "." in v else int(v) for k, v in (kv.split("=") for kv in ask("launch_choice_main", ["K"])[0].split())}
