"""bench.py's command line and --dump-outputs files (CPU: the arrays of a timed step are stood in for by
seeded random tensors of the same shapes)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def _outs(M):
    gen = torch.Generator().manual_seed(1)
    return (torch.randn((M, 1), generator=gen), torch.randn((M, 2, 1), generator=gen),
            torch.randn((M, 2, 2, 1), generator=gen))


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("u", "grad_u", "hessian_u")}


def test_dump_writes_every_output_whole_in_float32(tmp_path):
    outs = _outs(1000)
    bench.dump_outputs(outs, str(tmp_path / "d"))
    got = _load(tmp_path / "d")
    for o, x in zip(outs, got.values()):
        assert x.dtype == np.float32 and np.array_equal(x, o.numpy())


def test_dump_above_the_cap_takes_the_same_seeded_rows_of_every_output(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 28 * 100)          # 28 B per point: 100 of the 1000 points
    outs = _outs(1000)
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES
    rows = [int(np.flatnonzero(outs[0][:, 0].numpy() == v)[0]) for v in a["u"][:, 0]]
    assert len(rows) == 100 and rows == sorted(set(rows))
    for o, n in zip(outs, a):
        assert np.array_equal(a[n], b[n]) and np.array_equal(a[n], o.numpy()[rows])


def test_dump_cap_fits_the_contract():
    assert bench.DUMP_BYTES + 3 * 4096 <= 64 * 10 ** 6          # three .npy headers on top of the arrays


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_checked(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
