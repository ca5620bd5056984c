"""CPU: the list build's ellipse / rectangle arithmetic (pigs_amd/csrc/ellipse_rect.h) through a small stand-alone
program (tests/ellipse_rect_main.cpp, host code only): "axis terms, then combine" against a float64 minimum of q over
the rectangle that shares no formula with it, on 10^5 seeded ellipses, each against the 16 boxes of a 4 x 4 product of
intervals; and the two orders of evaluation -- shared axis terms (the product path of plan_lists.h) and
ellipse_min_q_rect box by box (the general path) -- against each other, bit for bit.

The bar.  q = a x^2 + 2 b x y + c y^2 at the minimising point of an edge: three terms of size up to q / (1 - rho^2)
each (they cancel to q for a correlation rho), formed by at most 8 float32 roundings (the two differences, the median's
inputs, p e, (p e) e, 2b e, nb e and the two FMAs) of 2^-24 relative each:  |q32 - q64| <= 8 * 2^-24 / (1 - rho^2) * q.
For |rho| <= 0.98 that is 1.2e-5, within the band DELTA = 2e-5 that the list tests leave open (oracle/plan_lists.py);
for |rho| = 0.9999, 2.4e-3.  Measured: 4.1e-6 and 1.3e-3."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELLIPSES = 100000


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")      # as pigs_amd/build.py's host extension
    exe = str(tmp_path_factory.mktemp("ellipse_rect") / "ellipse_rect_main")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "ellipse_rect_main.cpp")], check=True)
    out = subprocess.run([exe, str(ELLIPSES), "1"], capture_output=True, text=True, check=True).stdout.split()
    return dict(ellipses=int(out[0]), compared=int(out[1]), worst=float(out[2]), compared_extreme=int(out[3]),
                worst_extreme=float(out[4]), identical=int(out[5]))


def test_terms_then_combine_is_the_minimum_over_the_rectangle(result):
    print(result)
    assert result["ellipses"] == ELLIPSES and result["compared"] >= ELLIPSES and result["compared_extreme"] >= ELLIPSES // 10
    assert result["worst"] <= 8 * 2.0 ** -24 / (1 - 0.98 ** 2)
    assert result["worst_extreme"] <= 8 * 2.0 ** -24 / (1 - 0.9999 ** 2)


def test_shared_terms_and_box_by_box_agree_bit_for_bit(result):
    assert result["identical"] == ELLIPSES
