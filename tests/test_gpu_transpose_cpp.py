"""GPU: the C++ owners of the hits by target (bio_amd/csrc/sketches.hpp: SearchHits::transpose, SearchHits::tally, Tally) against a
std::stable_sort model and three counting loops (tests/cpp/test_transpose.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_transpose_against_the_sort_model():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_transpose"])
    out = subprocess.run([os.path.join(csrc, "test_transpose")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ transpose checks passed" in out.stdout, out.stdout + out.stderr
