"""GPU: the C++ owners of the sparse all-pairs comparison (bio_amd/csrc/sketches.hpp: DeviceSets::neighbors, SearchHits::totals_device /
fetch_totals) against a std::set_union walk and the rule (tests/cpp/test_neighbors.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_neighbors_against_a_set_union_walk():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_neighbors"])
    out = subprocess.run([os.path.join(csrc, "test_neighbors")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ neighbors checks passed" in out.stdout, out.stdout + out.stderr
