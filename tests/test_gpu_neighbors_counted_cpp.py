"""GPU: the C++ owners of the weighted sparse all-pairs comparison (bio_amd/csrc/sketches.hpp: DeviceSets::neighbors_counted,
SearchHits::weights_device / fetch_weights) against a per-pair walk with counts, and one object through the re-use chain
(tests/cpp/test_neighbors_counted.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_neighbors_counted_against_a_walk_with_counts():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_neighbors_counted"])
    out = subprocess.run([os.path.join(csrc, "test_neighbors_counted")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ neighbors_counted checks passed" in out.stdout, out.stdout + out.stderr
