"""GPU: the C++ owners of the weighted containment search (bio_amd/csrc/sketches.hpp: SearchIndex::build_counted / counted / fetch_norms /
search_counted) against a std::map walk over every pair, the four combinations of counted and uncounted operands, a query on the large
path, and one object through the re-use chain (tests/cpp/test_search_counted.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_search_counted_against_a_map_walk():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_search_counted"])
    out = subprocess.run([os.path.join(csrc, "test_search_counted")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ search_counted checks passed" in out.stdout, out.stdout + out.stderr
