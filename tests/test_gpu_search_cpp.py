"""GPU: the C++ owners of the containment search (bio_amd/csrc/sketches.hpp) against a std::unordered_map count (tests/cpp/test_search.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_search_against_unordered_map():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_search"])
    out = subprocess.run([os.path.join(csrc, "test_search")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ search checks passed" in out.stdout, out.stdout + out.stderr
