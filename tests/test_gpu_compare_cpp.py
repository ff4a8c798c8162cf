"""GPU: the C++ owners of the MinHash entries (bio_amd/csrc/sketches.hpp: DeviceSets::bottom, SetsCompare) against a std::set_union walk
(tests/cpp/test_compare.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_compare_against_a_set_union_walk():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_compare"])
    out = subprocess.run([os.path.join(csrc, "test_compare")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ compare checks passed" in out.stdout, out.stdout + out.stderr
