"""GPU: the C++ owners of the abundance-weighted entries (bio_amd/csrc/sketches.hpp: DeviceSets::compare_counted's home SetsCompare,
DeviceSets::sumsq) against a std::map walk (tests/cpp/test_compare_counted.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_compare_counted_against_a_map_walk():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_compare_counted"])
    out = subprocess.run([os.path.join(csrc, "test_compare_counted")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ weighted compare checks passed" in out.stdout, out.stdout + out.stderr
