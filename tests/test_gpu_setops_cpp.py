"""GPU: the C++ owners of the set algebra (bio_amd/csrc/sketches.hpp: DeviceSets::op / ::reduce) against std::set_union and its kin
(tests/cpp/test_setops.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_setops_against_the_standard_algorithms():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_setops"])
    out = subprocess.run([os.path.join(csrc, "test_setops")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ set-operation checks passed" in out.stdout, out.stdout + out.stderr
