"""GPU: the C++ owner of the merged hits (bio_amd/csrc/sketches.hpp: SearchHits::merge) against a std::map model
(tests/cpp/test_merge.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_merge_against_the_map_model():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_merge"])
    out = subprocess.run([os.path.join(csrc, "test_merge")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ merge checks passed" in out.stdout, out.stdout + out.stderr
