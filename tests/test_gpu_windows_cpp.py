"""GPU: the C++ owners of the window sets and the folded hits (bio_amd/csrc/sketches.hpp: DeviceSets::from_windows, SearchHits::fold /
fetch_members) against a std::map model built by the definition (tests/cpp/test_windows.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_windows_and_fold_against_a_map_model():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_windows"])
    out = subprocess.run([os.path.join(csrc, "test_windows")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ window checks passed" in out.stdout, out.stdout + out.stderr
