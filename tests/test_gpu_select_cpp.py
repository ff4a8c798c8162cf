"""GPU: the C++ owners of the selection by a measure (bio_amd/csrc/sketches.hpp: SearchHits::filter, SearchHits::top_by) against a
std::map model in unsigned __int128 host arithmetic (tests/cpp/test_select.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_select_against_the_map_model():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_select"])
    out = subprocess.run([os.path.join(csrc, "test_select")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ select checks passed" in out.stdout, out.stdout + out.stderr
