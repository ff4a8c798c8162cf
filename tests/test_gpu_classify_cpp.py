"""GPU: the C++ owners of the classification route (bio_amd/csrc/sketches.hpp: SearchIndex::attach, SearchHits::top, classify_memory)
against a std::unordered_map count over sets made on the host (tests/cpp/test_classify.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_classify_against_unordered_map():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_classify"])
    out = subprocess.run([os.path.join(csrc, "test_classify")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ classify checks passed" in out.stdout, out.stdout + out.stderr
