"""GPU: the C++ owners of the counted sets (bio_amd/csrc/sketches.hpp: DeviceSets::from_result_counted / ::op_counted / ::filter_counts /
::totals) against std::map counting (tests/cpp/test_counts.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_counted_sets_against_a_map_count():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_counts"])
    out = subprocess.run([os.path.join(csrc, "test_counts")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ counted-set checks passed" in out.stdout, out.stdout + out.stderr
