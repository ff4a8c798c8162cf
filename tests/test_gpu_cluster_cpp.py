"""GPU: the C++ owners of the clusters of a hits graph (bio_amd/csrc/sketches.hpp: SearchHits::from_host / cluster, Clusters) against a
union-find and the sequential greedy rule (tests/cpp/test_cluster.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_cluster_against_union_find_and_the_sequential_rule():
    csrc = os.path.join(ROOT, "bio_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "test_cluster"])
    out = subprocess.run([os.path.join(csrc, "test_cluster")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all C++ cluster checks passed" in out.stdout, out.stdout + out.stderr
