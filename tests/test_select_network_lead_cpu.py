"""CPU check of the selection network's entry behind its first triple (csrc/bldpc_select.hpp, two_smallest_lead), which the half-row
kernel uses for its local edges: tests/cpp/select_network_lead_host_test.cpp through a host policy."""
import os
import shutil
import subprocess

import pytest


def test_lead_entry_gives_the_two_smallest(tmp_path):
    """two_smallest_lead<N> for N = 4 ... 24 equals sorted(v)[:2] (multiplicity kept) and the bits of two_smallest<N>: every vector over
    {0,1,2} for N <= 10, draws from a seven-value set, random vectors, and the two smallest (equal or not) placed in every pair of
    places; it spends the whole network's operations less the first triple's two."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "sel_lead")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "select_network_lead_host_test.cpp")
    subprocess.check_call([gxx, "-O2", "-std=c++17", src, "-o", exe], cwd=str(tmp_path))
    out = subprocess.check_output([exe], timeout=120).decode()
    assert out.startswith("OK ") and "N=10: 10, N=8: 7" in out, out
