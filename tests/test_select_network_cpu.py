"""CPU checks behind the fused kernels' instruction trim: the selection network of csrc/bldpc_select.hpp through a host policy
(tests/cpp/select_network_host_test.cpp), and the oracle's value at the corner the GPU test test_qc2_valu_trim_gpu.py aims at."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from qc_trim_cases import MATRIX_SHAPES, corner_frame, path as _path


def test_selection_network_gives_the_two_smallest(tmp_path):
    """two_smallest<N> for N = 2 ... 24 equals sorted(v)[:2] (multiplicity kept): every vector over {0,1,2} for N <= 10, 4 000 draws
    from a seven-value set and 4 000 random vectors per N; the operation counts are the header's (12 for 10 values, 7 for 7)."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "sel")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "select_network_host_test.cpp")
    subprocess.check_call([gxx, "-O2", "-std=c++17", src, "-o", exe], cwd=str(tmp_path))
    out = subprocess.check_output([exe], timeout=120).decode()
    assert out.startswith("OK ") and "N=10: 12, N=7: 7" in out, out


@pytest.mark.parametrize("J,L,Z", MATRIX_SHAPES)
def test_oracle_sum_is_plus_zero_at_the_corner(orc, J, L, Z):
    """CPU side, once per matrix: where frame (b) sums -0.0f only, the oracle's sum is +0.0f -- the exact form's value, which the
    short form would not give.  max_iter 2 emits the sum after iteration 1's messages, max_iter 3 the one after iteration 2's."""
    y, corner = corner_frame(J, L, Z)
    ocode = orc.BinaryCode(_path(J, L, Z), J, L, Z)
    for its in (2, 3):
        app = orc.bldpc_decode(ocode, y, 1, its, early_exit=0, want_app=True)["app"].view(np.uint32).reshape(L, Z)
        assert (app[corner] == 0).all()  # +0.0f, not 0x80000000
