"""The fused kernels' check-node selection network (csrc/bldpc_select.hpp) and the variable-node sum that starts at R_0 inside
the fixed-iteration loop of k_qc2 (csrc/bldpc_qc2_body.inc), against the CPU oracle, bit for bit: hard bits, flag row and the
a-posteriori sums as uint32.

Network sizes reached: J4_L24_Z96 half-rows of 10, J8_L24_Z96 5, J6_L24_Z96 8, J12_L24_Z96 4, J32_L64_Z64 (k_qc) rows of 5 / 6 / 7.
Sum forms: max_iter 1 and 2 run no loop iteration (first phase, final phase: both exact), 3 runs one and 7 five (started at R_0
in the fixed exit, at 0 in the flag-tracking instantiations).

Inputs.  (a) Channel values drawn with a fixed seed from {-0, +0, +-0.5, +-1, +-1.5, +-2}: every sum is exact, ties and exact zeros
are common.  (b) The CORNER frame: y = -0.0f everywhere except a set C of block columns with an odd number of blocks in every block
row (J4_L24_Z96: one column with a block in every row; the other matrices have no such column and take a solution of B x = 1 over
GF(2)), where y = -1.0f.  The first sum is (+0) + y, so Q is +0.0f outside C and -1 in C: every check row has an odd number of
negatives and at least two zero magnitudes, so every R into a variable outside C is -0.0f after iteration 1 and stays so.  From
iteration 2 on, every variable outside C whose column has no padded slot (column weight = the heaviest) sums -0.0f only: the
reference's ((0 + R_0) + ...) + y is +0.0f there, the sum started at R_0 is -0.0f.  Inside the loop nobody reads that sign
(max_iter 3 and 7 go through it and emit +0.0f from the final, exact, phase); the flag-tracking kernels emit from inside the loop
and keep the exact form.  In the F = 3 batch the corner frame is frame 1 (frame pair 0, second lane), frame 2 is alone in the
second workgroup; with F = 1 it is frame 0."""
import numpy as np
import pytest
import torch

from qc_trim_cases import batches, path as _path

pytestmark = pytest.mark.gpu

ITERS = (1, 2, 3, 7)
# (J, L, Z, what the kernel's name starts with): the half-row kernel with local edges, half-row kernels, the row kernel
MATRICES = [(4, 24, 96, "qc_lds_halfrow-local<"), (8, 24, 96, "qc_lds_halfrow"), (6, 24, 96, "qc_lds_halfrow"), (12, 24, 96, "qc_lds_halfrow"),
            (32, 64, 64, "qc_lds_row")]


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    assert torch.cuda.is_available()
    return cuda_ldpc_amd


def _decode(C, code, y, **kw):
    r = C.LDPC_Decoder_GPU(code, torch.from_numpy(np.ascontiguousarray(y)).cuda(), **kw)
    torch.cuda.synchronize()
    return r


def _assert_same(r, want, N, F, what):
    D = r["D"].cpu().numpy().reshape(-1)
    assert r["iteraTime"] == want["it"], what
    assert np.array_equal(D[: N * F], want["D"][: N * F]), "hard bits differ: " + what
    assert np.array_equal(D[N * F:], want["D"][N * F:]), "flag row differs: " + what
    assert np.array_equal(r["app"].cpu().numpy().reshape(-1).view(np.uint32), want["app"].view(np.uint32)), "a-posteriori sums differ bitwise: " + what


def _fixed_exit_cases(C, orc, code, ocode, J, L, Z, tag):
    N = L * Z
    for name, (y, _) in batches(J, L, Z).items():
        F = y.shape[1]
        for its in ITERS:
            want = orc.bldpc_decode(ocode, np.ascontiguousarray(y).reshape(-1), F, its, early_exit=0, want_app=True)
            r = _decode(C, code, y, max_iter=its, exit_mode=C.EXIT_FIXED, want_app=True)
            k = code.last_kernel
            assert k.startswith(tag), k
            _assert_same(r, want, N, F, "%s max_iter %d %s" % (name, its, k))


@pytest.mark.parametrize("J,L,Z,tag", MATRICES)
def test_fixed_exit_bit_exact(C, orc, J, L, Z, tag):
    code = C.BinaryCode.from_blockh(_path(J, L, Z), J, L, Z)
    _fixed_exit_cases(C, orc, code, orc.BinaryCode(_path(J, L, Z), J, L, Z), J, L, Z, tag)


def test_fixed_exit_bit_exact_plain_form(C, orc, monkeypatch):
    """J4_L24_Z96 without local edges (vn_phase instead of vn_phase_loc)."""
    J, L, Z = 4, 24, 96
    monkeypatch.setenv("BLDPC_NO_LOCAL", "1")
    code = C.BinaryCode.from_blockh(_path(J, L, Z), J, L, Z)
    monkeypatch.delenv("BLDPC_NO_LOCAL")
    _fixed_exit_cases(C, orc, code, orc.BinaryCode(_path(J, L, Z), J, L, Z), J, L, Z, "qc_lds_halfrow<")


def test_flag_tracking_exits_keep_the_exact_sum(C, orc):
    """J4_L24_Z96, the F = 3 batch, batch-global and per-frame exit: these kernels emit S from inside the loop, so a sum started at
    R_0 there would show as -0.0f in the corner frame's sums (the frame never satisfies its checks: it runs to max_iter)."""
    J, L, Z, its = 4, 24, 96, 7
    N = L * Z
    y, corner_frame = batches(J, L, Z)["F3"]
    F = y.shape[1]
    ocode = orc.BinaryCode(_path(J, L, Z), J, L, Z)
    code = C.BinaryCode.from_blockh(_path(J, L, Z), J, L, Z)
    want = orc.bldpc_decode(ocode, np.ascontiguousarray(y).reshape(-1), F, its, early_exit=1, want_app=True)
    r = _decode(C, code, y, max_iter=its, exit_mode=C.EXIT_BATCH_GLOBAL, want_app=True)
    assert "halfrow-local" in code.last_kernel, code.last_kernel
    _assert_same(r, want, N, F, "batch-global")
    r = _decode(C, code, y, max_iter=its, exit_mode=C.EXIT_PER_FRAME, want_app=True)
    assert "halfrow-local" in code.last_kernel, code.last_kernel
    D, app, iters = r["D"].cpu().numpy(), r["app"].cpu().numpy(), r["iters"].cpu().numpy()
    for f in range(F):  # the reference's rule on every frame alone
        w = orc.bldpc_decode(ocode, np.ascontiguousarray(y[:, f]), 1, its, early_exit=1, want_app=True)
        assert iters[f] == w["it"] and np.array_equal(D[:, f], w["D"]), "per-frame exit, frame %d" % f
        assert np.array_equal(app[:, f].view(np.uint32), w["app"].view(np.uint32)), "per-frame exit, sums of frame %d" % f
    assert iters[corner_frame] == its
