"""GPU tests of the half-row kernel's prologue and first iteration: the per-thread address tables built by the host
(QcPlan::d_lane) and the first iteration that reads no R (every R is +0 at the start).

The fused kernel (kernel=qc) is compared bitwise -- hard bits, flag row, a-posteriori sums as uint32 -- with the table
kernels (kernel=table) and, where the batch is small, with the CPU oracle: at 1, 2 and 50 iterations, at batch sizes that
are not a multiple of the persistent grid, on a channel that holds -0.0f and +0.0f, on the local-edge and the plain
half-row forms, and in the per-frame exit with and without persistent workgroups.
"""
import os

import numpy as np
import pytest
import torch

from conftest import DATA

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def _path(J, L, Z):
    return os.path.join(BL, "J%d_L%d_Z%d_BlockH.txt" % (J, L, Z))


def _code(C, monkeypatch, J, L, Z, env=()):
    """A code whose plan is built with the given switches set (they are read once, when the plan is built)."""
    with monkeypatch.context() as m:
        for k in env:
            m.setenv(k, "1")
        code = C.BinaryCode.from_blockh(_path(J, L, Z), J, L, Z)
    return code


def _channel(orc, N, F, snr, zeros=False):
    y = orc.bldpc_awgn(np.array([173, 173, 173], np.int32), orc.bldpc_sigma(snr), N, F).reshape(N, F).copy()
    if zeros:  # signed zeros: the first sum is y + 0.0f, which turns -0.0f into +0.0f
        y[::7, :] = -0.0
        y[3::11, :] = 0.0
    return y


def _run(C, code, y, iters, kern, mode=None):
    yt = y if torch.is_tensor(y) else torch.from_numpy(np.ascontiguousarray(y)).cuda()
    mode = C.EXIT_FIXED if mode is None else mode
    r = C.LDPC_Decoder_GPU(code, yt, max_iter=iters, exit_mode=mode, kernel=kern, want_app=True)
    torch.cuda.synchronize()
    out = dict(D=r["D"].cpu().numpy(), app=r["app"].cpu().numpy().view(np.uint32), kernel=code.last_kernel)
    if mode == C.EXIT_PER_FRAME:
        out["iters"] = r["iters"].cpu().numpy()
    return out


def _same(a, b):
    assert np.array_equal(a["D"], b["D"]), "hard bits or flags differ (%s / %s)" % (a["kernel"], b["kernel"])
    assert np.array_equal(a["app"], b["app"]), "a-posteriori sums differ bitwise (%s / %s)" % (a["kernel"], b["kernel"])
    if "iters" in a:
        assert np.array_equal(a["iters"], b["iters"]), "per-frame iteration counts differ"


# (J, L, Z, Es/N0, switches, the half-row form the plan must pick)
FORMS = [(4, 24, 96, 3.0, (), "halfrow-local"), (4, 24, 96, 3.0, ("BLDPC_NO_LOCAL",), "halfrow<"), (8, 24, 96, 1.0, (), "halfrow<")]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "J%d_L%d_Z%d%s" % (f[0], f[1], f[2], "_plain" if f[4] else ""))
@pytest.mark.parametrize("iters", [1, 2, 50])
@pytest.mark.parametrize("F", [1, 37, 64])
def test_small_batches_vs_oracle_and_table(C, orc, monkeypatch, form, iters, F):
    J, L, Z, snr, env, tag = form
    code = _code(C, monkeypatch, J, L, Z, env)
    y = _channel(orc, L * Z, F, snr, zeros=True)
    got = _run(C, code, y, iters, C.KERNEL_QC_LDS)
    assert tag in got["kernel"], got["kernel"]
    _same(got, _run(C, code, y, iters, C.KERNEL_TABLE))
    want = orc.bldpc_decode(orc.BinaryCode(_path(J, L, Z), J, L, Z), y.reshape(-1), F, iters, early_exit=0, want_app=True)
    assert np.array_equal(got["D"].reshape(-1), want["D"]), "hard bits differ from the oracle"
    assert np.array_equal(got["app"].reshape(-1), want["app"].view(np.uint32)), "a-posteriori sums differ from the oracle"


@pytest.mark.parametrize("form", FORMS[:2], ids=["local", "plain"])
@pytest.mark.parametrize("iters", [1, 2, 50])
def test_large_ragged_batch_vs_table(C, orc, monkeypatch, form, iters):
    """65 536 + 6 frames: more frame pairs than any persistent grid, and not a multiple of it."""
    J, L, Z, snr, env, tag = form
    F = 65536 + 6
    code = _code(C, monkeypatch, J, L, Z, env)
    y = torch.from_numpy(_channel(orc, L * Z, 4096, snr, zeros=True)).cuda().repeat(1, F // 4096 + 1)[:, :F].contiguous()
    got = _run(C, code, y, iters, C.KERNEL_QC_LDS)
    assert tag in got["kernel"], got["kernel"]
    _same(got, _run(C, code, y, iters, C.KERNEL_TABLE))


@pytest.mark.parametrize("F", [37, 8192 + 6])
def test_per_frame_persistent_vs_dispatched_and_table(C, orc, monkeypatch, F):
    """Per-frame exit: the persistent local-edge kernel, the same kernel dispatched (BLDPC_NO_PERSIST) and the table kernels."""
    J, L, Z = 4, 24, 96
    y = _channel(orc, L * Z, F, 3.0, zeros=True)
    pers = _code(C, monkeypatch, J, L, Z, ())
    disp = _code(C, monkeypatch, J, L, Z, ("BLDPC_NO_PERSIST",))
    a = _run(C, pers, y, 50, C.KERNEL_QC_LDS, C.EXIT_PER_FRAME)
    assert "halfrow-local" in a["kernel"], a["kernel"]
    _same(a, _run(C, disp, y, 50, C.KERNEL_QC_LDS, C.EXIT_PER_FRAME))
    _same(a, _run(C, pers, y, 50, C.KERNEL_TABLE, C.EXIT_PER_FRAME))
