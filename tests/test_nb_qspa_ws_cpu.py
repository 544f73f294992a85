"""The workspace tier of the FHT sum-product decoders without a GPU: the plan (nbldpc_qspa_ws_plan_host) against the numbers the
layout of include/nbldpc.h gives for the shipped matrices and the restatement of tests/nb_qspa_ws_cases.py, its refusal, the layered
rule, monotony in N; that the two shipped matrices are acceptable; that the inputs tests/test_nb_qspa_ws_gpu.py decodes are worth
decoding; the keyword checks of Decoding_QSPA that need no device; and the plan header as a stand-alone program
(tests/cpp/nb_qspa_ws_plan_host_test.hip) under the address + undefined sanitizers, its digest against the library's answers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nb_qspa_cases as Q
import nb_qspa_layered_cases as LQ
import nb_qspa_ws_cases as W


@pytest.fixture(scope="module")
def nb():
    from cuda_ldpc_amd import nbldpc
    return nbldpc


def refused(nb, *args, **kw):
    from cuda_ldpc_amd._lib import LdpcError
    with pytest.raises(LdpcError, match=r"\(-5\).*workspace tier"):
        nb.QSPA_WS_Plan_host(*args, **kw)
    return True


def test_plan_of_the_shipped_matrices(nb):
    """The table of the layout: fixed part 4 (N + 4) + q^2, 4 dc q bytes per row slab, max(64 / q, 1) slabs per wave."""
    t = W.shipped_matrix(nb, W.TANNER)
    assert (t.N, t.M, t.q, t.dc) == (9472, 1152, 16, 21)
    assert W.ws_lds_bytes(t.N, 16, t.dc, 0) == 38160 and W.ws_lds_bytes(t.N, 16, t.dc, 64) - 38160 == 5376
    assert nb.QSPA_WS_Plan_host(t.N, t.M, 16, t.dc) == dict(threads=1024, lds_bytes=124176, slot_bytes=2154496, vectors=64)
    g = W.shipped_matrix(nb, W.N576)
    assert (g.N, g.M, g.q, g.dc) == (72, 12, 256, 12)
    assert W.ws_lds_bytes(g.N, 256, g.dc, 0) == 65840 and W.ws_lds_bytes(g.N, 256, g.dc, 64) - 65840 == 12288
    assert W.ws_lds_bytes(g.N, 256, g.dc, 512) == 164144 > W.LDS_LIMIT
    assert nb.QSPA_WS_Plan_host(g.N, g.M, 256, g.dc) == dict(threads=256, lds_bytes=114992, slot_bytes=221184, vectors=4)
    N, M, q, _, dc = W.dims("lds_over", False)
    assert (N, M, q, dc) == (206, 103, 64, 4) and Q.lds_bytes(N, M, q, dc) > Q.LDS_LIMIT
    p = nb.QSPA_WS_Plan_host(N, M, q, dc)
    assert (p["threads"], p["lds_bytes"]) == (1024, 21320)
    N, M, q, _, dc = W.dims("q256_dc12", False)
    assert (N, M) == (48, 8) and nb.QSPA_WS_Plan_host(N, M, q, dc)["vectors"] == 4 < M, "two row passes"


def test_plan_refuses_q256_dc96_whatever_n(nb):
    for N in (1, 2, 72, 10000):
        assert refused(nb, N, max(N // 8, 1), 256, 96)
        assert W.plan(N, max(N // 8, 1), 256, 96) is None
    assert nb.QSPA_WS_Plan_host(72, 9, 256, 94)["threads"] == 64, "one wave's slab of 94 vectors fits beside the table"
    assert refused(nb, 72, 9, 256, 95)
    assert refused(nb, 1 << 20, 1 << 19, 256, 4), "a slot of 2 GiB or more"
    from cuda_ldpc_amd._lib import LdpcError
    for bad_q in (2, 48, 512):
        with pytest.raises(LdpcError, match=r"\(-5\).*power of two"):
            nb.QSPA_WS_Plan_host(8, 4, bad_q, 4)


@pytest.mark.parametrize("layered", [False, True])
def test_plan_equals_its_restatement(nb, layered):
    for q in (4, 16, 64, 128, 256):
        for N in (1, 24, 206, 9472, 30000):
            for dc in (2, 4, 12, 21, 64):
                for wide in ((1, 3, 4, 17, 64, 200) if layered else (0,)):
                    want = W.plan(N, N // 2 + 1, q, dc, wide, layered)
                    if want is None:
                        assert refused(nb, N, N // 2 + 1, q, dc, wide, layered)
                    else:
                        assert nb.QSPA_WS_Plan_host(N, N // 2 + 1, q, dc, wide, layered) == want, (q, N, dc, wide)


def test_layered_takes_the_smallest_size_that_holds_the_widest_level(nb):
    for cid in ("wide_q16", "mix_q16", "q64_tail"):
        N, M, q, _, dc = W.dims(cid, True)
        wide = W.widest_level(cid)
        p = nb.QSPA_WS_Plan_host(N, M, q, dc, wide, True)
        flood = nb.QSPA_WS_Plan_host(N, M, q, dc)
        holds = [t for t in W.SIZES if W.vectors(t, q) >= wide and W.ws_lds_bytes(N, q, dc, t) <= W.LDS_LIMIT]
        assert p["threads"] == (min(holds) if holds else flood["threads"]), cid
        assert p["slot_bytes"] == flood["slot_bytes"]
    assert W.widest_level("wide_q16") == 21
    assert nb.QSPA_WS_Plan_host(84, 42, 16, 4, 21, True)["threads"] == 512, "21 rows: 6 waves of 4 vectors, the next size up"
    assert nb.QSPA_WS_Plan_host(84, 42, 64, 4, 21, True)["threads"] == 1024, "no size holds 21 rows of GF(64): the largest"
    # Tanner's level table: 9 levels of 128 rows; 1024 threads hold 64: no size holds a level, the largest that fits
    t = W.shipped_matrix(nb, W.TANNER)
    widths = W.matrix_levels(t)
    assert widths == [128] * 9
    assert nb.QSPA_WS_Plan_host(t.N, t.M, 16, t.dc, max(widths), True)["threads"] == 1024
    g = W.shipped_matrix(nb, W.N576)
    assert W.matrix_levels(g) == [3, 3, 3, 3]
    assert nb.QSPA_WS_Plan_host(g.N, g.M, 256, g.dc, 3, True)["threads"] == 256, "4 vectors hold 3 rows, 128 threads would hold 2"


def test_plan_is_monotone_in_n(nb):
    """More variables: never more threads, never less LDS at one size, never a smaller slot; a refusal stays one."""
    from cuda_ldpc_amd._lib import LdpcError
    for q, dc in ((16, 21), (64, 4), (256, 12), (256, 64)):
        last = None
        for N in (1, 10, 100, 1000, 5000, 10000, 20000, 30000, 40000, 41000):
            try:
                p = nb.QSPA_WS_Plan_host(N, N // 2 + 1, q, dc)
            except LdpcError:
                p = None
            if last is not None and N > 1:
                assert p is None or (last != "refused" and p["threads"] <= last["threads"] and p["slot_bytes"] > last["slot_bytes"]), (q, dc, N)
            last = "refused" if p is None else p
    assert nb.QSPA_WS_Plan_host(30000, 100, 64, 4)["threads"] == 1024 and nb.QSPA_WS_Plan_host(38000, 100, 64, 4)["threads"] < 1024


@pytest.mark.parametrize("sid", sorted(W.SHIPPED))
def test_shipped_matrices_are_acceptable(nb, sid):
    """With NBMatrix alone: no zero coefficient, no row that lists a variable twice, the LDS tier's bound missed, the plan met."""
    s = W.SHIPPED[sid]
    m = W.shipped_matrix(nb, s)
    used = np.arange(m.dc)[None, :] < m.cn_weight[:, None]
    assert not (m.cn_linkVNs_GF[used] == 0).any()
    assert all(len(set(m.cn_linkVNs[r, :m.cn_weight[r]].tolist())) == m.cn_weight[r] for r in range(m.M))
    assert m.dv <= 8 and Q.lds_bytes(m.N, m.M, m.q, m.dc) > Q.LDS_LIMIT
    assert nb.QSPA_WS_Plan_host(m.N, m.M, m.q, m.dc)["lds_bytes"] <= W.LDS_LIMIT


@pytest.mark.parametrize("layered", [False, True])
def test_shipped_inputs_are_worth_decoding(nb, layered):
    w = W.shipped_want(nb, W.N576, layered)
    assert w["iter_number"].shape == (8,) and len(set(w["iter_number"].tolist())) >= 2, w["iter_number"].tolist()
    assert ((w["ok"] == 1) & (w["iter_number"] < W.N576.maxIT)).any(), "a frame that stops early"
    assert np.isfinite(w["LLR"]).all() and np.isfinite(w["L_c2v"]).all()
    w = W.shipped_want(nb, W.TANNER, layered)
    assert w["iter_number"].shape == (2,) and (w["iter_number"] > 1).all(), w["iter_number"].tolist()
    assert np.isfinite(w["LLR"]).all() and np.isfinite(w["L_c2v"]).all()


@pytest.mark.parametrize("cid", ["lds_over", "q256_dc12"])
@pytest.mark.parametrize("layered", [False, True])
def test_new_case_inputs_are_worth_decoding(nb, cid, layered):
    """As the two tables ask of their cases: three or more different iteration counts, a failing frame, no NaN."""
    mod, case = W.mod_of(layered), W.case_of(cid, layered)
    w = mod.want(nb, case)
    assert len(set(w["iter_number"].tolist())) >= 3 and (w["ok"] == 0).any() and (w["ok"] == 1).any(), (w["iter_number"].tolist(), w["ok"].tolist())
    assert np.isfinite(w["LLR"]).all() and np.isfinite(w["L_c2v"]).all()
    assert mod.inputs(nb, case).shape[0] == 12


def test_slot_reuse_frames_stop_at_different_iterations(nb):
    for layered in (False, True):
        w = W.mod_of(layered).want(nb, W.case_of("q16_part", layered))
        assert len(set(w["iter_number"].tolist())) >= 3


def test_tier_keyword_is_checked_before_the_device(nb):
    with pytest.raises(ValueError, match="tier"):
        nb.Decoding_QSPA(None, None, tier="hbm")
    assert nb.QSPA_TIERS == ("lds", "workspace", "auto") and nb.QSPA_LDS_LIMIT == Q.LDS_LIMIT
    assert nb.qspa_lds_bytes(206, 103, 64, 4) == Q.lds_bytes(206, 103, 64, 4)
    import inspect
    from cuda_ldpc_amd import nb_simulation as S
    for fn in (S.Simulation_GPU, S.Simulation_HARQ_GPU, S.sweep, S.sweep_harq, S._decode):
        assert inspect.signature(fn).parameters["qspa_tier"].default == "lds", fn.__name__
    assert inspect.signature(nb.Decoding_QSPA).parameters["tier"].default == "lds"


def fnv64(a):
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_plan_stand_alone_under_sanitizers(nb, tmp_path):
    """The sweep of tests/cpp/nb_qspa_ws_plan_host_test.hip over q, N, M, dc and the widest level, through the library."""
    from cuda_ldpc_amd._lib import LdpcError
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "nb_qspa_ws_plan_host_test")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "nb_qspa_ws_plan_host_test.hip"), "-o", exe],
                          cwd=str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    wides = (0, 1, 3, 4, 5, 16, 17, 64, 65, 1000)
    answers = []
    for q in (4, 8, 16, 32, 64, 128, 256):
        for N in (1, 7, 72, 206, 1000, 9472, 24000, 40000):
            for dc in (2, 3, 4, 12, 21, 40, 64, 96):
                for M in (1, N // 2 + 1):
                    for k in range(11):
                        try:
                            p = nb.QSPA_WS_Plan_host(N, M, q, dc, wides[k - 1] if k else 0, k > 0)
                            answers += [p["threads"], p["lds_bytes"], p["slot_bytes"], p["vectors"]]
                        except LdpcError:
                            answers += [0, 0, 0, 0]
    lines = out.stdout.split()
    assert lines[0] == str(len(answers) // 4) and lines[-1] == fnv64(np.array(answers, np.int32)), out.stdout
