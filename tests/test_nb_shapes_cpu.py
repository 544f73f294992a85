"""The random GF(q) codes of tests/nb_shape_cases.py without a GPU: the generated files are what the case table says (weights, both
views of the graph, the field table), nb_tables_build sends every case where the table expects it (tests/cpp/nb_plan_host_test.hip
as a stand-alone program under the host sanitizers, whose own cross-index and trellis checks thereby run on every new shape), and
the inputs are worth decoding: judged by the oracle alone, the noisy frames of every batch stop at three or more different
iterations, some late, some never.  tests/test_nb_shapes_gpu.py holds the device kernels against the oracle on the same cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nb_shape_cases as S

FUSED_LDS_LIMIT = 160 * 1024


@pytest.mark.parametrize("cid", S.IDS)
def test_generated_files_are_what_the_case_states(orc, cid):
    case = S.BY_ID[cid]
    M, edges = S.graph(case)
    oc = S.ocode(orc, case)
    assert (oc.N, oc.M, oc.q, oc.dv, oc.dc) == (case.N, M, case.q, case.dv, case.dc)
    colw, roww = oc.vn_w, oc.cn_w
    assert colw.sum() == roww.sum() == len(edges)
    if case.drop is None:  # ladder
        assert M == case.N - 1 and (roww == 2).all() and colw.tolist() == [1] + [2] * (case.N - 2) + [1]
        assert S.levels_of(M, edges) == M
    else:
        assert M == case.N * case.dv // case.dc and len(edges) == M * case.dc - case.drop
        assert sorted(set(colw.tolist())) == ([case.dv - 1, case.dv] if case.drop else [case.dv])
        assert sorted(set(roww.tolist())) == ([case.dc - 1, case.dc] if case.drop else [case.dc])
        assert (colw == case.dv - 1).sum() == case.drop and (roww == case.dc - 1).sum() == case.drop
        assert colw.min() >= 1 and roww.min() >= 2
    # the two views agree: every (row, column, coefficient) of the rows' lists is in the column's list and the other way round
    vn_cn, vn_gf = oc.vn_cn.reshape(case.N, case.dv), oc.vn_gf.reshape(case.N, case.dv)
    cn_vn, cn_gf = oc.cn_vn.reshape(M, case.dc), oc.cn_gf.reshape(M, case.dc)
    from_cols = sorted((int(vn_cn[c, d]), c, int(vn_gf[c, d])) for c in range(case.N) for d in range(colw[c]))
    from_rows = sorted((r, int(cn_vn[r, s]), int(cn_gf[r, s])) for r in range(M) for s in range(roww[r]))
    assert from_cols == from_rows == sorted(edges)
    assert len(set((r, c) for r, c, _ in edges)) == len(edges), "no parallel edges"
    assert all(0 < h < case.q for _, _, h in edges)
    # the field table: a field with XOR addition whose inverse table inverts
    mul, add, inv = S.gf_tables(case.q)
    assert np.array_equal(oc.mul.reshape(case.q, case.q), mul) and np.array_equal(oc.inv, inv)
    assert np.array_equal(mul, mul.T) and (mul[1] == np.arange(case.q)).all() and (mul[0] == 0).all()
    assert all(sorted(mul[a, 1:].tolist()) == list(range(1, case.q)) for a in range(1, case.q))
    assert all(mul[a, inv[a]] == 1 for a in range(1, case.q))
    x, y, z = 3 % case.q, case.q - 1, case.q // 2 + 1
    assert mul[x, y ^ z] == mul[x, y] ^ mul[x, z] and mul[mul[x, y], z] == mul[x, mul[y, z]]
    # deterministic in the seed, and another seed is another graph
    if case.drop is not None:
        assert S.random_graph(case.N, case.dv, case.dc, case.drop, case.q, case.seed) == (M, edges)
        assert S.random_graph(case.N, case.dv, case.dc, case.drop, case.q, case.seed + 100) != (M, edges)


def test_the_shapes_the_cases_are_there_for():
    """Every row and column weight, field and size the issue names is in the table."""
    byq = {}
    for case in S.CASES:
        M, edges = S.graph(case)
        roww = np.bincount([r for r, _, _ in edges], minlength=M)
        colw = np.bincount([c for _, c, _ in edges], minlength=case.N)
        byq.setdefault((case.q, case.kernel), []).append((case.N, set(roww.tolist()), set(colw.tolist()), case.tmm))
    fused_w = set().union(*[w for k, v in byq.items() if k[1] == "k_nb_ems" for _, w, _, _ in v])
    assert {2, 3, 4, 5, 6} <= fused_w
    for q in (16, 32, 64):
        assert any(N > 96 for N, _, _, _ in byq[(q, "k_nb_ems")]) and any(max(cw) >= 3 for _, _, cw, _ in byq[(q, "k_nb_ems")])
    assert any(max(cw) == 3 for _, _, cw, _ in byq[(128, "k_nb_ems_wide")]) and any(max(cw) == 3 for _, _, cw, _ in byq[(256, "k_nb_ems_wide")])
    hbm_w = set().union(*[w for k, v in byq.items() if k[1] == "k_nb_ems_hbm" for _, w, _, _ in v])
    assert {3, 4, 7, 8, 11, 12} <= hbm_w and (4, "k_nb_ems_hbm") in byq and (8, "k_nb_ems_hbm") in byq
    tmm_w = set().union(*[w for v in byq.values() for _, w, _, t in v if t])
    assert {2, 3, 4, 5, 6, 7, 8} <= tmm_w
    assert {2, 3, 4} <= set().union(*[cw for v in byq.values() for _, _, cw, t in v if t])


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """tests/cpp/nb_plan_host_test.hip, built as test_nb_plan_tables_equal_the_parent_commit_under_host_sanitizers builds it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("nb_plan")
    exe = str(tmp / "nb_plan_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "nb_plan_host_test.hip"), "-o", exe],
                          cwd=str(tmp))
    return exe


@pytest.mark.parametrize("cid", S.IDS)
def test_routing_is_the_tables(plan_exe, cid):
    case = S.BY_ID[cid]
    mpath, gpath = S.files(case)
    r = subprocess.run([plan_exe, cid, mpath, gpath, "0"], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    lines = r.stdout.decode().strip().split("\n")
    assert r.returncode == 0 and lines[-1] == "OK 1", r.stdout.decode()
    tok = lines[0].split()
    assert tok[0] == cid
    got = dict(zip(("m", "hbm", "lds_bytes", "zero_coeff", "levels", "tmm_ok", "pipe_lds"), (int(x) for x in tok[1:8])))
    assert 1 << got["m"] == case.q and got["zero_coeff"] == 0
    assert got["hbm"] == (case.kernel == "k_nb_ems_hbm")
    if not got["hbm"]:
        assert 0 < got["lds_bytes"] <= FUSED_LDS_LIMIT
    if cid == "tail_q64":
        assert got["lds_bytes"] == 163016  # 824 bytes below the limit
    assert got["tmm_ok"] == case.tmm
    assert got["pipe_lds"] == 0, "no case may take the two-frame pipeline: the fused tests are about k_nb_ems"
    assert got["levels"] == S.levels_of(*S.graph(case))
    if cid in ("ladder63", "ladder64"):
        assert got["levels"] == case.N - 1 and case.tmm == (got["levels"] <= 63)


@pytest.mark.parametrize("cid", S.IDS)
def test_inputs_spread_over_the_iterations(orc, cid):
    """A condition on the inputs, judged by the oracle alone."""
    case = S.BY_ID[cid]
    Lch = S.inputs(orc, case)
    B, nn = Lch.shape[0], S.n_noisy(case)
    assert B <= 16 and B == nn + 4 and Lch.shape[1:] == (case.N, case.q - 1) and Lch.dtype == np.float32
    assert np.signbit(Lch[nn][Lch[nn] == 0]).any() and (Lch[nn] != 0).any(), "-0.0 entries"
    assert np.abs(Lch[nn + 1]).max() == np.float32(3) * np.float32(1e30) and np.isfinite(Lch[nn + 1]).all()
    tiny = np.abs(Lch[nn + 2][Lch[nn + 2] != 0])
    assert tiny.size and tiny.max() < np.finfo(np.float32).tiny, "denormals"
    ints = Lch[nn + 3]
    assert np.array_equal(ints, np.round(ints)) and ints.min() == -3 and ints.max() == 3
    assert ((ints == ints.max(1, keepdims=True)).sum(1) > 1).any(), "a vector whose maximum is tied"
    if case.q > 64:  # ... in two different waves of the vector
        top = ints == ints.max(1, keepdims=True)
        assert (top[:, :64].any(1) & top[:, 64:].any(1)).any()
    ok, what = S.spread_ok(case, S.want_ems(orc, case))
    assert ok, "EMS " + what
    for layered in ((False, True) if case.tmm else ()):
        ok, what = S.spread_ok(case, S.want_tmm(orc, case, layered))
        assert ok, ("layered " if layered else "flooding ") + "trellis " + what
