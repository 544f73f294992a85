"""The layered FHT sum-product decoder without a GPU: nbldpc_qspa_layered_decode_host (plain C++, the definition of the decoder inside
the product) against the fp32 numpy restatement of include/nbldpc.h ("FHT sum-product, layered schedule") written in
tests/nb_qspa_layered_cases.py, bit for bit, on every case of the table; the restatement run level by level against the one run row
by row (the claim k_nb_qspa_layered rests on); the level structure the cases are there for; a batch against its frames one at a time;
maxIT = 1; the refusals; the iteration count against the flooding statement on BDS.576.288.GF.64; the level tables of nb_tables_build
against their restatement here; and the host statement as a
stand-alone program (tests/cpp/nb_qspa_layered_host_test.hip) under the address + undefined sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import nb_qspa_cases as Q
import nb_qspa_layered_cases as LQ
from nb_shape_cases import POLY, levels_of

from conftest import DATA

f32 = np.float32


@pytest.fixture(scope="module")
def nb():
    from cuda_ldpc_amd import nbldpc
    return nbldpc


def frames_of(case, L):
    """Every frame of a small case; of the two largest codes three frames, chosen by the host statement's iteration counts."""
    return range(L.shape[0]) if LQ.graph(case)[0] <= 50 else (0, 5, 9)


@pytest.mark.parametrize("cid", LQ.IDS)
def test_host_statement_equals_numpy(nb, cid):
    case = LQ.BY_ID[cid]
    m, L, w = LQ.matrix(nb, case), LQ.inputs(nb, case), LQ.want(nb, case)
    N, M, dv, dc, edges = LQ.graph(case)
    assert (m.N, m.M, m.q, m.dv, m.dc) == (N, M, case.q, dv, dc) and Q.lds_bytes(N, M, case.q, dc) <= Q.LDS_LIMIT
    for b in frames_of(case, L):
        r = LQ.np_decode_layered(m, Q.mul_table(case.q), L[b], LQ.MAX_ITER)
        assert np.array_equal(r["out"], w["DecodeOutput"][b]) and (r["it"], r["ok"]) == (w["iter_number"][b], w["ok"][b]), (cid, b)
        assert Q.same_bits(r["APP"], w["LLR"][b]) and Q.same_bits(r["c2v"], w["L_c2v"][b]), (cid, b)


@pytest.mark.parametrize("cid", LQ.IDS)
def test_level_order_equals_row_order(nb, cid):
    """The rows of one level, each computed from the messages as they stood when the level began and stored together, level after
    level, give the bits of the rows run one after the other."""
    case = LQ.BY_ID[cid]
    m, L = LQ.matrix(nb, case), LQ.inputs(nb, case)
    N, M, _, _, edges = LQ.graph(case)
    level, order, begin = LQ.level_tables(M, edges)
    assert len(begin) - 1 == levels_of(M, edges) and sorted(order) == list(range(M))
    levels = [order[begin[k]:begin[k + 1]] for k in range(len(begin) - 1)]
    for rows in levels:  # the rows of a level share no variable
        cols = [c for r, c, _ in edges if r in rows]
        assert len(cols) == len(set(cols))
    for b in ((1, 6) if N <= 50 else (5,)):
        a = LQ.np_decode_layered(m, Q.mul_table(case.q), L[b], LQ.MAX_ITER)
        c = LQ.np_decode_layered(m, Q.mul_table(case.q), L[b], LQ.MAX_ITER, levels=levels)
        assert np.array_equal(a["out"], c["out"]) and (a["it"], a["ok"]) == (c["it"], c["ok"]), (cid, b)
        assert Q.same_bits(a["APP"], c["APP"]) and Q.same_bits(a["c2v"], c["c2v"]), (cid, b)


@pytest.mark.parametrize("cid", LQ.IDS)
def test_inputs_are_worth_decoding(nb, cid):
    """What tests/test_nb_qspa_layered_gpu.py relies on: by the layered host statement alone, the frames of every case stop at three or
    more different iteration counts and one at least fails; no state is NaN."""
    w = LQ.want(nb, LQ.BY_ID[cid])
    its, ok = w["iter_number"].tolist(), w["ok"].tolist()
    assert len(set(its)) >= 3 and 0 in ok and 1 in ok, (cid, its, ok)
    assert all(i == LQ.MAX_ITER for i, k in zip(its, ok) if not k)
    assert np.isfinite(w["LLR"]).all() and np.isfinite(w["L_c2v"]).all()
    assert w["LLR"].min() >= Q.FLOOR and w["LLR"].max() == 1 and w["L_c2v"].min() >= Q.FLOOR and w["L_c2v"].max() == 1


def test_the_level_structure_the_cases_are_there_for(nb):
    by = LQ.BY_ID
    assert [c.id for c in LQ.CASES[:len(Q.CASES)]] == Q.IDS, "the shapes of the flooding table, all of them"
    for c in LQ.CASES[:len(Q.CASES)]:
        assert LQ.graph(c)[4] is Q.graph(Q.BY_ID[c.id])[1]
    # a level wider than one pass of the largest workgroup (16 rows at q = 64), and one whose row count is no multiple of the 4
    # vectors a wave holds at q = 16; both graphs the same shape
    for cid in ("wide_q64", "wide_q16"):
        assert LQ.graph(by[cid])[0] >= 80 and LQ.level_widths(by[cid]) == [21, 21]
    assert 21 > 1024 // 64 and 21 % (64 // 16) != 0
    # levels of one row next to wide ones; the ladder: nothing but single rows
    wd = LQ.level_widths(by["mix_q16"])
    assert max(wd) >= 3 and wd.count(1) >= 3 and wd[-1] == 1
    assert set(LQ.level_widths(by["ladder"])) == {1} and len(LQ.level_widths(by["ladder"])) == LQ.graph(by["ladder"])[1]
    # column weights 0, 1 and dvmax, the last two in one row
    N, M, dv, dc, edges = LQ.graph(by["thin_q32"])
    colw = np.bincount([c for _, c, _ in edges], minlength=N)
    assert colw[0] == 0 and sorted(set(colw.tolist())) == [0, 1, dv]
    assert any({1, dv} <= {int(colw[c]) for r, c, _ in edges if r == row} for row in range(M))
    m = LQ.matrix(nb, by["thin_q32"])
    assert m.vn_weight.tolist() == colw.tolist() and m.cn_weight.min() >= 2
    # both sizes the rule can choose are chosen on some case; the third of the set runs pinned (test_nb_qspa_layered_gpu.py)
    chosen = {LQ.threads_rule(c.q, max(LQ.level_widths(c))) for c in LQ.CASES}
    assert chosen == {256, 512} and set(LQ.THREAD_SET) == {256, 512, 1024}
    assert LQ.threads_rule(by[LQ.PINNED].q, 21) == 512 and 256 // 64 * 4 < 21


@pytest.mark.parametrize("cid", ["q8", "q64_dv3", "q128", "mix_q16"])
def test_batch_equals_its_frames(nb, cid):
    case = LQ.BY_ID[cid]
    m, L, w = LQ.matrix(nb, case), LQ.inputs(nb, case), LQ.want(nb, case)
    for b in (0, 3, 7, 11):
        one = nb.Decoding_QSPA_host(m, L[b:b + 1], LQ.MAX_ITER, want_state=True, layered=True)
        for k in ("DecodeOutput", "iter_number", "ok"):
            assert np.array_equal(one[k][0], w[k][b])
        assert Q.same_bits(one["LLR"][0], w["LLR"][b]) and Q.same_bits(one["L_c2v"][0], w["L_c2v"][b])


@pytest.mark.parametrize("cid", ["q8", "q64_dv3", "wide_q16", "thin_q32"])
def test_one_iteration(nb, cid):
    """maxIT = 1: a frame that needed more fails with the first iteration's state, which the numpy restatement gives too."""
    case = LQ.BY_ID[cid]
    m, L, w = LQ.matrix(nb, case), LQ.inputs(nb, case), LQ.want(nb, case)
    one = LQ.want(nb, case, 1)
    assert ((one["ok"] == 1) == (w["iter_number"] == 0) & (w["ok"] == 1)).all() and (one["iter_number"][one["ok"] == 0] == 1).all()
    b = int(np.flatnonzero(one["ok"] == 0)[0])
    r = LQ.np_decode_layered(m, Q.mul_table(case.q), L[b], 1)
    assert np.array_equal(r["out"], one["DecodeOutput"][b]) and Q.same_bits(r["APP"], one["LLR"][b]) and Q.same_bits(r["c2v"], one["L_c2v"][b])


def test_layered_differs_from_flooding(nb):
    """The keyword selects another decoder: on a case's frames the two host statements' c2v differ, and layered=False is the flooding
    statement of tests/nb_qspa_cases.py."""
    case = LQ.BY_ID["q64"]
    m, L = LQ.matrix(nb, case), LQ.inputs(nb, case)
    flood = nb.Decoding_QSPA_host(m, L, LQ.MAX_ITER, want_state=True, layered=False)
    again = nb.Decoding_QSPA_host(m, L, LQ.MAX_ITER, want_state=True)
    assert Q.same_bits(flood["L_c2v"], again["L_c2v"]) and np.array_equal(flood["iter_number"], again["iter_number"])
    assert not Q.same_bits(flood["L_c2v"], LQ.want(nb, case)["L_c2v"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def raw_host(nb, m, mul, L, B, maxIT, out=True, cn_gf=None, q=None):
    lib = nb.lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    o, it, ok = np.zeros((max(B, 1), m.N), np.int32), np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
    gf = m.cn_linkVNs_GF if cn_gf is None else cn_gf
    return lib.nbldpc_qspa_layered_decode_host(m.N, m.M, m.q if q is None else q, m.dv, m.dc, p(m.vn_weight), p(m.vn_linkCNs), p(m.vn_linkCNs_GF),
                                               p(m.cn_weight), p(m.cn_linkVNs), p(gf), p(mul), None if L is None else p(L), B, maxIT,
                                               p(o) if out else None, p(it), p(ok), None, None)


def test_refusals(nb):
    case = LQ.BY_ID["q16_part"]
    m, mul, L = LQ.matrix(nb, case), Q.mul_table(case.q), np.ascontiguousarray(LQ.inputs(nb, case)[:2])
    EINVAL, EUNSUPPORTED = -1, -5
    assert raw_host(nb, m, mul, L, 2, 8) == 0
    assert raw_host(nb, m, mul, L, 2, 0) == EINVAL and raw_host(nb, m, mul, L, 0, 8) == EINVAL
    assert raw_host(nb, m, mul, None, 2, 8) == EINVAL and raw_host(nb, m, mul, L, 2, 8, out=False) == EINVAL
    assert raw_host(nb, m, mul, L, 2, 8, q=2) == EUNSUPPORTED and raw_host(nb, m, mul, L, 2, 8, q=512) == EUNSUPPORTED
    gf = m.cn_linkVNs_GF.copy()
    gf[3, 1] = 0
    assert raw_host(nb, m, mul, L, 2, 8, cn_gf=gf) == EUNSUPPORTED and b"coefficient is 0" in nb.lib.nbldpc_last_error()
    gf = m.cn_linkVNs_GF.copy()
    gf[3, 1] ^= 1
    if gf[3, 1] == 0:
        gf[3, 1] = 2
    assert raw_host(nb, m, mul, L, 2, 8, cn_gf=gf) == EINVAL, "the two views of the graph differ"
    with pytest.raises(ValueError):
        nb.Decoding_QSPA_host(m, L[:, :-1], 8, layered=True)


class _Graph:
    """One row that lists variable 0 in slots 0 and 2 with one coefficient: both views agree under the first-match cross indices."""
    N, M, q, dv, dc = 3, 1, 16, 2, 4
    vn_weight = np.array([2, 1, 1], np.int32)
    vn_linkCNs = np.array([[0, 0], [0, 0], [0, 0]], np.int32)
    vn_linkCNs_GF = np.array([[1, 1], [2, 0], [3, 0]], np.int32)
    cn_weight = np.array([4], np.int32)
    cn_linkVNs = np.array([[0, 1, 0, 2]], np.int32)
    cn_linkVNs_GF = np.array([[1, 2, 1, 3]], np.int32)


def test_a_row_that_lists_a_variable_twice_is_refused(nb):
    """The flooding statement takes such a row (as nbldpc_code_create does); the layered one has no other-edges rule for it:
    NBLDPC_EUNSUPPORTED, outputs untouched."""
    from cuda_ldpc_amd._lib import LdpcError
    g = _Graph()
    g.TableMultiply = Q.mul_table(16)
    L = np.full((1, 3, 15), -1.0, f32)
    assert nb.Decoding_QSPA_host(g, L, 2)["ok"].shape == (1,)
    with pytest.raises(LdpcError, match=r"\(-5\).*two slots"):
        nb.Decoding_QSPA_host(g, L, 2, layered=True)


# ---- fewer iterations than flooding -------------------------------------------------------------------------------------------------------
BDS_SNR = 2.0  # chosen with the flooding statement alone: its mean iter_number over the 200 frames is 4.95 there (maxIT 20)


def test_fewer_iterations_than_flooding_on_bds(nb, orc):
    """BDS.576.288.GF.64 over BPSK, the shipped codeword, 200 frames of the oracle's channel, 20 iterations, at an Eb/N0 at which the
    flooding statement needs 4 iterations or more on average: the layered statement's total iteration count is strictly smaller.
    Measured: flooding 990 iterations (1 frame in error), layered 608 (1): ratio 0.614."""
    nbd = os.path.join(DATA, "nb")
    oc = orc.NBCode(os.path.join(nbd, "BDS.576.288.GF.64.txt"), os.path.join(nbd, "GF", "Arith.Table.GF.64.txt"))
    m = nb.NBMatrix(os.path.join(nbd, "BDS.576.288.GF.64.txt"))
    mul, _, _ = nb.GFInitial(64, os.path.join(nbd, "GF", "Arith.Table.GF.64.txt"))
    cw = np.loadtxt(os.path.join(nbd, "codeword_bds_gf64.txt"), dtype=np.int32)
    seed = np.array([173, 173, 173], np.int32)
    sigma = orc.nb_sigma(BDS_SNR, oc.rate)
    L = np.stack([orc.nb_channel(oc, cw, seed, sigma)[1] for _ in range(200)])
    flood = nb.Decoding_QSPA_host(m, L, 20, TableMultiply=mul)
    lay = nb.Decoding_QSPA_host(m, L, 20, TableMultiply=mul, layered=True)
    tot = [int(r["iter_number"].sum()) for r in (flood, lay)]
    bad = [int((r["DecodeOutput"] != cw[None, :]).any(axis=1).sum()) for r in (flood, lay)]
    print("200 frames at %.2f dB, maxIT 20: flooding %d iterations, %d frames in error; layered %d iterations, %d frames in error; ratio %.3f"
          % (BDS_SNR, tot[0], bad[0], tot[1], bad[1], tot[1] / tot[0]))
    assert tot[0] >= 4 * 200, "the operating point: flooding needs 4 iterations or more on average"
    assert tot[1] < tot[0]


# ---- the level tables the kernel walks against their restatement -------------------------------------------------------------------------
def test_level_tables_equal_the_plan(tmp_path):
    """row_order and level_begin as nb_tables_build makes them (tests/cpp/nb_plan_host_test.hip prints the FNV-1a 64 digest of every
    table it would upload; the level tables are the last two where the trellis kernels are offered) against level_tables() here."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "nb_plan_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", os.path.join(here, "cpp", "nb_plan_host_test.hip"),
                           "-o", exe], cwd=str(tmp_path))
    for cid in ("wide_q16", "mix_q16", "q64_tail", "ladder"):
        case = LQ.BY_ID[cid]
        _, M, _, _, edges = LQ.graph(case)
        out = subprocess.run([exe, cid] + list(LQ.files(case)) + ["0"], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.splitlines()[-1] == "OK 1", out.stdout + out.stderr
        tok = out.stdout.splitlines()[0].split()
        _, order, begin = LQ.level_tables(M, edges)
        assert int(tok[5]) == len(begin) - 1 and int(tok[6]) == 1 and len(tok) == 8 + 11, (cid, tok)
        assert tok[-2:] == [plan_digest(np.array(order, np.int32)), plan_digest(np.array(begin, np.int32))], cid


def plan_digest(a):
    """The digest nb_plan_host_test.hip prints: FNV-1a 64 with that program's own offset basis."""
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


# ---- the host statement under the host sanitizers, stand-alone ---------------------------------------------------------------------------
def fnv64(a):
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.fixture(scope="module")
def layered_exe(tmp_path_factory):
    """tests/cpp/nb_qspa_layered_host_test.hip, built as test_nb_qspa_cpu.py builds nb_qspa_host_test.hip, with address + undefined."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("nb_qspa_layered_host")
    exe = str(tmp / "nb_qspa_layered_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "nb_qspa_layered_host_test.hip"), "-o", exe],
                          cwd=str(tmp))
    return exe


@pytest.mark.parametrize("cid", ["q4", "q32", "q64_dv4", "q256", "ladder", "dc12_q8", "wide_q16", "mix_q16", "thin_q32"])
def test_host_statement_stand_alone_under_sanitizers(nb, layered_exe, tmp_path, cid):
    case = LQ.BY_ID[cid]
    L, w = LQ.inputs(nb, case), LQ.want(nb, case)
    llr = str(tmp_path / "llr.bin")
    L.tofile(llr)
    out = subprocess.run([layered_exe, LQ.files(case)[0], str(POLY[case.q]), llr, str(L.shape[0]), str(LQ.MAX_ITER)], capture_output=True, text=True)
    assert out.returncode == 0 and "refusals ok" in out.stdout, out.stdout + out.stderr
    want = " ".join(fnv64(w[k]) for k in ("DecodeOutput", "iter_number", "ok", "LLR", "L_c2v"))
    assert out.stdout.splitlines()[0] == want, "the stand-alone build of the host statement differs from the library's"
