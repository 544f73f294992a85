"""The FHT sum-product decoder without a GPU: the shared exponential against float64 exp, nbldpc_qspa_decode_host (plain C++, the
definition of the decoder inside the product) against an fp32 numpy restatement of include/nbldpc.h written in
tests/nb_qspa_cases.py, bit for bit, on every case of the table; the check-node rule against the float64 brute-force convolution;
special values; the frame error rate against EMS(2,2) on the same noise; the refusals; a batch against its frames one at a time; the
condition on the inputs that tests/test_nb_qspa_gpu.py relies on; and the host statement as a stand-alone program
(tests/cpp/nb_qspa_host_test.hip) under the address + undefined sanitizers."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import nb_qspa_cases as Q
from nb_shape_cases import POLY, gf_tables

from conftest import DATA

f32 = np.float32
# Largest relative error of qspa_exp against float64 exp measured on exp_arguments() (402 177 arguments): 9.78e-08 (at x = -71.02).
EXP_REL_MEASURED = 9.78e-8
EXP_REL_BOUND = 2 * EXP_REL_MEASURED
# Largest deviation of the fp32 FHT check-node rule from the float64 convolution, entries above the floor, relative to the vector's
# maximum, measured on check_rows(): 1.55e-07 (weight 3 over GF(16)).
CN_DEV_MEASURED = 1.55e-7
CN_DEV_BOUND = 4 * CN_DEV_MEASURED


@pytest.fixture(scope="module")
def nb():
    from cuda_ldpc_amd import nbldpc
    return nbldpc


def exp_arguments():
    """A dense set of fp32 arguments in [-90, 0]: 400 001 evenly spaced, every range-reduction boundary -(k + 1/2) ln 2 with its eight
    neighbours on either side, the cut -87 with its neighbours, and 0."""
    xs = [np.linspace(-90, 0, 400001).astype(f32)]
    for k in range(131):
        b = f32(-(k + 0.5) * np.log(2.0))
        up = dn = b
        v = [b]
        for _ in range(8):
            up, dn = np.nextafter(up, f32(0)), np.nextafter(dn, f32(-100))
            v += [up, dn]
        xs.append(np.array(v, f32))
    xs.append(np.array([0, -87, np.nextafter(f32(-87), f32(-100)), np.nextafter(f32(-87), f32(0)), -90], f32))
    x = np.unique(np.concatenate(xs))
    return x[(x <= 0) & (x >= -90)]


def test_qspa_exp_against_float64(nb):
    x = exp_arguments()
    y = nb.QSPA_Exp_host(x)
    live = x >= -87
    ref = np.exp(x.astype(np.float64))
    rel = np.abs(y[live].astype(np.float64) - ref[live]) / ref[live]
    print("qspa_exp: %d arguments, largest relative error %.3e at x = %r" % (x.size, rel.max(), float(x[live][rel.argmax()])))
    assert rel.max() <= EXP_REL_BOUND
    assert y[x == 0].tolist() == [1.0]
    assert (~live).sum() > 1000 and (y[~live] == 0).all() and np.signbit(y[~live]).sum() == 0
    assert (np.diff(y) >= 0).all(), "not monotone"
    assert y[live].min() >= 2.0 ** -126, "a result below the normal range"
    assert Q.same_bits(Q.np_exp(x), y), "the numpy restatement of qspa_exp differs"
    assert nb.QSPA_Exp_host(np.array([-np.inf, -1e30, np.nan], f32)).tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("cid", Q.IDS)
def test_host_statement_equals_numpy(nb, cid):
    case = Q.BY_ID[cid]
    m, L, w = Q.matrix(nb, case), Q.inputs(nb, case), Q.want(nb, case)
    M, edges = Q.graph(case)
    assert (m.N, m.M, m.q, m.dv, m.dc) == (case.N, M, case.q, case.dv, case.dc) and Q.lds_bytes(m.N, m.M, m.q, m.dc) <= Q.LDS_LIMIT
    frames = range(L.shape[0]) if case.N <= 100 else (0, 5, 9)  # the largest code: three frames (one fails, two stop at different counts)
    for b in frames:
        r = Q.np_decode(m, Q.mul_table(case.q), L[b], Q.MAX_ITER)
        assert np.array_equal(r["out"], w["DecodeOutput"][b]) and (r["it"], r["ok"]) == (w["iter_number"][b], w["ok"][b]), (cid, b)
        assert Q.same_bits(r["APP"], w["LLR"][b]) and Q.same_bits(r["c2v"], w["L_c2v"][b]), (cid, b)


@pytest.mark.parametrize("cid", Q.IDS)
def test_inputs_are_worth_decoding(nb, cid):
    """What tests/test_nb_qspa_gpu.py relies on: by the host statement alone, the frames of every case stop at three or more different
    iteration counts and one at least fails; no state is NaN."""
    w = Q.want(nb, Q.BY_ID[cid])
    its, ok = w["iter_number"].tolist(), w["ok"].tolist()
    assert len(set(its)) >= 3 and 0 in ok and 1 in ok, (cid, its, ok)
    assert all(i == Q.MAX_ITER for i, k in zip(its, ok) if not k)
    assert np.isfinite(w["LLR"]).all() and np.isfinite(w["L_c2v"]).all()
    assert w["LLR"].min() >= Q.FLOOR and w["LLR"].max() == 1 and w["L_c2v"].min() >= Q.FLOOR and w["L_c2v"].max() == 1


def test_the_shapes_the_cases_are_there_for():
    by = {c.id: c for c in Q.CASES}
    assert {c.q for c in Q.CASES} == {4, 8, 16, 32, 64, 128, 256}
    assert by["q64_tail"].N > 96 and by["q64_dv3"].dv == 3 and by["q64_dv4"].dv == 4 and by["q64"].drop == 0 and by["q64_tail"].drop > 0
    assert by["q16_part"].N % 4 and (Q.graph(by["q16_part"])[0]) % 4, "the last wave of variables and of rows is partly empty"
    M, edges = Q.graph(by["ladder"])
    assert np.bincount([c for _, c, _ in edges]).tolist() == [1] + [2] * (by["ladder"].N - 2) + [1]
    M, edges = Q.graph(by["dc12_q8"])
    assert sorted(set(np.bincount([r for r, _, _ in edges]).tolist())) == [11, 12]
    for c, fits in ((by["lds_under"], True), (Q.LDS_OVER, False)):
        assert (Q.lds_bytes(c.N, Q.graph(c)[0], c.q, c.dc) <= Q.LDS_LIMIT) == fits
    assert Q.LDS_OVER.N - by["lds_under"].N == 2, "the next (2, 4) code up"


# ---- the check-node rule against the convolution it computes -----------------------------------------------------------------------------
def check_rows():
    """(q, w, coefficients, inputs float32 [w, q]): weights 2, 3, 4 over GF(4), GF(8), GF(16), five rows each; random vectors spread
    over e^-12 ... 1, max-normalised."""
    rng = np.random.default_rng(77)
    for q, w in itertools.product((4, 8, 16), (2, 3, 4)):
        for _ in range(5):
            v = np.exp(rng.uniform(-12, 0, size=(w, q)))
            v = np.maximum(v / v.max(axis=1, keepdims=True), 2.0 ** -40).astype(f32)
            yield q, w, [int(h) for h in rng.integers(1, q, size=w)], v


def brute_force(q, hs, v, mul):
    """float64: c_t[a] = sum over the other edges' symbols x_s with XOR_s h_s x_s = h_t a of prod_s v_s[x_s], max-normalised."""
    w = len(hs)
    res = []
    for t in range(w):
        others = [s for s in range(w) if s != t]
        c = np.zeros(q)
        for xs in itertools.product(range(q), repeat=w - 1):
            acc, pr = 0, 1.0
            for s, xv in zip(others, xs):
                acc ^= int(mul[hs[s], xv])
                pr *= float(v[s, xv])
            a = int(np.flatnonzero(mul[hs[t]] == acc)[0])
            c[a] += pr
        res.append(c / c.max())
    return res


def test_check_node_rule_against_convolution():
    worst = 0.0
    for q, w, hs, v in check_rows():
        mul = gf_tables(q)[0]
        got = Q.np_check_node([v[t] for t in range(w)], hs, mul)
        ref = brute_force(q, hs, v, mul)
        for t in range(w):
            above = ref[t] > 2.0 ** -40
            dev = np.abs(got[t].astype(np.float64) - ref[t])[above].max()
            if dev > worst:
                worst, where = dev, (q, w)
    print("check-node rule: largest deviation %.3e at (q, w) = %s" % (worst, where))
    assert worst <= CN_DEV_BOUND


# ---- special values ------------------------------------------------------------------------------------------------------------------------
def finite_state(r):
    return np.isfinite(r["LLR"]).all() and np.isfinite(r["L_c2v"]).all() and r["LLR"].min() >= Q.FLOOR and r["L_c2v"].min() >= Q.FLOOR


@pytest.mark.parametrize("cid", ["q16_part", "q64", "q256"])
def test_special_values(nb, cid):
    case = Q.BY_ID[cid]
    m, V = Q.matrix(nb, case), case.q - 1
    # everything punctured
    r = nb.Decoding_QSPA_host(m, np.zeros((1, case.N, V), f32), Q.MAX_ITER, want_state=True)
    assert r["DecodeOutput"].tolist() == [[0] * case.N] and r["ok"].tolist() == [1] and r["iter_number"].tolist() == [0] and finite_state(r)
    assert (r["LLR"] == 1).all() and (r["L_c2v"] == 1).all()
    # two shortened symbols (-1e4 everywhere), the rest noisy: they decode to 0; a symbol at +1e4 on element 3 alone decodes to 3
    L = Q.inputs(nb, case)[4:8].copy()
    L[:, [0, 5], :] = f32(-1e4)
    r = nb.Decoding_QSPA_host(m, L, Q.MAX_ITER, want_state=True)
    assert finite_state(r) and (r["DecodeOutput"][:, [0, 5]] == 0).all()
    L2 = np.zeros((1, case.N, V), f32)
    L2[0, 2, :] = f32(-1e4)
    L2[0, 2, 2] = f32(1e4)
    r = nb.Decoding_QSPA_host(m, L2, 1, want_state=True)
    assert finite_state(r) and r["DecodeOutput"][0, 2] == 3 and r["ok"].tolist() == [0], "one forced symbol against an all-zero rest violates its checks"
    # one column at the extremes of the format, the rest punctured: elements 1, 3, 5, ... at -big, elements 2, 4, 6, ... at +big
    for big, first in ((3e38, 2), (-3e38, 1)):
        L3 = np.zeros((1, case.N, V), f32)
        L3[0, 1, :] = f32(big)
        L3[0, 1, ::2] = f32(-big)
        one = nb.Decoding_QSPA_host(m, L3, 1, want_state=True)
        assert finite_state(one) and one["DecodeOutput"][0, 1] == first, big
        want = np.full(case.q, Q.FLOOR, f32)  # the differences to the maximum are infinite: 1 where the maximum is, the floor elsewhere
        want[first::2] = 1
        assert Q.same_bits(one["LLR"][0, 1], want)
        # and among noisy symbols, through all iterations
        L4 = Q.inputs(nb, case)[8:10].copy()
        L4[:, 1, :] = L3[0, 1, :]
        r = nb.Decoding_QSPA_host(m, L4, Q.MAX_ITER, want_state=True)
        assert finite_state(r), big
        ref = Q.np_decode(m, Q.mul_table(case.q), L4[0], Q.MAX_ITER)
        assert np.array_equal(ref["out"], r["DecodeOutput"][0]) and Q.same_bits(ref["APP"], r["LLR"][0]) and Q.same_bits(ref["c2v"], r["L_c2v"][0])


ERR_SNR = 3.0  # Eb/N0 of test_error_rate_against_ems, chosen with the oracle's EMS(2,2) alone: it leaves 82 of the 400 frames in error there


def test_error_rate_against_ems(nb, orc):
    """BDS.576.288.GF.64 over BPSK, the shipped codeword, 400 frames of the oracle's channel, 10 iterations: at an Eb/N0 at which
    EMS(2,2) (the oracle's Decoding_EMS) leaves at least 20 frames in error, the host statement leaves strictly fewer."""
    nbd = os.path.join(DATA, "nb")
    oc = orc.NBCode(os.path.join(nbd, "BDS.576.288.GF.64.txt"), os.path.join(nbd, "GF", "Arith.Table.GF.64.txt"))
    m = nb.NBMatrix(os.path.join(nbd, "BDS.576.288.GF.64.txt"))
    mul, _, _ = nb.GFInitial(64, os.path.join(nbd, "GF", "Arith.Table.GF.64.txt"))
    cw = np.loadtxt(os.path.join(nbd, "codeword_bds_gf64.txt"), dtype=np.int32)
    seed = np.array([173, 173, 173], np.int32)
    sigma = orc.nb_sigma(ERR_SNR, oc.rate)
    L = np.stack([orc.nb_channel(oc, cw, seed, sigma)[1] for _ in range(400)])
    ems = sum(int((orc.nb_ems_decode(oc, L[b], 2, 2, 10)["out"] != cw).any()) for b in range(400))
    r = nb.Decoding_QSPA_host(m, L, 10, TableMultiply=mul)
    spa = int((r["DecodeOutput"] != cw[None, :]).any(axis=1).sum())
    print("frame errors of 400 at %.2f dB after 10 iterations: EMS(2,2) %d, FHT sum-product %d" % (ERR_SNR, ems, spa))
    assert ems >= 20
    assert spa < ems


# ---- refusals, batches --------------------------------------------------------------------------------------------------------------------
def raw_host(nb, m, mul, L, B, maxIT, out=True, cn_gf=None, q=None):
    lib = nb.lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    o, it, ok = np.zeros((max(B, 1), m.N), np.int32), np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
    gf = m.cn_linkVNs_GF if cn_gf is None else cn_gf
    return lib.nbldpc_qspa_decode_host(m.N, m.M, m.q if q is None else q, m.dv, m.dc, p(m.vn_weight), p(m.vn_linkCNs), p(m.vn_linkCNs_GF),
                                       p(m.cn_weight), p(m.cn_linkVNs), p(gf), p(mul), None if L is None else p(L), B, maxIT,
                                       p(o) if out else None, p(it), p(ok), None, None)


def test_refusals(nb):
    case = Q.BY_ID["q16_part"]
    m, mul, L = Q.matrix(nb, case), Q.mul_table(case.q), np.ascontiguousarray(Q.inputs(nb, case)[:2])
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
        nb.Decoding_QSPA_host(m, L[:, :-1], 8)


@pytest.mark.parametrize("cid", ["q8", "q64_dv3", "q128"])
def test_batch_equals_its_frames(nb, cid):
    case = Q.BY_ID[cid]
    m, L, w = Q.matrix(nb, case), Q.inputs(nb, case), Q.want(nb, case)
    for b in (0, 3, 7, 11):
        one = nb.Decoding_QSPA_host(m, L[b:b + 1], Q.MAX_ITER, want_state=True)
        for k in ("DecodeOutput", "iter_number", "ok"):
            assert np.array_equal(one[k][0], w[k][b])
        assert Q.same_bits(one["LLR"][0], w["LLR"][b]) and Q.same_bits(one["L_c2v"][0], w["L_c2v"][b])
    # maxIT = 1: a frame that needed more fails with the first iteration's state
    one = nb.Decoding_QSPA_host(m, L, 1)
    assert ((one["ok"] == 1) == (w["iter_number"] == 0) & (w["ok"] == 1)).all() and (one["iter_number"][one["ok"] == 0] == 1).all()


# ---- the host statement under the host sanitizers, stand-alone ---------------------------------------------------------------------------
def fnv64(a):
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.fixture(scope="module")
def qspa_exe(tmp_path_factory):
    """tests/cpp/nb_qspa_host_test.hip, built as test_bp_cpu.py builds bp_host_test.hip, with address + undefined."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("nb_qspa_host")
    exe = str(tmp / "nb_qspa_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "nb_qspa_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("cid", ["q4", "q32", "q64_dv4", "q256", "ladder", "dc12_q8"])
def test_host_statement_stand_alone_under_sanitizers(nb, qspa_exe, tmp_path, cid):
    case = Q.BY_ID[cid]
    L, w = Q.inputs(nb, case), Q.want(nb, case)
    llr = str(tmp_path / "llr.bin")
    L.tofile(llr)
    out = subprocess.run([qspa_exe, Q.files(case)[0], str(POLY[case.q]), llr, str(L.shape[0]), str(Q.MAX_ITER)], capture_output=True, text=True)
    assert out.returncode == 0 and "refusals ok" in out.stdout, out.stdout + out.stderr
    want = " ".join(fnv64(w[k]) for k in ("DecodeOutput", "iter_number", "ok", "LLR", "L_c2v"))
    assert out.stdout.splitlines()[0] == want, "the stand-alone build of the host statement differs from the library's"
