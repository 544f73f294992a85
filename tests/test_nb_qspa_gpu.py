"""k_nb_qspa, the FHT sum-product kernel, against its definition nbldpc_qspa_decode_host: DecodeOutput, iter_number, ok, APP and c2v
bit for bit, on the cases of tests/nb_qspa_cases.py (every field size 4 ... 256, sub-wave vectors with a partly empty last wave, more
than 96 columns, column weights 3 and 4, irregular rows, rows of weight 2 and 12, a code just under the LDS bound and one just over),
batches of 1, 3 and 300, maxIT 1 and 8, the shipped matrices, a rate-matched input and the simulation loop; and every cross-lane step
of the kernel against a plain LDS exchange (tests/cpp/qspa_step_test.hip).  tests/test_nb_qspa_cpu.py asserts that the inputs are
worth decoding and that the host statement is what include/nbldpc.h says."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import nb_qspa_cases as Q
from conftest import DATA

pytestmark = pytest.mark.gpu
NB = os.path.join(DATA, "nb")


@pytest.fixture(scope="module")
def nb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cuda_ldpc_amd import nbldpc
    return nbldpc


_CODES = {}


def dev_code(nb, case):
    if case.id not in _CODES:
        _CODES[case.id] = nb.NBCode(Q.files(case)[0], Q.mul_table(case.q))
    return _CODES[case.id]


def dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()  # a writable copy: the cases' inputs are read-only


def assert_same(r, w, what):
    torch.cuda.synchronize()
    for k in ("DecodeOutput", "iter_number", "ok"):
        assert np.array_equal(r[k].cpu().numpy(), w[k]), (what, k, r[k].cpu().numpy().tolist(), w[k].tolist())
    for k in ("LLR", "L_c2v"):
        if w[k] is not None:
            got = r[k].cpu().numpy()
            assert Q.same_bits(got, w[k]), (what, k, int((got.view(np.uint32) != w[k].view(np.uint32)).sum()), "entries differ")


def test_cross_lane_steps(tmp_path):
    """Each cross-lane fetch (DPP, ds_swizzle, ds_bpermute), the vector maximum and the transform of every field size against a plain
    exchange through LDS."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "qspa_step_test")
    subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function",
                           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "qspa_step_test.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "total 0" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("cid", Q.IDS)
def test_kernel_equals_host_statement(nb, cid):
    case = Q.BY_ID[cid]
    code, L, w = dev_code(nb, case), Q.inputs(nb, case), Q.want(nb, case)
    r = nb.Decoding_QSPA(code, dev(L), Q.MAX_ITER, want_state=True)
    assert code.last_kernel == "k_nb_qspa"
    assert_same(r, w, cid)
    r = nb.Decoding_QSPA(code, dev(L), Q.MAX_ITER)  # without the state outputs
    assert r["LLR"] is None and r["L_c2v"] is None
    assert_same(r, dict(w, LLR=None, L_c2v=None), cid)


@pytest.mark.parametrize("cid", ["q4", "q16_part", "q64_dv3", "q256", "dc12_q8"])
def test_one_iteration(nb, cid):
    case = Q.BY_ID[cid]
    assert_same(nb.Decoding_QSPA(dev_code(nb, case), dev(Q.inputs(nb, case)), 1, want_state=True), Q.want(nb, case, 1), cid)


@pytest.mark.parametrize("cid", ["q16_part", "q64", "q128"])
@pytest.mark.parametrize("B", [1, 3, 300])
def test_batch_sizes(nb, cid, B):
    case = Q.BY_ID[cid]
    L = Q.inputs(nb, case)
    idx = (np.arange(B) * 5 + 1) % L.shape[0]  # frame b of the batch is frame 5 b + 1 of the case: every frame, in another order
    w = Q.want(nb, case)
    r = nb.Decoding_QSPA(dev_code(nb, case), dev(L[idx]), Q.MAX_ITER, want_state=True)
    assert_same(r, {k: np.ascontiguousarray(w[k][idx]) for k in w}, (cid, B))


def test_lds_bound_refusal(nb):
    """The (2, 4) code over GF(64) with 206 columns needs 163 144 bytes: NBLDPC_EUNSUPPORTED, nothing launched, outputs untouched; the
    one with 204 columns (161 600 bytes) is in the table."""
    from cuda_ldpc_amd._lib import LdpcError
    case = Q.LDS_OVER
    M, _ = Q.graph(case)
    assert Q.lds_bytes(case.N, M, case.q, case.dc) > Q.LDS_LIMIT
    code = dev_code(nb, case)
    L = torch.zeros((2, case.N, case.q - 1), dtype=torch.float32, device="cuda")
    with pytest.raises(LdpcError, match=r"\(-5\).*LDS"):
        nb.Decoding_QSPA(code, L, 4)
    assert code.last_kernel != "k_nb_qspa"
    torch.cuda.synchronize()
    m = nb.NBMatrix(Q.files(case)[0])
    m.TableMultiply = Q.mul_table(case.q)
    assert nb.Decoding_QSPA_host(m, L.cpu().numpy(), 4)["ok"].tolist() == [1, 1], "the host statement has no such bound"


def test_shipped_bds(nb):
    """BDS.576.288.GF.64, 32 frames at 2 and 3 dB, 20 iterations."""
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "BDS.576.288.GF.64.txt"), mul)
    rng = np.random.default_rng(9)
    L = np.concatenate([Q.bpsk_llr(nb, code.N, 64, s, 0.5, rng, 16) for s in (2.0, 3.0)])
    w = nb.Decoding_QSPA_host(code, L, 20, want_state=True)
    assert len(set(w["iter_number"].tolist())) >= 3
    assert_same(nb.Decoding_QSPA(code, dev(L), 20, want_state=True), w, "BDS")


def test_shipped_gf256(nb):
    """LDPC_N96_K48_GF256_d1_exp: decoded like any code if every edge coefficient is non-zero, refused if one is 0."""
    from cuda_ldpc_amd._lib import LdpcError
    mul, _, _ = nb.GFInitial(256, os.path.join(NB, "GF", "Arith.Table.GF.256.txt"))
    code = nb.NBCode(os.path.join(NB, "LDPC_N96_K48_GF256_d1_exp.txt"), mul)
    used = np.arange(code.dc)[None, :] < code.cn_weight[:, None]
    rng = np.random.default_rng(10)
    L = np.concatenate([Q.bpsk_llr(nb, code.N, 256, s, 0.5, rng, 4) for s in (2.0, 4.0)])
    if (code.cn_linkVNs_GF[used] == 0).any():
        with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
            nb.Decoding_QSPA(code, dev(L), 20)
        with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
            nb.Decoding_QSPA_host(code, L, 20)
    else:
        assert_same(nb.Decoding_QSPA(code, dev(L), 20, want_state=True), nb.Decoding_QSPA_host(code, L, 20, want_state=True), "GF256")


def test_rate_matched_input(nb):
    """Two shortened and four punctured symbols through nbldpc_rm_demodulate_bpsk_recover: -1e4 and +0.0 vectors among the noisy ones."""
    import cuda_ldpc_amd as C
    case = Q.BY_ID["q64"]
    code = dev_code(nb, case)
    rm = C.RateMatch(case.N, [0, 5], range(20, 24))
    words = torch.zeros((6, case.N), dtype=torch.int32, device="cuda")
    rx = nb.AWGNChannel_RM_GPU(np.array([173, 173, 173], np.int32), 0.7, rm, case.q, nb.RM_Select(rm, words))
    L = nb.RM_Demodulate_Recover(rm, case.q, rx, 0.7)
    Lh = L.cpu().numpy()
    assert (Lh[:, [0, 5]] == -1e4).all() and (Lh[:, 20:] == 0).all()
    w = nb.Decoding_QSPA_host(Q.matrix(nb, case), Lh, Q.MAX_ITER, want_state=True)
    r = nb.Decoding_QSPA(code, L, Q.MAX_ITER, want_state=True)
    assert_same(r, w, "rate matched")
    assert (w["DecodeOutput"][:, [0, 5]] == 0).all() and np.isfinite(w["LLR"]).all()


def test_simulation_counts_what_the_host_statement_decodes(nb):
    """Simulation_GPU(decoder_method=4) over the device channel with random codewords: the counters of the same 24 frames decoded by
    Decoding_QSPA_host."""
    from cuda_ldpc_amd import nb_simulation as S
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "BDS.576.288.GF.64.txt"), mul)
    sigma, B, maxIT = nb.sigma_of(2.0, code.rate), 24, 6
    sim = S.NBSim(2.0)
    seed = np.array([173, 173, 173], np.int32)
    S.Simulation_GPU(code, seed, sigma, sim, None, maxIT=maxIT, batch=B, leastErrorFrames=10 ** 6, max_frames=B, device_channel=True,
                     decoder_method=4, PN_Message=1, pn_seed=7)
    assert code.last_kernel == "k_nb_qspa" and sim.num_Frames == B
    words = nb.PN_CodeWords(code, 7, B, first_frame=0)
    rx = nb.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code, words, B)
    w = nb.Decoding_QSPA_host(code, nb.Demodulate(code, rx, sigma).cpu().numpy(), maxIT)
    errs = (w["DecodeOutput"] != words.cpu().numpy()).sum(axis=1)
    assert (sim.num_Error_Frames, sim.num_Error_Bits, sim.Total_Iteration) == (int((errs > 0).sum()), int(errs.sum()), int(w["iter_number"].sum()))


def test_device_refusals(nb):
    """maxIT < 1 is NBLDPC_EINVAL; a code with a zero edge coefficient (the shipped exponent-format GF(64) file, which EMS decodes with
    the zeros in place) is NBLDPC_EUNSUPPORTED on the device and in the host statement alike.  Nothing is launched."""
    from cuda_ldpc_amd._lib import LdpcError
    case = Q.BY_ID["q64"]
    with pytest.raises(LdpcError, match=r"\(-1\)"):
        nb.Decoding_QSPA(dev_code(nb, case), dev(Q.inputs(nb, case)), 0)
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "LDPC_N576_K288_GF64_d1_exp.txt"), mul)
    used = np.arange(code.dc)[None, :] < code.cn_weight[:, None]
    assert (code.cn_linkVNs_GF[used] == 0).any()
    L = np.zeros((1, code.N, 63), np.float32)
    with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
        nb.Decoding_QSPA(code, dev(L), 4)
    with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
        nb.Decoding_QSPA_host(code, L, 4)
    assert code.last_kernel == "none"
    torch.cuda.synchronize()
