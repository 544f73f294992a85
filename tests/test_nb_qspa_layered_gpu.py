"""k_nb_qspa_layered, the layered schedule of the FHT sum-product kernel, against its definition nbldpc_qspa_layered_decode_host:
DecodeOutput, iter_number, ok, APP and c2v bit for bit, on the cases of tests/nb_qspa_layered_cases.py (the shapes of the flooding
table, levels wider than one pass of the workgroup, single-row levels, column weights 0, 1 and dvmax), under every workgroup size of
the kernel's set, batches of 1, 3 and 300, maxIT 1 and 8, the shipped matrices, a rate-matched input, the simulation loop and the
refusals.  tests/test_nb_qspa_layered_cpu.py asserts that the inputs are worth decoding, that the cases have the level structure they
are there for, and that the host statement is what include/nbldpc.h says."""
import os

import numpy as np
import pytest
import torch

import nb_qspa_cases as Q
import nb_qspa_layered_cases as LQ
from conftest import DATA

pytestmark = pytest.mark.gpu
NB = os.path.join(DATA, "nb")
SWITCH = "NBLDPC_QSPA_LAYERED_THREADS"


@pytest.fixture(scope="module")
def nb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cuda_ldpc_amd import nbldpc
    return nbldpc


_CODES = {}


def dev_code(nb, case, threads=None):
    """The case's code object; threads: created with the workgroup size pinned by the experiment switch (read at create time)."""
    if (case.id, threads) not in _CODES:
        old = os.environ.pop(SWITCH, None)
        try:
            if threads is not None:
                os.environ[SWITCH] = str(threads)
            _CODES[(case.id, threads)] = nb.NBCode(LQ.files(case)[0], Q.mul_table(case.q))
        finally:
            os.environ.pop(SWITCH, None)
            if old is not None:
                os.environ[SWITCH] = old
    return _CODES[(case.id, threads)]


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


@pytest.mark.parametrize("cid", LQ.IDS)
def test_kernel_equals_host_statement(nb, cid):
    case = LQ.BY_ID[cid]
    code, L, w = dev_code(nb, case), LQ.inputs(nb, case), LQ.want(nb, case)
    assert code.qspa_layered_threads == LQ.threads_rule(case.q, max(LQ.level_widths(case)))
    r = nb.Decoding_QSPA(code, dev(L), LQ.MAX_ITER, want_state=True, layered=True)
    assert code.last_kernel == "k_nb_qspa_layered"
    assert_same(r, w, cid)
    r = nb.Decoding_QSPA(code, dev(L), LQ.MAX_ITER, layered=True)  # without the state outputs
    assert r["LLR"] is None and r["L_c2v"] is None
    assert_same(r, dict(w, LLR=None, L_c2v=None), cid)


@pytest.mark.parametrize("threads", LQ.THREAD_SET)
@pytest.mark.parametrize("cid", [LQ.PINNED, "q64_tail", "q256"])
def test_results_do_not_depend_on_the_workgroup_size(nb, cid, threads):
    """One code under each workgroup size of the kernel's set, pinned at create time: the host statement's bits under every one."""
    case = LQ.BY_ID[cid]
    code = dev_code(nb, case, threads)
    assert code.qspa_layered_threads == threads
    r = nb.Decoding_QSPA(code, dev(LQ.inputs(nb, case)), LQ.MAX_ITER, want_state=True, layered=True)
    assert code.last_kernel == "k_nb_qspa_layered"
    assert_same(r, LQ.want(nb, case), (cid, threads))


@pytest.mark.parametrize("cid", ["q4", "q16_part", "q64_dv3", "q256", "dc12_q8"])
def test_one_iteration(nb, cid):
    case = LQ.BY_ID[cid]
    assert_same(nb.Decoding_QSPA(dev_code(nb, case), dev(LQ.inputs(nb, case)), 1, want_state=True, layered=True), LQ.want(nb, case, 1), cid)


@pytest.mark.parametrize("cid", ["q16_part", "wide_q64", "q128"])
@pytest.mark.parametrize("B", [1, 3, 300])
def test_batch_sizes(nb, cid, B):
    case = LQ.BY_ID[cid]
    L = LQ.inputs(nb, case)
    idx = (np.arange(B) * 5 + 1) % L.shape[0]  # frame b of the batch is frame 5 b + 1 of the case: every frame, in another order
    w = LQ.want(nb, case)
    r = nb.Decoding_QSPA(dev_code(nb, case), dev(L[idx]), LQ.MAX_ITER, want_state=True, layered=True)
    assert_same(r, {k: np.ascontiguousarray(w[k][idx]) for k in w}, (cid, B))


def test_flooding_call_unchanged(nb):
    """layered=False is still the flooding kernel and equals the flooding host statement: the check-row function both kernels now
    call did not move a bit."""
    case = Q.BY_ID["q64_dv3"]
    code = dev_code(nb, LQ.BY_ID["q64_dv3"])
    r = nb.Decoding_QSPA(code, dev(Q.inputs(nb, case)), Q.MAX_ITER, want_state=True, layered=False)
    assert code.last_kernel == "k_nb_qspa"
    assert_same(r, Q.want(nb, case), "flooding")


def test_shipped_bds(nb):
    """BDS.576.288.GF.64, 32 frames at 2 and 3 dB, 20 iterations."""
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "BDS.576.288.GF.64.txt"), mul)
    rng = np.random.default_rng(9)
    L = np.concatenate([Q.bpsk_llr(nb, code.N, 64, s, 0.5, rng, 16) for s in (2.0, 3.0)])
    w = nb.Decoding_QSPA_host(code, L, 20, want_state=True, layered=True)
    assert len(set(w["iter_number"].tolist())) >= 3
    assert_same(nb.Decoding_QSPA(code, dev(L), 20, want_state=True, layered=True), w, "BDS")
    assert code.last_kernel == "k_nb_qspa_layered"


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
            nb.Decoding_QSPA(code, dev(L), 20, layered=True)
        with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
            nb.Decoding_QSPA_host(code, L, 20, layered=True)
    else:
        assert_same(nb.Decoding_QSPA(code, dev(L), 20, want_state=True, layered=True),
                    nb.Decoding_QSPA_host(code, L, 20, want_state=True, layered=True), "GF256")


def test_rate_matched_input(nb):
    """Two shortened and four punctured symbols through nbldpc_rm_demodulate_bpsk_recover: -1e4 and +0.0 vectors among the noisy ones."""
    import cuda_ldpc_amd as C
    case = LQ.BY_ID["q64"]
    N = LQ.graph(case)[0]
    code = dev_code(nb, case)
    rm = C.RateMatch(N, [0, 5], range(20, 24))
    words = torch.zeros((6, N), dtype=torch.int32, device="cuda")
    rx = nb.AWGNChannel_RM_GPU(np.array([173, 173, 173], np.int32), 0.7, rm, case.q, nb.RM_Select(rm, words))
    L = nb.RM_Demodulate_Recover(rm, case.q, rx, 0.7)
    Lh = L.cpu().numpy()
    assert (Lh[:, [0, 5]] == -1e4).all() and (Lh[:, 20:] == 0).all()
    w = nb.Decoding_QSPA_host(LQ.matrix(nb, case), Lh, LQ.MAX_ITER, want_state=True, layered=True)
    r = nb.Decoding_QSPA(code, L, LQ.MAX_ITER, want_state=True, layered=True)
    assert_same(r, w, "rate matched")
    assert (w["DecodeOutput"][:, [0, 5]] == 0).all() and np.isfinite(w["LLR"]).all()


def test_simulation_counts_what_the_host_statement_decodes(nb):
    """Simulation_GPU(decoder_method=5) over the device channel with random codewords: the counters of the same 24 frames decoded by
    the layered host statement."""
    from cuda_ldpc_amd import nb_simulation as S
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "BDS.576.288.GF.64.txt"), mul)
    sigma, B, maxIT = nb.sigma_of(2.0, code.rate), 24, 6
    sim = S.NBSim(2.0)
    seed = np.array([173, 173, 173], np.int32)
    S.Simulation_GPU(code, seed, sigma, sim, None, maxIT=maxIT, batch=B, leastErrorFrames=10 ** 6, max_frames=B, device_channel=True,
                     decoder_method=5, PN_Message=1, pn_seed=7)
    assert code.last_kernel == "k_nb_qspa_layered" and sim.num_Frames == B
    words = nb.PN_CodeWords(code, 7, B, first_frame=0)
    rx = nb.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code, words, B)
    w = nb.Decoding_QSPA_host(code, nb.Demodulate(code, rx, sigma).cpu().numpy(), maxIT, layered=True)
    errs = (w["DecodeOutput"] != words.cpu().numpy()).sum(axis=1)
    assert (sim.num_Error_Frames, sim.num_Error_Bits, sim.Total_Iteration) == (int((errs > 0).sum()), int(errs.sum()), int(w["iter_number"].sum()))


# ---- refusals: nothing is launched, the outputs are untouched ---------------------------------------------------------------------------
def refused(nb, code, L, maxIT, match):
    """The raw call on outputs filled with a mark: the return code through Decoding_QSPA's error, and every output word still the mark."""
    import ctypes
    from cuda_ldpc_amd._lib import LdpcError
    before = code.last_kernel
    with pytest.raises(LdpcError, match=match):
        nb.Decoding_QSPA(code, L, maxIT, layered=True)
    B = L.shape[0]
    out = torch.full((B, code.N), -7, dtype=torch.int32, device="cuda")
    its, ok = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = nb.lib.nbldpc_qspa_layered_decode_batch(code._h, P(L), B, maxIT, P(out), P(its), P(ok), None, None,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and code.last_kernel == before and before != "k_nb_qspa_layered"
    assert (out == -7).all() and (its == -7).all() and (ok == -7).all()
    return rc


def test_lds_bound_from_both_sides(nb):
    """The (2, 4) code over GF(64) with 206 columns needs 163 144 bytes: NBLDPC_EUNSUPPORTED; the one with 204 columns (161 600 bytes)
    is decoded (it is in the table: test_kernel_equals_host_statement)."""
    case = LQ.LDS_OVER
    N, M, _, dc, _ = LQ.graph(case)
    assert Q.lds_bytes(N, M, case.q, dc) > Q.LDS_LIMIT
    under = LQ.BY_ID["lds_under"]
    Nu, Mu, _, dcu, _ = LQ.graph(under)
    assert Q.lds_bytes(Nu, Mu, under.q, dcu) <= Q.LDS_LIMIT and N - Nu == 2
    code = dev_code(nb, case)
    L = torch.zeros((2, N, case.q - 1), dtype=torch.float32, device="cuda")
    assert refused(nb, code, L, 4, r"\(-5\).*LDS") == -5
    assert nb.Decoding_QSPA_host(LQ.matrix(nb, case), L.cpu().numpy(), 4, layered=True)["ok"].tolist() == [1, 1], "the host statement has no such bound"
    r = nb.Decoding_QSPA(dev_code(nb, under), dev(LQ.inputs(nb, under)[:2]), LQ.MAX_ITER, layered=True)
    assert_same(r, {k: (None if v is None or k in ("LLR", "L_c2v") else v[:2]) for k, v in LQ.want(nb, under).items()}, "lds_under")


def test_device_refusals(nb):
    """maxIT < 1 is NBLDPC_EINVAL; a code with a zero edge coefficient (the shipped exponent-format GF(64) file) is NBLDPC_EUNSUPPORTED
    on the device and in the host statement alike."""
    from cuda_ldpc_amd._lib import LdpcError
    case = LQ.BY_ID["q64"]
    fresh = nb.NBCode(LQ.files(case)[0], Q.mul_table(case.q))  # a code object no decode call has touched
    assert refused(nb, fresh, dev(LQ.inputs(nb, case)), 0, r"\(-1\)") == -1
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "LDPC_N576_K288_GF64_d1_exp.txt"), mul)
    used = np.arange(code.dc)[None, :] < code.cn_weight[:, None]
    assert (code.cn_linkVNs_GF[used] == 0).any()
    L = np.zeros((1, code.N, 63), np.float32)
    assert refused(nb, code, dev(L), 4, r"\(-5\).*coefficient is 0") == -5
    with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
        nb.Decoding_QSPA_host(code, L, 4, layered=True)
    assert code.last_kernel == "none"


def test_a_row_that_lists_a_variable_twice_is_refused_on_the_device(nb, tmp_path):
    """One row that lists variable 0 in slots 0 and 2 with one coefficient: nbldpc_code_create takes it (first-match cross indices),
    the flooding call decodes it, the layered call is NBLDPC_EUNSUPPORTED like its host statement; nothing is launched."""
    from nb_shape_cases import write_matrix
    from cuda_ldpc_amd._lib import LdpcError
    path = str(tmp_path / "repeat.txt")
    write_matrix(path, 3, 1, 16, 2, 4, [(0, 0, 1), (0, 1, 2), (0, 0, 1), (0, 2, 3)])
    code = nb.NBCode(path, Q.mul_table(16))
    assert code.vn_weight.tolist() == [2, 1, 1] and code.cn_linkVNs[0].tolist() == [0, 1, 0, 2]
    L = torch.full((2, 3, 15), -1.0, dtype=torch.float32, device="cuda")
    assert refused(nb, code, L, 2, r"\(-5\).*two slots") == -5
    with pytest.raises(LdpcError, match=r"\(-5\).*two slots"):
        nb.Decoding_QSPA_host(code, L.cpu().numpy(), 2, layered=True)
    r = nb.Decoding_QSPA(code, L, 2)
    torch.cuda.synchronize()
    assert code.last_kernel == "k_nb_qspa" and r["ok"].shape == (2,)
