"""k_nb_qspa_ws / k_nb_qspa_ws_layered, the workspace tier of the FHT sum-product decoders, against the host statements
nbldpc_qspa_decode_host / nbldpc_qspa_layered_decode_host: DecodeOutput, iter_number, ok, APP and c2v bit for bit.  Every case of
tests/nb_qspa_cases.py (flooding) and tests/nb_qspa_layered_cases.py (layered) under tier="workspace"; the code just over the LDS
bound under "workspace" and "auto"; a GF(256) code with rows of 12 whose plan runs the rows in two passes; one and five workspace
slots for 12 and 300 frames; pinned workgroup sizes; the two shipped matrices the LDS tier refuses; B = 1, no state outputs, a
rate-matched input; the refusals; and the simulation loop.  tests/test_nb_qspa_ws_cpu.py asserts that the inputs are worth decoding.
The codes and texts of the refusals of all three decode calls, and which one wins where two apply, are pinned by
tests/golden/nb_qspa_refusals.json; `python tests/test_nb_qspa_ws_gpu.py --record FILE` writes that file from the library it runs on."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import nb_qspa_cases as Q
import nb_qspa_layered_cases as LQ
import nb_qspa_ws_cases as W

pytestmark = pytest.mark.gpu
KERNEL = {False: "k_nb_qspa_ws", True: "k_nb_qspa_ws_layered"}
SWITCHES = ("NBLDPC_QSPA_WS_SLOTS", "NBLDPC_QSPA_WS_THREADS")


@pytest.fixture(scope="module")
def nb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cuda_ldpc_amd import nbldpc
    return nbldpc


_CODES = {}


def new_code(nb, path, mul, **switches):
    """A code object created under the given experiment switches (read once at nbldpc_code_create), the environment restored."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        for k, v in switches.items():
            os.environ[k] = str(v)
        return nb.NBCode(path, mul)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def dev_code(nb, cid, layered, **switches):
    key = (cid, layered, tuple(sorted(switches.items())))
    if key not in _CODES:
        mod, case = W.mod_of(layered), W.case_of(cid, layered)
        _CODES[key] = new_code(nb, mod.files(case)[0], Q.mul_table(case.q), **switches)
    return _CODES[key]


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


def no_state(w):
    return dict(w, LLR=None, L_c2v=None)


def pick(w, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in w.items()}


def run_case(nb, cid, layered, maxIT=W.MAX_ITER, tier="workspace", want_state=True, **switches):
    mod, case = W.mod_of(layered), W.case_of(cid, layered)
    code = dev_code(nb, cid, layered, **switches)
    r = nb.Decoding_QSPA(code, dev(mod.inputs(nb, case)), maxIT, want_state=want_state, layered=layered, tier=tier)
    w = mod.want(nb, case, maxIT)
    assert_same(r, w if want_state else no_state(w), (cid, layered, maxIT, tier, switches))
    return code, r


# ---- the existing cases, the new tier ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", Q.IDS)
def test_flooding_cases(nb, cid):
    code, _ = run_case(nb, cid, False)
    assert code.last_kernel == "k_nb_qspa_ws"
    _, r = run_case(nb, cid, False, want_state=False)
    assert r["LLR"] is None and r["L_c2v"] is None


@pytest.mark.parametrize("cid", LQ.IDS)
def test_layered_cases(nb, cid):
    code, _ = run_case(nb, cid, True)
    assert code.last_kernel == "k_nb_qspa_ws_layered"
    _, r = run_case(nb, cid, True, want_state=False)
    assert r["LLR"] is None and r["L_c2v"] is None


# ---- over the bound ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layered", [False, True])
def test_over_the_lds_bound(nb, layered):
    from cuda_ldpc_amd._lib import LdpcError
    N, M, q, _, dc = W.dims("lds_over", layered)
    assert Q.lds_bytes(N, M, q, dc) > Q.LDS_LIMIT
    for tier in ("workspace", "auto"):
        code, _ = run_case(nb, "lds_over", layered, tier=tier)
        assert code.last_kernel == KERNEL[layered], tier
    with pytest.raises(LdpcError, match=r"\(-5\).*LDS"):  # the LDS call still refuses it, and "lds" is the default
        nb.Decoding_QSPA(code, dev(W.mod_of(layered).inputs(nb, W.case_of("lds_over", layered))), 4, layered=layered)
    assert code.last_kernel == KERNEL[layered]
    code, _ = run_case(nb, "lds_under", layered, tier="auto")
    assert code.last_kernel == ("k_nb_qspa_layered" if layered else "k_nb_qspa")
    info = code.qspa_ws_info(layered)
    assert info == nb.QSPA_WS_Plan_host(*[W.dims("lds_under", layered)[i] for i in (0, 1, 2, 4)], widest_level=W.widest_level("lds_under"), layered=layered)
    with pytest.raises(ValueError, match="tier"):
        nb.Decoding_QSPA(code, dev(np.zeros((1, 204, 63), np.float32)), 4, tier="hbm")


# ---- q = 256 with rows of 12: 256 threads, four row slabs for eight rows ------------------------------------------------------------
@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("maxIT", [1, 8])
def test_q256_dc12(nb, layered, maxIT):
    code, _ = run_case(nb, "q256_dc12", layered, maxIT=maxIT)
    assert code.last_kernel == KERNEL[layered]
    info = code.qspa_ws_info(layered)
    N, M, q, _, dc = W.dims("q256_dc12", layered)
    assert info == W.plan(N, M, q, dc, W.widest_level("q256_dc12"), layered)
    if layered:  # the smallest size that holds the widest level: fewer slabs than the flooding plan's, one pass per level
        assert W.widest_level("q256_dc12") <= info["vectors"] <= 4 and len(LQ.level_widths(W.layered_case("q256_dc12"))) > 1
        run_case(nb, "q256_dc12", True, maxIT=maxIT, NBLDPC_QSPA_WS_THREADS=64)  # one slab: the level of two rows in two passes
    else:
        assert info["threads"] == 256 and info["vectors"] == 4 < code.M == 8 and info["lds_bytes"] == 4 * 52 + 65536 + 4 * 12288


# ---- a slot serves several frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("slots", [1, 5])
def test_slot_reuse(nb, layered, slots):
    cid = "q16_part"
    run_case(nb, cid, layered, NBLDPC_QSPA_WS_SLOTS=slots)  # the case's 12 frames, three or more different iteration counts
    mod, case = W.mod_of(layered), W.case_of(cid, layered)
    L, w = mod.inputs(nb, case), mod.want(nb, case)
    idx = (np.arange(300) * 5 + 1) % L.shape[0]
    code = dev_code(nb, cid, layered, NBLDPC_QSPA_WS_SLOTS=slots)
    assert code.qspa_ws_slots(12, layered) == slots == code.qspa_ws_slots(300, layered), "the cap took effect: 12 and 300 frames share them"
    free = dev_code(nb, cid, layered)
    assert [free.qspa_ws_slots(B, layered) for B in (1, 12, 300, 5000)] == [1, 12, 300, 1024]
    r = nb.Decoding_QSPA(code, dev(L[idx]), W.MAX_ITER, want_state=True, layered=layered, tier="workspace")
    assert_same(r, pick(w, idx), (cid, layered, slots, 300))


# ---- pinned workgroup sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("cid", ["q16_part", "q64_dv3"])
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_results_do_not_depend_on_the_workgroup_size(nb, cid, layered, threads):
    code, _ = run_case(nb, cid, layered, NBLDPC_QSPA_WS_THREADS=threads)
    assert code.qspa_ws_info(layered)["threads"] == threads and code.last_kernel == KERNEL[layered]


def test_a_pin_that_does_not_fit_is_refused(nb):
    """q256_dc12 under 512 threads would need 65 744 + 8 * 12 288 = 164 048 bytes of LDS."""
    from cuda_ldpc_amd._lib import LdpcError
    code = dev_code(nb, "q256_dc12", False, NBLDPC_QSPA_WS_THREADS=512)
    L = dev(Q.inputs(nb, W.Q256_DC12)[:2])
    assert raw_refusal(nb, code, L, 0, 4) == -5
    with pytest.raises(LdpcError, match=r"\(-5\).*pinned"):
        nb.Decoding_QSPA(code, L, 4, tier="workspace")
    with pytest.raises(LdpcError, match=r"\(-5\).*pinned"):
        code.qspa_ws_info()


# ---- the shipped matrices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("sid", sorted(W.SHIPPED))
def test_shipped_matrices(nb, sid, layered):
    from cuda_ldpc_amd._lib import LdpcError
    s = W.SHIPPED[sid]
    key = ("shipped", sid)
    if key not in _CODES:
        _CODES[key] = new_code(nb, W.shipped_path(s), W.shipped_mul(nb, s))
    code, L = _CODES[key], dev(W.shipped_inputs(nb, s))
    with pytest.raises(LdpcError, match=r"\(-5\).*LDS"):
        nb.Decoding_QSPA(code, L, s.maxIT, layered=layered)
    r = nb.Decoding_QSPA(code, L, s.maxIT, want_state=True, layered=layered, tier="auto")
    assert code.last_kernel == KERNEL[layered]
    assert_same(r, W.shipped_want(nb, s, layered), (sid, layered))


# ---- batch and options ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layered", [False, True])
def test_batch_of_one(nb, layered):
    cid = "q64_dv3"
    mod, case = W.mod_of(layered), W.case_of(cid, layered)
    L, w = mod.inputs(nb, case), mod.want(nb, case)
    for b in (0, 7):
        r = nb.Decoding_QSPA(dev_code(nb, cid, layered), dev(L[b:b + 1]), W.MAX_ITER, want_state=True, layered=layered, tier="workspace")
        assert_same(r, pick(w, slice(b, b + 1)), (cid, layered, b))


@pytest.mark.parametrize("layered", [False, True])
def test_rate_matched_input(nb, layered):
    """Two shortened and four punctured symbols through nbldpc_rm_demodulate_bpsk_recover: -1e4 and +0.0 vectors among the noisy ones."""
    import cuda_ldpc_amd as C
    mod, case = W.mod_of(layered), W.case_of("q64", layered)
    code = dev_code(nb, "q64", layered)
    rm = C.RateMatch(code.N, [0, 5], range(20, 24))
    words = torch.zeros((6, code.N), dtype=torch.int32, device="cuda")
    rx = nb.AWGNChannel_RM_GPU(np.array([173, 173, 173], np.int32), 0.7, rm, case.q, nb.RM_Select(rm, words))
    L = nb.RM_Demodulate_Recover(rm, case.q, rx, 0.7)
    Lh = L.cpu().numpy()
    assert (Lh[:, [0, 5]] == -1e4).all() and (Lh[:, 20:] == 0).all()
    w = nb.Decoding_QSPA_host(mod.matrix(nb, case), Lh, W.MAX_ITER, want_state=True, layered=layered)
    assert_same(nb.Decoding_QSPA(code, L, W.MAX_ITER, want_state=True, layered=layered, tier="workspace"), w, "rate matched")
    assert (w["DecodeOutput"][:, [0, 5]] == 0).all() and np.isfinite(w["LLR"]).all()


# ---- refusals: nothing is launched, the outputs are untouched, last_kernel is unchanged --------------------------------------------------
def raw_refusal(nb, code, L, layered, maxIT):
    """The raw call on outputs filled with a mark: the return code, and every output word still the mark."""
    before = code.last_kernel
    B = L.shape[0]
    mark = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")  # noqa: E731
    out, its, ok = mark(B, code.N), mark(B), mark(B)
    APP = torch.full((B, code.N, code.q), -7.0, dtype=torch.float32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = nb.lib.nbldpc_qspa_ws_decode_batch(code._h, P(L), B, layered, maxIT, P(out), P(its), P(ok), P(APP), None,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and code.last_kernel == before
    assert (out == -7).all() and (its == -7).all() and (ok == -7).all() and (APP == -7.0).all()
    return rc


def test_refusals(nb, tmp_path):
    from nb_shape_cases import write_matrix
    from cuda_ldpc_amd._lib import LdpcError
    NB = W.NB
    mul, _, _ = nb.GFInitial(64, os.path.join(NB, "GF", "Arith.Table.GF.64.txt"))
    code = nb.NBCode(os.path.join(NB, "LDPC_N576_K288_GF64_d1_exp.txt"), mul)
    used = np.arange(code.dc)[None, :] < code.cn_weight[:, None]
    assert (code.cn_linkVNs_GF[used] == 0).any()
    L = dev(np.zeros((2, code.N, 63), np.float32))
    for layered in (0, 1):
        assert raw_refusal(nb, code, L, layered, 4) == -5
        with pytest.raises(LdpcError, match=r"\(-5\).*coefficient is 0"):
            nb.Decoding_QSPA(code, L, 4, layered=bool(layered), tier="workspace")
    assert code.last_kernel == "none"
    # a row that lists variable 0 in slots 0 and 2: the flooding schedule decodes it, the layered one refuses it
    path = str(tmp_path / "repeat.txt")
    write_matrix(path, 3, 1, 16, 2, 4, [(0, 0, 1), (0, 1, 2), (0, 0, 1), (0, 2, 3)])
    code = nb.NBCode(path, Q.mul_table(16))
    L = torch.full((2, 3, 15), -1.0, dtype=torch.float32, device="cuda")
    assert raw_refusal(nb, code, L, 1, 2) == -5
    with pytest.raises(LdpcError, match=r"\(-5\).*two slots"):
        nb.Decoding_QSPA(code, L, 2, layered=True, tier="workspace")
    assert code.last_kernel == "none"
    m = nb.NBMatrix(path)
    m.TableMultiply = Q.mul_table(16)
    r = nb.Decoding_QSPA(code, L, 2, want_state=True, tier="workspace")
    assert_same(r, nb.Decoding_QSPA_host(m, L.cpu().numpy(), 2, want_state=True), "repeat, flooding")
    assert code.last_kernel == "k_nb_qspa_ws"
    assert raw_refusal(nb, code, L, 0, 0) == -1  # maxIT < 1
    assert code.last_kernel == "k_nb_qspa_ws"


# ---- every refusal's code and text, and which one wins: as recorded in tests/golden/nb_qspa_refusals.json ---------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nb_qspa_refusals.json")
CALLS = {"lds": ("nbldpc_qspa_decode_batch", None), "lds_layered": ("nbldpc_qspa_layered_decode_batch", None),
         "ws": ("nbldpc_qspa_ws_decode_batch", 0), "ws_layered": ("nbldpc_qspa_ws_decode_batch", 1)}


def refusals(nb, tmp):
    """{"case/call": [return code, nbldpc_last_error text]} of the refused calls; last_kernel is unchanged after each."""
    from nb_shape_cases import write_matrix
    got = {}

    def refuse(case, code, calls, B=2, maxIT=4):
        L = torch.zeros((2, code.N, code.q - 1), dtype=torch.float32, device="cuda")
        out = torch.zeros((2, code.N), dtype=torch.int32, device="cuda")
        its, ok = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        for call in calls:
            before = code.last_kernel
            name, layered = CALLS[call]
            args = (code._h, P(L), B) + (() if layered is None else (layered,)) + (maxIT, P(out), P(its), P(ok), None, None, None)
            rc = getattr(nb.lib, name)(*args)
            got["%s/%s" % (case, call)] = [rc, nb.lib.nbldpc_last_error().decode()]
            assert rc != 0 and code.last_kernel == before, (case, call, rc, code.last_kernel)

    def written(name, N, M, q, dv, dc, edges):
        path = os.path.join(tmp, name + ".txt")
        write_matrix(path, N, M, q, dv, dc, edges)
        return nb.NBCode(path, Q.mul_table(q))

    refuse("lds_over", dev_code(nb, "lds_over", False), ("lds", "lds_layered"))
    mul, _, _ = nb.GFInitial(64, os.path.join(W.NB, "GF", "Arith.Table.GF.64.txt"))
    refuse("zero_coefficient", nb.NBCode(os.path.join(W.NB, "LDPC_N576_K288_GF64_d1_exp.txt"), mul), CALLS)
    repeat = written("repeat", 3, 1, 16, 2, 4, [(0, 0, 1), (0, 1, 2), (0, 0, 1), (0, 2, 3)])
    refuse("repeated_variable", repeat, ("lds_layered", "ws_layered"))
    small = dev_code(nb, "q16_part", False)
    refuse("B_0", small, CALLS, B=0)
    refuse("maxIT_0", small, CALLS, maxIT=0)
    refuse("pin_too_large", dev_code(nb, "q256_dc12", False, NBLDPC_QSPA_WS_THREADS=512), ("ws", "ws_layered"))
    # two refusals at once: the zero coefficient is named, not the LDS bound
    M, edges = Q.graph(Q.LDS_OVER)
    r0, c0, _ = edges[0]
    over = Q.LDS_OVER
    refuse("lds_over_and_zero_coefficient", written("over_zero", over.N, M, over.q, over.dv, over.dc, [(r0, c0, 0)] + list(edges[1:])),
           ("lds", "lds_layered"))
    return got


def test_refusal_codes_and_texts_are_those_recorded(nb, tmp_path):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = refusals(nb, str(tmp_path))
    assert sorted(got) == sorted(golden["cases"])
    for key in sorted(got):
        assert got[key] == golden["cases"][key], key


# ---- the simulation loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [4, 5])
def test_simulation_counts_what_the_host_statement_decodes(nb, method):
    """Simulation_GPU(decoder_method=4 | 5, qspa_tier="auto") on the code over the LDS bound, the all-zero word over the device
    channel: the counters of the same 256 frames decoded by the host statement."""
    from cuda_ldpc_amd import nb_simulation as S
    from cuda_ldpc_amd._lib import LdpcError
    layered = method == 5
    code = dev_code(nb, "lds_over", layered)
    sigma, B, maxIT = nb.sigma_of(2.0, code.rate), 256, 6
    cw = np.zeros(code.N, np.int32)
    sim = S.NBSim(2.0)
    S.Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, sim, cw, maxIT=maxIT, batch=B, leastErrorFrames=10 ** 6, max_frames=B,
                     device_channel=True, decoder_method=method, qspa_tier="auto")
    assert code.last_kernel == KERNEL[layered] and sim.num_Frames == B
    rx = nb.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code, torch.from_numpy(cw).cuda(), B)
    m = W.mod_of(layered).matrix(nb, W.case_of("lds_over", layered))
    w = nb.Decoding_QSPA_host(m, nb.Demodulate(code, rx, sigma).cpu().numpy(), maxIT, layered=layered)
    errs = (w["DecodeOutput"] != cw[None, :]).sum(axis=1)
    assert len(set(w["iter_number"].tolist())) >= 3
    assert (sim.num_Error_Frames, sim.num_Error_Bits, sim.Total_Iteration) == (int((errs > 0).sum()), int(errs.sum()), int(w["iter_number"].sum()))
    with pytest.raises(LdpcError, match=r"\(-5\).*LDS"):  # the default tier is today's call
        S.Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, S.NBSim(2.0), cw, maxIT=maxIT, batch=8, max_frames=8,
                         device_channel=True, decoder_method=method)


if __name__ == "__main__":  # --record FILE COMMIT: the refusals of the library this runs on (built from COMMIT), in the golden file's form
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cuda_ldpc_amd import nbldpc
    at = sys.argv.index("--record")
    with tempfile.TemporaryDirectory() as tmp, open(sys.argv[at + 1], "w") as f:
        json.dump({"recorded": "by `python tests/test_nb_qspa_ws_gpu.py --record FILE COMMIT`, this file copied into a built checkout of "
                               "COMMIT = " + sys.argv[at + 2], "cases": refusals(nbldpc, tmp)}, f, indent=1)
        f.write("\n")
