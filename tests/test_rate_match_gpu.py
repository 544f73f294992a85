"""Shortened and punctured binary codes on the GPU (bldpc_rm_*): the three data movements against their host statements and against
each other, bit for bit; every decoder tier on inputs that hold exact zeros and a 1.0e4 next to values near 1, against the CPU oracle
and the host statements of the normalised and the layered decoder; random codewords with shortened bits; Simulation_GPU(rate_match=...)
against the same batches composed from the primitive calls."""
import ctypes
import os

import numpy as np
import pytest
import torch

import qc_variant_cases as Q
from conftest import DATA

pytestmark = pytest.mark.gpu

N0 = 2304  # J4_L24_Z96
SHORT_LLR = 1.0e4


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def ibits(t):
    return t.contiguous().view(torch.int32)


def nbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# none, shorten only, puncture only, both, the last position punctured; lists unsorted, a range that crosses a row tile of 32
PROFILES = {
    "none": ((), ()),
    "shorten": ([700, 3, 0, 1, 2] + list(range(1000, 1040)), ()),
    "puncture": ((), list(range(2100, 2170)) + [17]),
    "both": (list(range(0, 24)) + [999], list(range(2188, 2260)) + [392]),
    "last-punctured": ([0], [N0 - 1, N0 - 2, 31, 32]),
}


@pytest.mark.parametrize("F", [1, 63, 257])  # 257: a full block of 256 frames and a ragged one of 1
@pytest.mark.parametrize("name", list(PROFILES))
def test_select_and_recover_equal_their_host_statements(C, name, F):
    rm = C.RateMatch(N0, *PROFILES[name])
    g = torch.Generator(device="cuda").manual_seed(F)
    cw = torch.randint(0, 2 ** 31 - 1, (N0, F), generator=g, device="cuda", dtype=torch.int32)
    tx = C.RM_Select(rm, cw)
    assert tx.shape == (rm.E, F) and np.array_equal(tx.cpu().numpy(), C.RM_Select_host(rm, cw.cpu().numpy()))
    rx = torch.randn((rm.E, F), generator=g, device="cuda")
    rx.view(-1)[:3] = torch.tensor([-0.0, float("inf"), 1e-42], device="cuda")[:rx.numel()]
    got = C.RM_Recover(rm, rx, SHORT_LLR)
    torch.cuda.synchronize()
    want = C.RM_Recover_host(rm, rx.cpu().numpy(), SHORT_LLR)
    assert got.shape == (N0, F) and np.array_equal(nbits(got.cpu().numpy()), nbits(want))
    if rm.n_punct:
        assert not ibits(got)[torch.from_numpy(rm.puncture).long().cuda()].any(), "punctured rows are 0x00000000"


# E = 2304 - 9 - 58 = 2237 is no multiple of 32.  Punctured: 40..49 starts and ends inside the run 32..63; 60..99 starts inside that
# run, removes the whole run 64..95 and ends inside 96..127; the last position.  Shortened: the head of the first run and a position
# between two punctured ranges.
CH_SHORT = list(range(0, 8)) + [55]
CH_PUNCT = list(range(40, 50)) + list(range(60, 100)) + list(range(1200, 1207)) + [N0 - 1]


@pytest.mark.parametrize("F", [1, 257])
@pytest.mark.parametrize("profile", ["mixed", "none"])
def test_fused_channel_equals_select_channel_recover(C, profile, F):
    from cuda_ldpc_amd import sharding
    rm = C.RateMatch(N0, CH_SHORT, CH_PUNCT) if profile == "mixed" else C.RateMatch(N0)
    assert profile == "none" or (rm.E == 2237 and rm.E % 32)
    g = torch.Generator(device="cuda").manual_seed(10 + F)
    cw = torch.randint(0, 2, (N0, F), generator=g, device="cuda", dtype=torch.int32)
    cw[torch.tensor(CH_SHORT, device="cuda")] = 0
    start, sigma = [173, 40001, 63598], 0.73
    for word in (cw, None):
        seed, seed_ref = np.array(start, np.int32), np.array(start, np.int32)
        for call in range(2):  # the second call continues from the advanced seed
            got = C.AWGNChannel_RM_GPU(rm, seed, sigma, F, CodeWord=word, short_llr=SHORT_LLR)
            rx = C.AWGNChannel_GPU(seed_ref, sigma, rm.E, F, CodeWord=None if word is None else C.RM_Select(rm, word))
            want = C.RM_Recover(rm, rx, SHORT_LLR)
            torch.cuda.synchronize()
            assert torch.equal(ibits(got), ibits(want)), "call %d, %s" % (call, "codeword" if word is not None else "zero word")
            assert np.array_equal(seed, seed_ref) and np.array_equal(seed, sharding.lcg_jump(start, 2 * rm.E * F * (call + 1)))
        if profile == "none":  # the identity profile is the plain channel at N
            s = np.array(start, np.int32)
            C.AWGNChannel_GPU(s, sigma, N0, F)
            assert torch.equal(ibits(got), ibits(C.AWGNChannel_GPU(s, sigma, N0, F, CodeWord=word)))


def test_kernels_write_inside_their_outputs(C):
    """Guard words around the outputs of all three kernels stay as set (F = 257: a ragged frame block; E and N no multiple of the row tile)."""
    from cuda_ldpc_amd._lib import check, lib
    rm = C.RateMatch(N0 - 3, CH_SHORT, CH_PUNCT[:-1])
    N, E, F, G = rm.N, rm.E, 257, 64
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cw = torch.ones((N, F), dtype=torch.int32, device="cuda")
    tx = torch.full((E * F + 2 * G,), -7, dtype=torch.int32, device="cuda")
    check(lib.bldpc_rm_select(rm._h, P(cw), F, P(tx[G:]), st), "select")
    assert (tx[:G] == -7).all() and (tx[G + E * F:] == -7).all() and (tx[G:G + E * F] == 1).all()
    rx = torch.full((E, F), 2.5, device="cuda")
    for fill in ("recover", "channel"):
        y = torch.full((N * F + 2 * G,), 123.0, device="cuda")
        if fill == "recover":
            check(lib.bldpc_rm_recover(rm._h, P(rx), F, ctypes.c_float(SHORT_LLR), P(y[G:]), st), fill)
        else:
            seed = np.array([173, 173, 173], np.int32)
            check(lib.bldpc_rm_awgn_channel_device(rm._h, seed.ctypes.data_as(ctypes.c_void_p), ctypes.c_float(0.0), None, F, ctypes.c_float(SHORT_LLR),
                                                   P(y[G:]), st), fill)
        torch.cuda.synchronize()
        body = y[G:G + N * F].reshape(N, F)
        assert (y[:G] == 123.0).all() and (y[G + N * F:] == 123.0).all(), fill
        assert (body[torch.from_numpy(rm.tx_pos).long().cuda()] == (2.5 if fill == "recover" else 1.0)).all(), fill  # sigma 0: y = 1 - 2c exactly
        assert (body[torch.from_numpy(rm.shorten).long().cuda()] == SHORT_LLR).all() and not body[torch.from_numpy(rm.puncture).long().cuda()].any()


def test_device_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    rm = C.RateMatch(N0, [0], [1])
    rx = torch.ones((rm.E, 2), device="cuda")
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="short_llr"):
            C.RM_Recover(rm, rx, bad)
        with pytest.raises(ValueError, match="short_llr"):
            C.AWGNChannel_RM_GPU(rm, np.array([173, 173, 173], np.int32), 0.7, 2, short_llr=bad)
    from cuda_ldpc_amd._lib import lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = torch.empty((N0, 2), device="cuda")
    seed = np.array([173, 173, 173], np.int32)
    sp = seed.ctypes.data_as(ctypes.c_void_p)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.bldpc_rm_recover(rm._h, P(rx), 2, ctypes.c_float(float("inf")), P(y), st) == -1 and b"short_llr" in lib.bldpc_last_error()
    assert lib.bldpc_rm_awgn_channel_device(rm._h, sp, ctypes.c_float(0.7), None, 2, ctypes.c_float(0.0), P(y), st) == -1
    assert lib.bldpc_rm_awgn_channel_device(rm._h, sp, ctypes.c_float(0.7), None, 0, ctypes.c_float(1.0), P(y), st) == -1
    assert lib.bldpc_rm_awgn_channel_device(None, sp, ctypes.c_float(0.7), None, 2, ctypes.c_float(1.0), P(y), st) == -1
    assert lib.bldpc_rm_select(rm._h, None, 2, P(y), st) == -1 and lib.bldpc_rm_recover(rm._h, P(rx), 2, ctypes.c_float(1.0), None, st) == -1
    bad_seed = np.array([173, 173, 63599], np.int32)
    with pytest.raises(LdpcError, match="seed"):
        C.AWGNChannel_RM_GPU(rm, bad_seed, 0.7, 2)
    with pytest.raises(ValueError):
        C.RM_Recover(rm, rx[:-1].contiguous())
    with pytest.raises(ValueError):
        C.RM_Select(rm, torch.zeros((N0 + 1, 2), dtype=torch.int32, device="cuda"))


# ---- the decoders on rate-matched inputs ---------------------------------------------------------------------------------------
# (matrix, the tag of the fused tier it runs on, shortened, punctured).  PON: the issue's profile.  The others: about 1 % of the
# positions shortened at the head of the information part and about 3 % punctured in the parity part, across a block boundary.
def _generic(name):
    J, L, Z = Q.SHIPPED[name]
    N = L * Z
    end = N - Z + Z // 4  # inside the last block column; the range of N / 32 positions before it crosses at least one block boundary
    return range(0, max(8, N // 100)), range(end - N // 32, end)


TIERS = [
    ("J4_L24_Z96", "halfrow-local") + _generic("J4_L24_Z96"),
    ("J32_L64_Z64", "row-local") + _generic("J32_L64_Z64"),
    ("J10_L60_Z160", "compressed") + _generic("J10_L60_Z160"),
    ("PON_LDPC", "regstate", range(0, 200), range(69 * 256 - 512, 69 * 256)),
    ("J4_L24_Z512", "regstate-halo") + _generic("J4_L24_Z512"),
]
F_DEC, ITS_FIXED, MAXIT_PF, MAXIT_LAY, ALPHA = 8, 10, 40, 25, 0.75
# Es/N0 where that of qc_variant_cases.SNR leaves no frame of the punctured code converging (host statements, host channel: at 2.5 dB
# every frame of PON runs all 40 iterations)
SNR_RM = {"PON_LDPC": 3.6}

_inputs = {}


def _tier_input(C, name, sh, pu):
    """(code, y on the device, y on the host, rm): eight frames of the all-zero word through the fused channel at the matrix's Es/N0 of
    qc_variant_cases.py.  The host references read the same bits the kernels read."""
    if name not in _inputs:
        spec = ("shipped", name)
        path, _, J, L, Z = Q.matrix(spec)
        code = C.BinaryCode.from_blockh(path, J, L, Z)
        rm = C.RateMatch(code.N, sh, pu)
        y = C.AWGNChannel_RM_GPU(rm, np.array([173, 173, 173], np.int32), C.sigma_of(SNR_RM.get(name, Q.SNR[spec])), F_DEC, short_llr=SHORT_LLR)
        torch.cuda.synchronize()
        _inputs[name] = (code, y, y.cpu().numpy(), rm)
    return _inputs[name]


def _got(r):
    torch.cuda.synchronize()
    return r["D"].cpu().numpy(), r["app"].cpu().numpy(), None if r.get("iters") is None else r["iters"].cpu().numpy()


def _same(got, D, app, iters, what):
    gD, gapp, git = got
    assert np.array_equal(gD[:-1], np.asarray(D).reshape(gD.shape)[:-1]), what + ": hard bits differ"
    assert np.array_equal(gD[-1], np.asarray(D).reshape(gD.shape)[-1]), what + ": flag row differs"
    assert np.array_equal(nbits(gapp), nbits(np.asarray(app).reshape(gapp.shape))), what + ": a-posteriori sums differ bitwise"
    if iters is not None:
        assert np.array_equal(git, iters), what + ": iteration counts %s, expected %s" % (git, iters)


@pytest.mark.parametrize("name,tag,sh,pu", TIERS, ids=[t[0] for t in TIERS])
def test_flooding_decoders_equal_the_oracle(C, orc, name, tag, sh, pu):
    code, yt, y, rm = _tier_input(C, name, sh, pu)
    assert C.qc_variants()[code.qc_variant]["tag"] == tag
    assert not nbits(y)[rm.puncture].any() and (y[rm.shorten] == np.float32(SHORT_LLR)).all()
    oc = Q.ocode(orc, ("shipped", name))
    w = orc.bldpc_decode(oc, y, F_DEC, ITS_FIXED, early_exit=0, want_app=True)
    r = C.LDPC_Decoder_GPU(code, yt, max_iter=ITS_FIXED, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, want_app=True)
    _same(_got(r), w["D"], w["app"], None, name + " fixed")
    assert not np.isnan(w["app"]).any() and not w["D"].reshape(code.N + 1, F_DEC)[rm.shorten].any()
    Dw, appw, itw = Q.oracle_per_frame(orc, oc, y, F_DEC, MAXIT_PF)
    r = C.LDPC_Decoder_GPU(code, yt, max_iter=MAXIT_PF, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, want_app=True)
    _same(_got(r), Dw, appw, itw, name + " per-frame")


@pytest.mark.parametrize("name,tag,sh,pu", TIERS, ids=[t[0] for t in TIERS])
def test_normalised_decoders_equal_the_host_statement(C, name, tag, sh, pu):
    code, yt, y, rm = _tier_input(C, name, sh, pu)
    _, H, J, L, Z = Q.matrix(("shipped", name))
    w = C.normalised_host(H, J, L, Z, y, max_iter=ITS_FIXED, alpha=ALPHA)
    r = C.LDPC_Decoder_GPU(code, yt, max_iter=ITS_FIXED, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, want_app=True, alpha=ALPHA)
    assert code.last_kernel.endswith("_norm")
    _same(_got(r), w["D"], w["app"], None, name + " fixed")
    w = C.normalised_host(H, J, L, Z, y, max_iter=MAXIT_PF, alpha=ALPHA, exit_mode=C.EXIT_PER_FRAME)
    r = C.LDPC_Decoder_GPU(code, yt, max_iter=MAXIT_PF, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, want_app=True, alpha=ALPHA)
    _same(_got(r), w["D"], w["app"], w["iters"], name + " per-frame")


@pytest.mark.parametrize("name,tag,sh,pu", TIERS, ids=[t[0] for t in TIERS])
def test_layered_decoder_equals_the_host_statement(C, name, tag, sh, pu):
    code, yt, y, rm = _tier_input(C, name, sh, pu)
    _, H, J, L, Z = Q.matrix(("shipped", name))
    for exit_mode, its in ((C.EXIT_FIXED, ITS_FIXED), (C.EXIT_PER_FRAME, MAXIT_LAY)):
        w = C.layered_host(H, J, L, Z, y, max_iter=its, alpha=ALPHA, exit_mode=exit_mode, stop_rule=C.STOP_SYNDROME)
        r = C.LDPC_Decoder_Layered_GPU(code, yt, max_iter=its, alpha=ALPHA, exit_mode=exit_mode, stop_rule=C.STOP_SYNDROME, want_app=True)
        _same(_got(r), w["D"], w["app"], w["iters"], "%s exit_mode %d" % (name, exit_mode))


# ---- random codewords with shortened bits --------------------------------------------------------------------------------------
def test_pn_codewords_with_shortened_bits(C):
    from cuda_ldpc_amd._lib import LdpcError
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    info = code.info_positions
    sh = np.r_[info[:24], info[100], info[-1]]
    rm = C.RateMatch(code.N, sh, range(2188, 2260))
    F, pn_seed = 160, 777
    cw, msg = C.PN_CodeWords(code, pn_seed, F, want_msg=True, rate_match=rm)
    assert not cw[torch.from_numpy(rm.shorten).long().cuda()].any(), "shortened rows are all zero"
    assert bool((C.Syndrome(code, cw, into_flag_row=False)["flag"] == 1).all()), "every frame is a codeword"
    want = C.pn_messages(pn_seed, code.K_info, F)
    want[np.isin(info, rm.shorten)] = 0
    assert np.array_equal(msg.cpu().numpy(), want) and np.array_equal(cw.cpu().numpy()[info], want)
    assert want.any(axis=1).sum() == code.K_info - rm.n_short, "every other message bit is random"
    plain = C.PN_CodeWords(code, pn_seed, F)
    assert not torch.equal(plain, cw) and torch.equal(C.PN_CodeWords(code, pn_seed, F, rate_match=C.RateMatch(code.N, (), [5])), plain)
    alone = C.PN_CodeWords(code, pn_seed, 32, first_frame=100, rate_match=rm)
    assert torch.equal(alone, cw[:, 100:132]), "frames 100..131 drawn on their own"
    parity = np.setdiff1d(np.arange(code.N), info)
    with pytest.raises(LdpcError, match="parity position"):
        C.PN_CodeWords(code, pn_seed, F, rate_match=C.RateMatch(code.N, [0, int(parity[3])]))
    with pytest.raises(ValueError):
        C.PN_CodeWords(code, pn_seed, F, rate_match=C.RateMatch(code.N + 1, [0]))


# ---- Simulation_GPU(rate_match=...) --------------------------------------------------------------------------------------------
class _Rank:
    """One rank of a world of `world` without a process group (as in test_modem_gpu.py): the all-reduce is the sum the test makes."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def is_initialized(self):
        return True

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def all_reduce(self, t):
        return t


# About 3 % of the bits punctured moves the waterfall of J4_L24_Z96 up by some 0.4 dB: with the host statements on the host channel,
# 512 frames lose 155 (flooding, 20 iterations, Es/N0 3.0 dB) and 174 (layered, alpha 0.75, 2.7 dB).
SIM_SHORT, SIM_PUNCT = range(0, 24), range(2188, 2260)


def _counts(D, cw, iters, K):
    """The five counters of Statistic from host arrays (flag row: what the decoder or Syndrome left there)."""
    errs = (D[:K] != cw[:K]).sum(0)
    ok = D[-1] != 0
    return np.array([np.sum((errs != 0) | ~ok), errs.sum(), np.sum(iters), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)], np.int64)


@pytest.mark.parametrize("mode", ["flooding-fixed-zero", "layered-per-frame-pn", "qam64"])
def test_simulation_equals_a_loop_of_the_primitives(C, mode):
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd.simulation import Simulation_GPU
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    rm = C.RateMatch(code.N, SIM_SHORT, SIM_PUNCT)
    F, batches, pn_seed, q, m = 512, 2, 31337, 64, 6
    N, K, E = code.N, code.K, rm.E
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, device_channel=True, rate_match=rm, short_llr=SHORT_LLR, leastTestFrames=10 ** 9)
    con = cond = None
    if mode == "flooding-fixed-zero":
        sigma, maxIT = C.sigma_of(3.0), 20
        kw.update(maxIT=maxIT, exit_mode=C.EXIT_FIXED)
    elif mode == "layered-per-frame-pn":
        sigma, maxIT = C.sigma_of(2.7), 25
        kw.update(maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, PN_Message=1, pn_seed=pn_seed, schedule="layered", alpha=ALPHA)
    else:
        con = C.Get_CONSTELLATION(os.path.join(DATA, "nb", "Constellation", "GRAY_64QAM.txt"), q)
        cond = torch.from_numpy(con).cuda()
        sigma, maxIT = nb.sigma_of(10.5, rm.rate(K), 0, q), 25
        kw.update(maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, PN_Message=1, pn_seed=pn_seed, schedule="layered", alpha=ALPHA, n_QAM=q, CONSTELLATION=con)

    def run(dist):
        SIM, seed = C.SimCounters(), np.array([173, 173, 173], np.int32)
        Simulation_GPU(code, seed, sigma, SIM, dist=dist, **kw)
        assert SIM.num_Frames == F * batches
        return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames], seed

    got, got_seed = run(None)
    seed = np.array([173, 173, 173], np.int32)
    tot = np.zeros(5, np.int64)
    for b in range(batches):  # the unfused composition: select, the plain channel or the modem on E bits, recover
        if mode == "flooding-fixed-zero":
            cw = torch.zeros((N, F), dtype=torch.int32, device="cuda")
            y = C.RM_Recover(rm, C.AWGNChannel_GPU(seed, sigma, E, F), SHORT_LLR)
            r = C.LDPC_Decoder_GPU(code, y, max_iter=maxIT, length=K, exit_mode=C.EXIT_FIXED)
            iters = np.full(F, maxIT)
        else:
            cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F, rate_match=rm)
            tx = C.RM_Select(rm, cw)
            if mode == "qam64":
                rx = C.AWGNChannel_QAM_GPU(seed, sigma, C.Modulate_QAM(tx, E, m), cond)
                y = C.RM_Recover(rm, C.Demodulate_QAM(rx, cond, 1.0 / (2.0 * sigma * sigma), E), SHORT_LLR)
            else:
                y = C.RM_Recover(rm, C.AWGNChannel_GPU(seed, sigma, E, F, CodeWord=tx), SHORT_LLR)
            r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=maxIT, alpha=ALPHA, length=K, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
            iters = r["iters"].cpu().numpy()
        tot += _counts(r["D"].cpu().numpy(), cw.cpu().numpy(), iters, K)
    print("%s sigma %.5f: counters %s" % (mode, sigma, got))
    assert got == tot.tolist() and np.array_equal(got_seed, seed)
    assert 0 < got[0] < F * batches, "pick a sigma inside the waterfall"
    parts = [run(_Rank(r, 2)) for r in range(2)]  # world size 2: each rank jumps 2 E (or 4 ceil(E / m)) draws per frame of the other
    assert [a + b for a, b in zip(parts[0][0], parts[1][0])] == got
    assert np.array_equal(parts[0][1], got_seed) and np.array_equal(parts[1][1], got_seed)


def test_simulation_refuses_a_shortened_parity_position(C):
    from cuda_ldpc_amd.simulation import Simulation_GPU
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    parity = np.setdiff1d(np.arange(code.N), code.info_positions)
    rm = C.RateMatch(code.N, [int(parity[0])])
    with pytest.raises(ValueError, match="parity position"):
        Simulation_GPU(code, np.array([173, 173, 173], np.int32), 0.7, C.SimCounters(), Num_Frames_OneTime=64, max_batches=1, log=None,
                       device_channel=True, PN_Message=1, exit_mode=C.EXIT_FIXED, rate_match=rm)
