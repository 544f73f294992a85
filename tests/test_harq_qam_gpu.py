"""Binary HARQ over QAM on the GPU: the modem kernels under both index rules against their host statements; the fused select +
interleave + map against select, map on the device and against its host twin; the fused demap + de-interleave + recover / combine
against demap, recover / combine on the device, all as bit patterns; guard words around every output; the device refusals;
Simulation_GPU with a rate-matched word over 64-QAM and Simulation_HARQ_GPU over 64-QAM against loops written out from the unfused
primitives, the latter with and without frame compaction and at world size 2."""
import ctypes

import numpy as np
import pytest
import torch

import harq_qam_cases as K
import qc_variant_cases as Q
from harq_qam_cases import IL_NONE, IL_ROWCOL, SHORT_LLR, make_done
from test_harq_gpu import SIM_PUNCT, SIM_RVS, SIM_SHORT, _Rank, ibits
from test_rate_match_gpu import _counts

pytestmark = pytest.mark.gpu

P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
SIGMA = 0.25  # of the noise on the test points: a good share of them leave their decision region


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def noisy_points(con, sym, g):
    """rx [F, Ns, 2] around the points of sym, with one received point exactly on a constellation point."""
    rx = (con[sym.long()] + SIGMA * torch.randn(sym.shape + (2,), generator=g, device="cuda")).contiguous()
    rx[0, 0] = con[0]
    return rx


def start_acc(N, F, g):
    """Channel_Acc before a combine: random values with -0.0 and a large one in every column, so that "untouched" is visible."""
    acc = torch.randn((N, F), generator=g, device="cuda")
    acc[3] = -0.0
    acc[100 % N] = 3.0e38
    return acc


@pytest.mark.parametrize("F", [1, 257])
@pytest.mark.parametrize("N,m", K.MODEM_SHAPES)
def test_modem_kernels_equal_their_host_twins(C, N, m, F):
    from cuda_ldpc_amd._lib import check, lib
    con = K.constellation(C, 1 << m)
    cond = torch.from_numpy(con).cuda()
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + m * 10 + F)
    cw = torch.randint(0, 2 ** 31 - 1, (N, F), generator=g, device="cuda", dtype=torch.int32)
    Ns = K.n_sym(N, m)
    for il in K.RULES:
        sym = C.Modulate_QAM(cw, N, m, interleave=il)
        assert sym.shape == (F, Ns) and np.array_equal(sym.cpu().numpy(), C.Modulate_QAM_host(cw.cpu().numpy(), N, m, interleave=il)), ("map", il)
        rx = noisy_points(cond, sym, g)
        for scale in (1.0, 1.0 / (2 * SIGMA * SIGMA)):
            got = C.Demodulate_QAM(rx, cond, scale, N, interleave=il)
            want = C.Demodulate_QAM_host(rx.cpu().numpy(), con, scale, N, interleave=il)
            assert got.shape == (N, F) and np.array_equal(K.bits(got.cpu().numpy()), K.bits(want)), ("demap", il, scale)
        if il == IL_NONE:  # the entry points from before the interleaver, device against device
            old_sym, old = torch.empty_like(sym), torch.empty_like(got)
            check(lib.bldpc_qam_map(P(cw), N, F, m, P(old_sym), stream()), "bldpc_qam_map")
            check(lib.bldpc_qam_demap(P(rx), P(cond), len(con), ctypes.c_float(scale), N, F, P(old), stream()), "bldpc_qam_demap")
            assert torch.equal(old_sym, sym) and torch.equal(ibits(old), ibits(got))


@pytest.mark.parametrize("F", [1, 257])
@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_fused_map_equals_select_then_map(C, case, F):
    k0, E = case
    rm = C.RateMatch.circular(K.N1, K.CH_SHORT, K.CH_PUNCT, k0, E)
    g = torch.Generator(device="cuda").manual_seed(E + F)
    cw = torch.randint(0, 2 ** 31 - 1, (K.N1, F), generator=g, device="cuda", dtype=torch.int32)
    tx = C.RM_Select(rm, cw)
    cwh = cw.cpu().numpy()
    for m in (2, 6, 8):
        for il in K.RULES:
            got = C.RM_Modulate_QAM(rm, cw, m, interleave=il)
            assert got.shape == (F, K.n_sym(E, m)) and got.dtype == torch.int32
            assert torch.equal(got, C.Modulate_QAM(tx, E, m, interleave=il)), (m, il)
            assert np.array_equal(got.cpu().numpy(), C.RM_Modulate_QAM_host(rm, cwh, m, interleave=il)), (m, il)
            zero = C.RM_Modulate_QAM(rm, None, m, F=F, interleave=il)
            assert zero.shape == got.shape and not zero.any()


def _check_recover_and_combine(C, rm, q, il, F, kinds, g):
    m = q.bit_length() - 1
    cond = torch.from_numpy(K.constellation(C, q)).cuda()
    sym = torch.randint(0, q, (F, K.n_sym(rm.E, m)), generator=g, device="cuda", dtype=torch.int32)
    rx = noisy_points(cond, sym, g)
    scale = 1.0 / (2 * SIGMA * SIGMA)
    tmp = C.Demodulate_QAM(rx, cond, scale, rm.E, interleave=il)
    got = C.RM_Demodulate_QAM_Recover(rm, rx, cond, scale, SHORT_LLR, interleave=il)
    assert got.shape == (rm.N, F) and torch.equal(ibits(got), ibits(C.RM_Recover(rm, tmp, SHORT_LLR))), ("recover", q, il)
    acc0 = start_acc(rm.N, F, g)
    for kind in kinds:
        done = make_done(kind, F)
        a, b = acc0.clone(), acc0.clone()
        assert C.RM_Demodulate_QAM_Combine(rm, rx, cond, scale, a, done, SHORT_LLR, interleave=il) is a
        C.RM_Combine(rm, tmp, b, done, SHORT_LLR)
        assert torch.equal(ibits(a), ibits(b)), ("combine", kind, q, il)
        if done is not None:
            d = done.bool()
            assert torch.equal(ibits(a)[:, d], ibits(acc0)[:, d]) and (bool(d.all()) or not torch.equal(ibits(a), ibits(acc0)))
    return got


@pytest.mark.parametrize("F", [1, 257])
@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_fused_recover_and_combine_at_64qam_rowcol(C, case, F):
    """Every case and every kind of done.  Also against the host twin once per case: the device composition is held to its own host
    statements elsewhere, this ties the fused call to its twin directly."""
    k0, E = case
    rm = C.RateMatch.circular(K.N1, K.CH_SHORT, K.CH_PUNCT, k0, E)
    g = torch.Generator(device="cuda").manual_seed(7 * E + F)
    _check_recover_and_combine(C, rm, 64, IL_ROWCOL, F, K.DONES, g)
    if F == 1:
        con = K.constellation(C, 64)
        cond = torch.from_numpy(con).cuda()
        rx = noisy_points(cond, torch.randint(0, 64, (3, K.n_sym(E, 6)), generator=g, device="cuda", dtype=torch.int32), g)
        got = C.RM_Demodulate_QAM_Recover(rm, rx, cond, 2.0, SHORT_LLR, interleave=IL_ROWCOL)
        want = C.RM_Demodulate_QAM_Recover_host(rm, rx.cpu().numpy(), con, 2.0, SHORT_LLR, interleave=IL_ROWCOL)
        assert np.array_equal(K.bits(got.cpu().numpy()), K.bits(want))


OTHER = [(1 << m, il) for m in (1, 2, 6, 7, 8) for il in K.RULES if (m, il) != (6, IL_ROWCOL)]


@pytest.mark.parametrize("q,il", OTHER)
def test_fused_recover_and_combine_at_the_other_sizes(C, q, il):
    """One lap with unreached positions, three laps, eight; every other frame done."""
    for k0, E in (K.CASES[1], K.CASES[3], K.CASES[4]):
        rm = C.RateMatch.circular(K.N1, K.CH_SHORT, K.CH_PUNCT, k0, E)
        g = torch.Generator(device="cuda").manual_seed(q + il + E)
        _check_recover_and_combine(C, rm, q, il, 257, ["alternating"], g)
    lin = C.RateMatch(K.N1, K.CH_SHORT, K.CH_PUNCT)  # a linear profile through the same calls
    _check_recover_and_combine(C, lin, q, il, 65, ["null", "alternating"], torch.Generator(device="cuda").manual_seed(q))


def test_new_kernels_write_inside_their_outputs(C):
    """Guard words around sym, Channel_Out and Channel_Acc stay as set: F = 257 (a ragged frame tile) at profiles whose E is no multiple
    of any tile, and the two smallest modem shapes, (7, 3) and (1, 8), with and without a profile."""
    from cuda_ldpc_amd._lib import check, lib
    F, G = 257, 64
    st = stream()
    done = make_done("alternating", F)
    d = done.bool()
    llr = ctypes.c_float(SHORT_LLR)
    small = C.RateMatch.circular(10, [0], [9], 2, 7), C.RateMatch.circular(10, [0], [9], 3, 1)
    profiles = [(C.RateMatch.circular(K.N1, K.CH_SHORT, K.CH_PUNCT, k0, E), 6) for k0, E in ((1000, 2 * K.NCB + 5), (37, K.NCB - 100))]
    for rm, m in profiles + [(small[0], 3), (small[1], 8)]:
        N, E, q = rm.N, rm.E, 1 << m
        Ns = K.n_sym(E, m)
        cond = torch.from_numpy(K.constellation(C, q)).cuda()
        cw = torch.ones((max(N, E), F), dtype=torch.int32, device="cuda")  # N rows for the profile, E for the modem alone
        reps =torch.from_numpy(np.bincount(rm.tx_pos, minlength=N)).cuda()
        sent = reps > 0
        short = torch.zeros(N, dtype=torch.bool, device="cuda")
        short[torch.from_numpy(rm.shorten).long().cuda()] = True
        for il in K.RULES:
            # the two maps: every bit 1, so every index is all ones but for its pad bits
            want_sym = torch.from_numpy(K.np_map(np.ones((E, 1), np.int32), E, m, il)).cuda().expand(F, Ns)
            for fused in (False, True):
                sym = torch.full((F * Ns + 2 * G,), -7, dtype=torch.int32, device="cuda")
                if fused:
                    check(lib.bldpc_rm_qam_map(rm._h, P(cw), F, m, il, P(sym[G:]), st), "rm_qam_map")
                else:
                    check(lib.bldpc_qam_map_il(P(cw), E, F, m, il, P(sym[G:]), st), "qam_map_il")
                assert (sym[:G] == -7).all() and (sym[G + F * Ns:] == -7).all(), (fused, il)
                assert torch.equal(sym[G:G + F * Ns].reshape(F, Ns), want_sym), (fused, il)
            # received exactly on the points of the all-ones word: every soft value is negative
            rx = cond[want_sym.long()].contiguous()
            one = ctypes.c_float(1.0)
            y = torch.full((E * F + 2 * G,), 123.0, device="cuda")
            check(lib.bldpc_qam_demap_il(P(rx), P(cond), q, one, E, F, il, P(y[G:]), st), "qam_demap_il")
            assert (y[:G] == 123.0).all() and (y[G + E * F:] == 123.0).all() and (y[G:G + E * F] < 0).all(), il
            tmp = y[G:G + E * F].reshape(E, F)
            for combine in (False, True):
                y = torch.full((N * F + 2 * G,), 123.0, device="cuda")
                if combine:
                    check(lib.bldpc_rm_qam_combine(rm._h, P(rx), P(cond), q, one, il, F, llr, P(done), P(y[G:]), st), "rm_qam_combine")
                else:
                    check(lib.bldpc_rm_qam_recover(rm._h, P(rx), P(cond), q, one, il, F, llr, P(y[G:]), st), "rm_qam_recover")
                torch.cuda.synchronize()
                assert (y[:G] == 123.0).all() and (y[G + N * F:] == 123.0).all(), (combine, il)
                body = y[G:G + N * F].reshape(N, F)
                rest = ~sent & ~short
                if combine:
                    assert (body[:, d] == 123.0).all(), "done columns"
                    live = body[:, ~d]
                    assert (live[sent] < 123.0).all() and (live[rest] == 123.0).all() and (live[short] == SHORT_LLR).all(), il
                    ref = torch.full((N, F), 123.0, device="cuda")
                    assert torch.equal(ibits(C.RM_Combine(rm, tmp, ref, done, SHORT_LLR)), ibits(body))
                else:
                    assert (body[sent] < 0).all() and not ibits(body[rest]).any() and (body[short] == SHORT_LLR).all(), il
                    assert torch.equal(ibits(C.RM_Recover(rm, tmp.contiguous(), SHORT_LLR)), ibits(body))


def test_device_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError, lib
    rm = C.RateMatch.circular(K.N1, [0], [1], 5, 3000)
    F, m, q = 2, 2, 4
    Ns = K.n_sym(rm.E, m)
    st = stream()
    cond = torch.from_numpy(K.constellation(C, q)).cuda()
    cw = torch.ones((K.N1, F), dtype=torch.int32, device="cuda")
    sym = torch.full((F, Ns), -7, dtype=torch.int32, device="cuda")
    rx = torch.ones((F, Ns, 2), device="cuda")
    acc = torch.zeros((K.N1, F), device="cuda")
    tmp = torch.zeros((rm.E, F), device="cuda")
    one, inf = ctypes.c_float(1.0), ctypes.c_float(float("inf"))
    err = lambda: lib.bldpc_last_error().decode()  # noqa: E731
    for il in (-1, 2):
        assert lib.bldpc_qam_map_il(P(cw), rm.E, F, m, il, P(sym), st) == -1 and "interleave=%d" % il in err()
        assert lib.bldpc_qam_demap_il(P(rx), P(cond), q, one, rm.E, F, il, P(tmp), st) == -1 and "interleave=%d" % il in err()
        assert lib.bldpc_rm_qam_map(rm._h, P(cw), F, m, il, P(sym), st) == -1 and "interleave=%d" % il in err()
        assert lib.bldpc_rm_qam_recover(rm._h, P(rx), P(cond), q, one, il, F, one, P(acc), st) == -1 and "interleave=%d" % il in err()
        assert lib.bldpc_rm_qam_combine(rm._h, P(rx), P(cond), q, one, il, F, one, None, P(acc), st) == -1 and "interleave=%d" % il in err()
    assert lib.bldpc_rm_qam_map(None, P(cw), F, m, 0, P(sym), st) == -1 and "null profile" in err()
    assert lib.bldpc_rm_qam_map(rm._h, P(cw), 0, m, 0, P(sym), st) == -1 and "F=0" in err()
    assert lib.bldpc_rm_qam_map(rm._h, P(cw), F, 9, 0, P(sym), st) == -1 and "m=9" in err()
    assert lib.bldpc_rm_qam_map(rm._h, P(cw), F, m, 0, None, st) == -1 and "sym is NULL" in err()
    for fn, tail in ((lib.bldpc_rm_qam_recover, [P(acc)]), (lib.bldpc_rm_qam_combine, [None, P(acc)])):
        assert fn(None, P(rx), P(cond), q, one, 0, F, one, *tail, st) == -1 and "null profile" in err()
        assert fn(rm._h, P(rx), P(cond), q, one, 0, 0, one, *tail, st) == -1 and "F=0" in err()
        assert fn(rm._h, P(rx), P(cond), 3, one, 0, F, one, *tail, st) == -1 and "q=3" in err()
        assert fn(rm._h, P(rx), P(cond), 512, one, 0, F, one, *tail, st) == -1 and "q=512" in err()
        assert fn(rm._h, P(rx), P(cond), q, inf, 0, F, one, *tail, st) == -1 and "scale" in err()
        for bad in (0.0, -2.0, float("inf"), float("nan")):
            assert fn(rm._h, P(rx), P(cond), q, one, 0, F, ctypes.c_float(bad), *tail, st) == -1 and "short_llr" in err()
        assert fn(rm._h, None, P(cond), q, one, 0, F, one, *tail, st) == -1 and "NULL" in err()
        assert fn(rm._h, P(rx), None, q, one, 0, F, one, *tail, st) == -1 and fn(rm._h, P(rx), P(cond), q, one, 0, F, one, *tail[:-1], None, st) == -1
    torch.cuda.synchronize()
    assert (sym == -7).all() and not acc.any() and not tmp.any(), "a refused call launches nothing"
    with pytest.raises(ValueError, match="interleave"):
        C.RM_Modulate_QAM(rm, cw, m, interleave=2)
    with pytest.raises(ValueError):
        C.RM_Modulate_QAM(rm, cw[:-1].contiguous(), m)
    with pytest.raises(ValueError, match=r"ceil\(E / m\)"):
        C.RM_Demodulate_QAM_Recover(rm, rx[:, :-1].contiguous(), cond, 1.0)
    with pytest.raises(ValueError, match="rx holds"):
        C.RM_Demodulate_QAM_Combine(rm, rx[:1].contiguous(), cond, 1.0, acc)
    with pytest.raises(ValueError):
        C.RM_Demodulate_QAM_Combine(rm, rx, cond, 1.0, acc, done=torch.zeros(F + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="short_llr"):
        C.RM_Demodulate_QAM_Combine(rm, rx, cond, 1.0, acc, short_llr=float("inf"))
    with pytest.raises(ValueError, match="constellation"):
        C.RM_Demodulate_QAM_Recover(rm, rx, cond.cpu(), 1.0)
    assert LdpcError is not None and not acc.any()


# ---- the sweeps -------------------------------------------------------------------------------------------------------------------
ALPHA = 0.75


@pytest.mark.parametrize("il", K.RULES, ids=["none", "rowcol"])
def test_simulation_over_qam_equals_a_loop_of_the_unfused_primitives(C, il):
    """Simulation_GPU(rate_match, n_QAM=64): the fused calls inside it against select, map, channel, demap, recover written out here,
    in every counter and in the seed.  J4_L24_Z96 with the lists of test_rate_match_gpu.py, Eb/N0 10.5 dB as there."""
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd.simulation import Simulation_GPU
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    rm = C.RateMatch(code.N, SIM_SHORT, SIM_PUNCT)
    F, batches, pn_seed, q, m, maxIT = 512, 2, 31337, 64, 6, 25
    Kc, E = code.K, rm.E
    con = K.constellation(C, q)
    cond = torch.from_numpy(con).cuda()
    sigma = nb.sigma_of(10.5, rm.rate(Kc), 0, q)
    SIM, seed = C.SimCounters(), np.array([173, 173, 173], np.int32)
    Simulation_GPU(code, seed, sigma, SIM, Num_Frames_OneTime=F, max_batches=batches, log=None, device_channel=True, rate_match=rm, short_llr=SHORT_LLR,
                   leastTestFrames=10 ** 9, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, PN_Message=1, pn_seed=pn_seed, schedule="layered", alpha=ALPHA,
                   n_QAM=q, CONSTELLATION=con, interleave=il)
    got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
    ref_seed = np.array([173, 173, 173], np.int32)
    tot = np.zeros(5, np.int64)
    for b in range(batches):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F, rate_match=rm)
        tx = C.RM_Select(rm, cw)
        rx = C.AWGNChannel_QAM_GPU(ref_seed, sigma, C.Modulate_QAM(tx, E, m, interleave=il), cond)
        y = C.RM_Recover(rm, C.Demodulate_QAM(rx, cond, 1.0 / (2.0 * sigma * sigma), E, interleave=il), SHORT_LLR)
        r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=maxIT, alpha=ALPHA, length=Kc, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        tot += _counts(r["D"].cpu().numpy(), cw.cpu().numpy(), r["iters"].cpu().numpy(), Kc)
    print("interleave %d sigma %.5f: counters %s" % (il, sigma, got))
    assert got == tot.tolist() and np.array_equal(seed, ref_seed)
    assert 0 < got[0] < F * batches, "pick a sigma inside the waterfall"


HARQ_EBN0 = 11.0  # dB on the first transmission's rate: on the CPU, with numpy noise, 81 of 128 first transmissions fail the syndrome


def test_simulation_harq_over_qam_equals_a_loop_of_the_primitives(C):
    """Simulation_HARQ_GPU(n_QAM=64, interleave=IL_ROWCOL, PN_Message=1), layered per-frame with the syndrome stop, J4_L24_Z96 with the
    profiles of test_harq_gpu.py, 2 batches of 512 frames, against select, map, channel, demap, recover / combine and a decode of the
    whole batch after every transmission."""
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd import sharding
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, Kc = code.N, code.K
    rvs = [C.RateMatch.circular(N, SIM_SHORT, SIM_PUNCT, k0, E) for k0, E in SIM_RVS]
    F, batches, pn_seed, T, q, m, maxIT, il = 512, 2, 31337, len(rvs), 64, 6, 25, IL_ROWCOL
    con = K.constellation(C, q)
    cond = torch.from_numpy(con).cuda()
    sigma = nb.sigma_of(HARQ_EBN0, rvs[0].rate(Kc), 0, q)
    scale = 1.0 / (2.0 * sigma * sigma)
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, short_llr=SHORT_LLR, leastTestFrames=10 ** 9, PN_Message=1, pn_seed=pn_seed,
              alpha=ALPHA, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, schedule="layered", stop_rule=C.STOP_SYNDROME, n_QAM=q, CONSTELLATION=con,
              interleave=il)

    def run(dist, compact=True):
        SIM, seed, Ds = HarqCounters(), np.array([173, 173, 173], np.int32), []
        Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, dist=dist, compact=compact, keep_D=Ds, **kw)
        assert SIM.num_Frames == F * batches
        return [SIM.acked, SIM.undetected, SIM.never_acked, SIM.bits_sent, SIM.Total_Iteration], seed, Ds

    got, got_seed, got_D = run(None)
    seed = np.array([173, 173, 173], np.int32)
    acked_t, und_t, never, nbits, its = [0] * T, [0] * T, 0, 0, 0
    want_D = []
    for b in range(batches):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F, rate_match=rvs[0])
        cwh = cw.cpu().numpy()
        ack = np.zeros(F, bool)
        for t, rm in enumerate(rvs):
            sym = C.Modulate_QAM(C.RM_Select(rm, cw), rm.E, m, interleave=il)
            rx = C.AWGNChannel_QAM_GPU(seed, sigma, sym, cond)  # the seed moves 4 ceil(E_t / m) F draws whether any frame needs them or not
            llr = C.Demodulate_QAM(rx, cond, scale, rm.E, interleave=il)
            if t == 0:
                y = C.RM_Recover(rm, llr, SHORT_LLR)
            elif ack.all():
                continue
            else:
                C.RM_Combine(rm, llr, y, torch.from_numpy(ack.astype(np.int32)).cuda(), SHORT_LLR)
            r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=maxIT, alpha=ALPHA, length=Kc, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
            Dh, it = r["D"].cpu().numpy(), r["iters"].cpu().numpy().astype(np.int64)
            now = (Dh[N] != 0) & ~ack
            wrong = (Dh[:Kc] != cwh[:Kc]).any(0)
            acked_t[t] += int(now.sum())
            und_t[t] += int((now & wrong).sum())
            nbits += rm.E * int((~ack).sum())
            its += int(it[~ack].sum())
            ack |= now
        never += int((~ack).sum())
        want_D.append(Dh)
    want = [acked_t, und_t, never, nbits, its]
    print("64-QAM rowcol sigma %.5f: acked %s undetected %s never %d bits %d iterations %d" % (sigma, *got))
    assert got == want and np.array_equal(got_seed, seed)
    draws = sum(sharding.qam_draws_per_frame(E, m) for _, E in SIM_RVS)
    assert np.array_equal(seed, sharding.lcg_jump([173, 173, 173], draws * F * batches))
    assert all(np.array_equal(a.cpu().numpy(), w) for a, w in zip(got_D, want_D)), "D after the last decode of every batch"
    assert 0 < got[0][0] < F * batches and sum(got[0][1:]) > 0, "pick a sigma at which the first transmission fails for some frames and not for all"
    whole, whole_seed, whole_D = run(None, compact=False)
    assert whole == got and np.array_equal(whole_seed, got_seed) and all(torch.equal(a, w) for a, w in zip(got_D, whole_D))
    parts = [run(_Rank(r, 2)) for r in range(2)]  # world size 2: each rank jumps 4 ceil(E_t / m) draws per frame of the other
    summed = [[a + b for a, b in zip(parts[0][0][i], parts[1][0][i])] for i in (0, 1)] + [parts[0][0][i] + parts[1][0][i] for i in (2, 3, 4)]
    assert summed == got
    assert np.array_equal(parts[0][1], got_seed) and np.array_equal(parts[1][1], got_seed)
    assert all(torch.equal(torch.cat([p0, p1], 1), d) for p0, p1, d in zip(parts[0][2], parts[1][2], got_D))
