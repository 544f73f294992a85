"""Binary HARQ on the GPU: circular profiles through select, recover and combine against their host statements, the fused channel and
the fused channel + combine against the three-call composition on the device, all as bit patterns; guard words around every new
kernel's output; frame gather and scatter; the device refusals; Simulation_HARQ_GPU against a loop written out from the primitives,
with and without frame compaction and at world size 2."""
import ctypes

import numpy as np
import pytest
import torch

import qc_variant_cases as Q

pytestmark = pytest.mark.gpu

N1 = 2301  # the size of the rate-matching guard test: no multiple of the row tile of 32
SHORT_LLR = 1.0e4
# The lists of test_rate_match_gpu.py's channel test at this N.  Punctured: 40..49 starts and ends inside the run 32..63; 60..99 starts
# inside that run, removes the whole run 64..95 and ends inside 96..127; the last position.  Shortened: the head of the first run and a
# position between two punctured ranges.  Ncb = 2301 - 9 - 58 = 2234 is no multiple of 32.
CH_SHORT = list(range(0, 8)) + [55]
CH_PUNCT = list(range(40, 50)) + list(range(60, 100)) + list(range(1200, 1207)) + [N1 - 1]
NCB = N1 - len(CH_SHORT) - len(CH_PUNCT)
# (k0, E): the linear one; a wrap inside a run of 32 with unreached positions behind it; one position twice; two laps and a ragged third;
# eight laps.  k0 = 1000 wraps at codeword position 1000 + 9 + 50 = 1059, inside the run 1056..1087.
CASES = [(0, NCB), (37, NCB - 100), (NCB - 1, NCB + 1), (1000, 2 * NCB + 5), (5, 8 * NCB)]
CASE_IDS = ["k0=%d-E=%d" % c for c in CASES]
DONES = ["null", "all", "none", "alternating", "wavefront"]


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


def make_done(kind, F):
    """done as a CUDA int32 [F] (or None): every frame, none, every other one, and one whole wavefront of 64 frames inside a block of 256
    (frames 64..127; with F = 1 the one frame)."""
    if kind == "null":
        return None
    d = torch.zeros(F, dtype=torch.int32)
    if kind == "all":
        d[:] = 1
    elif kind == "alternating":
        d[1::2] = 9
    elif kind == "wavefront":
        d[64:128] = 1
        if F == 1:
            d[:] = 1
    return d.cuda()


def test_the_cases_are_what_they_are_there_for(C):
    assert NCB == 2234 and NCB % 32
    lin = C.RateMatch(N1, CH_SHORT, CH_PUNCT)
    wrap = int(lin.tx_pos[1000])
    assert wrap % 32 not in (0, 31), "k0 = 1000 wraps inside a run of 32"
    rm = C.RateMatch.circular(N1, CH_SHORT, CH_PUNCT, 37, NCB - 100)
    unreached = np.setdiff1d(lin.tx_pos, rm.tx_pos)
    assert unreached.size == 100 and (unreached % 32 == 0).any(), "a run whose first position is unreached"
    assert [C.RateMatch.circular(N1, CH_SHORT, CH_PUNCT, k0, E).laps for k0, E in CASES] == [1, 1, 2, 3, 8]
    assert any(E % 32 for _, E in CASES)


@pytest.mark.parametrize("F", [1, 257])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_select_recover_combine_equal_their_host_statements(C, case, F):
    k0, E = case
    rm = C.RateMatch.circular(N1, CH_SHORT, CH_PUNCT, k0, E)
    g = torch.Generator(device="cuda").manual_seed(E + F)
    cw = torch.randint(0, 2 ** 31 - 1, (N1, F), generator=g, device="cuda", dtype=torch.int32)
    tx = C.RM_Select(rm, cw)
    assert tx.shape == (E, F) and np.array_equal(tx.cpu().numpy(), C.RM_Select_host(rm, cw.cpu().numpy()))
    rx = torch.randn((E, F), generator=g, device="cuda")
    rx.view(-1)[:3] = torch.tensor([-0.0, float("inf"), 1e-42], device="cuda")[:rx.numel()]
    rxh = rx.cpu().numpy()
    got = C.RM_Recover(rm, rx, SHORT_LLR)
    torch.cuda.synchronize()
    assert got.shape == (N1, F) and np.array_equal(nbits(got.cpu().numpy()), nbits(C.RM_Recover_host(rm, rxh, SHORT_LLR)))
    acc0 = torch.randn((N1, F), generator=g, device="cuda")
    col = 65 if F > 65 else 0  # a NaN-payload sentinel column: with F = 257 done in "all", "alternating" and "wavefront"
    ibits(acc0)[:, col] = 0x7FC0BEEF
    for kind in DONES:
        done = make_done(kind, F)
        acc = acc0.clone()
        assert C.RM_Combine(rm, rx, acc, done, SHORT_LLR) is acc
        torch.cuda.synchronize()
        want = C.RM_Combine_host(rm, rxh, acc0.cpu().numpy().copy(), None if done is None else done.cpu().numpy(), SHORT_LLR)
        live = np.ones(F, bool) if done is None else done.cpu().numpy() == 0
        a = acc.cpu().numpy()
        # the sentinel column, where live, holds NaN + x: a NaN on both sides whose payload is not pinned; every other word is
        ok = nbits(a) == nbits(want)
        ok[:, col] |= np.isnan(a[:, col]) & np.isnan(want[:, col])
        assert ok.all(), kind
        assert np.array_equal(nbits(a)[:, ~live], nbits(acc0.cpu().numpy())[:, ~live]), kind + ": done columns keep their bits"


@pytest.mark.parametrize("F", [1, 257])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_channel_and_channel_combine_equal_the_composition(C, case, F):
    from cuda_ldpc_amd import sharding
    k0, E = case
    rm = C.RateMatch.circular(N1, CH_SHORT, CH_PUNCT, k0, E)
    g = torch.Generator(device="cuda").manual_seed(10 + F)
    cw = torch.randint(0, 2, (N1, F), generator=g, device="cuda", dtype=torch.int32)
    cw[torch.tensor(CH_SHORT, device="cuda")] = 0
    start, sigma = [173, 40001, 63598], 0.73
    for word in (cw, None):
        tx = None if word is None else C.RM_Select(rm, word)
        seed, seed_ref = np.array(start, np.int32), np.array(start, np.int32)
        for call in range(2):  # the second call continues from the advanced seed
            got = C.AWGNChannel_RM_GPU(rm, seed, sigma, F, CodeWord=word, short_llr=SHORT_LLR)
            want = C.RM_Recover(rm, C.AWGNChannel_GPU(seed_ref, sigma, E, F, CodeWord=tx), SHORT_LLR)
            torch.cuda.synchronize()
            assert torch.equal(ibits(got), ibits(want)), "channel, call %d, %s" % (call, "codeword" if word is not None else "zero word")
            assert np.array_equal(seed, seed_ref) and np.array_equal(seed, sharding.lcg_jump(start, 2 * E * F * (call + 1)))
        acc0 = got
        for kind in DONES:
            done = make_done(kind, F)
            seed, seed_ref = np.array(start, np.int32), np.array(start, np.int32)
            a, b = acc0.clone(), acc0.clone()
            for call in range(2):
                C.AWGNChannel_RM_Combine_GPU(rm, seed, sigma, a, done, CodeWord=word, short_llr=SHORT_LLR)
                C.RM_Combine(rm, C.AWGNChannel_GPU(seed_ref, sigma, E, F, CodeWord=tx), b, done, SHORT_LLR)
                torch.cuda.synchronize()
                assert torch.equal(ibits(a), ibits(b)), "channel + combine, %s, call %d" % (kind, call)
                assert np.array_equal(seed, seed_ref) and np.array_equal(seed, sharding.lcg_jump(start, 2 * E * F * (call + 1))), kind
            if done is not None:
                d = done.bool()
                assert torch.equal(ibits(a)[:, d], ibits(acc0)[:, d]) and (bool(d.all()) or not torch.equal(ibits(a), ibits(acc0)))


def test_new_kernels_write_inside_their_outputs(C):
    """Guard words around the outputs of every new kernel stay as set (F = 257: a ragged frame block; N, Ncb and E no multiple of the row
    tile), and the columns of done frames are bit-identical before and after."""
    from cuda_ldpc_amd._lib import check, lib
    F, G = 257, 64
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    done = make_done("alternating", F)
    d = done.bool()
    for k0, E in ((1000, 2 * NCB + 5), (37, NCB - 100)):
        rm = C.RateMatch.circular(N1, CH_SHORT, CH_PUNCT, k0, E)
        N = rm.N
        cw = torch.ones((N, F), dtype=torch.int32, device="cuda")
        tx = torch.full((E * F + 2 * G,), -7, dtype=torch.int32, device="cuda")
        check(lib.bldpc_rm_select(rm._h, P(cw), F, P(tx[G:]), st), "select")
        assert (tx[:G] == -7).all() and (tx[G + E * F:] == -7).all() and (tx[G:G + E * F] == 1).all()
        rx = torch.full((E, F), 2.5, device="cuda")
        reps = torch.from_numpy(np.bincount(rm.tx_pos, minlength=N)).cuda().float()[:, None]  # contributions per position
        sent = reps[:, 0] > 0
        short = torch.from_numpy(rm.shorten).long().cuda()
        for fill in ("recover", "channel", "combine", "channel+combine"):
            y = torch.full((N * F + 2 * G,), 123.0, device="cuda")
            seed = np.array([173, 173, 173], np.int32)
            sp = seed.ctypes.data_as(ctypes.c_void_p)
            llr, zero = ctypes.c_float(SHORT_LLR), ctypes.c_float(0.0)
            if fill == "recover":
                check(lib.bldpc_rm_recover(rm._h, P(rx), F, llr, P(y[G:]), st), fill)
            elif fill == "channel":  # sigma 0: every sample is 1 - 2c = 1.0 exactly
                check(lib.bldpc_rm_awgn_channel_device(rm._h, sp, zero, None, F, llr, P(y[G:]), st), fill)
            elif fill == "combine":
                check(lib.bldpc_rm_combine(rm._h, P(rx), F, llr, P(done), P(y[G:]), st), fill)
            else:
                check(lib.bldpc_rm_awgn_combine_device(rm._h, sp, zero, None, F, llr, P(done), P(y[G:]), st), fill)
            torch.cuda.synchronize()
            body = y[G:G + N * F].reshape(N, F)
            assert (y[:G] == 123.0).all() and (y[G + N * F:] == 123.0).all(), fill
            v = 2.5 if fill in ("recover", "combine") else 1.0
            if fill in ("recover", "channel"):  # small multiples of 2.5 and of 1.0 add exactly
                assert torch.equal(body[sent], (v * reps[sent]).expand(-1, F)), fill
                rest = ~sent
                rest[short] = False
                assert not ibits(body[rest]).any(), fill + ": no contribution is 0x00000000"
                assert (body[short] == SHORT_LLR).all(), fill
            else:
                assert (body[:, d] == 123.0).all(), fill + ": done columns"
                live = body[:, ~d]
                assert torch.equal(live[sent], (123.0 + v * reps[sent]).expand(-1, live.shape[1])), fill
                rest = ~sent
                rest[short] = False
                assert (live[rest] == 123.0).all() and (live[short] == SHORT_LLR).all(), fill
    # gather and scatter
    rows, Fa = 71, 63
    idx = torch.arange(0, 2 * Fa, 2, dtype=torch.int32, device="cuda")
    src = torch.ones((rows, F), dtype=torch.int32, device="cuda")
    out = torch.full((rows * Fa + 2 * G,), -7, dtype=torch.int32, device="cuda")
    check(lib.bldpc_frames_gather(P(src), rows, F, P(idx), Fa, P(out[G:]), st), "gather")
    assert (out[:G] == -7).all() and (out[G + rows * Fa:] == -7).all() and (out[G:G + rows * Fa] == 1).all()
    back = torch.full((rows * F + 2 * G,), -7, dtype=torch.int32, device="cuda")
    check(lib.bldpc_frames_scatter(P(out[G:]), rows, F, P(idx), Fa, P(back[G:]), st), "scatter")
    body = back[G:G + rows * F].reshape(rows, F)
    assert (back[:G] == -7).all() and (back[G + rows * F:] == -7).all()
    assert (body[:, idx.long()] == 1).all() and int((body == 1).sum()) == rows * Fa


@pytest.mark.parametrize("Fa", [1, 63, 257])
def test_gather_and_scatter_equal_their_host_twins(C, Fa):
    F, rows = 257, N1 + 1  # a whole D
    g = torch.Generator(device="cuda").manual_seed(Fa)
    D = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, F), generator=g, device="cuda", dtype=torch.int32)
    idx = torch.sort(torch.randperm(F, generator=g, device="cuda")[:Fa]).values.to(torch.int32)
    got = C.Frames_Gather(D, idx)
    assert got.shape == (rows, Fa) and np.array_equal(got.cpu().numpy(), C.Frames_Gather_host(D.cpu().numpy(), idx.cpu().numpy()))
    dst = torch.full((rows, F), -7, dtype=torch.int32, device="cuda")
    assert C.Frames_Scatter(got, idx, dst) is dst
    want = np.full((rows, F), -7, np.int32)
    C.Frames_Scatter_host(got.cpu().numpy(), idx.cpu().numpy(), want)
    assert np.array_equal(dst.cpu().numpy(), want)
    y = torch.randn((33, F), generator=g, device="cuda")  # float words, and a single row as iters
    assert torch.equal(ibits(C.Frames_Gather(y, idx)), ibits(y[:, idx.long()])) and torch.equal(C.Frames_Gather(D[5], idx), D[5][idx.long()])
    it = torch.zeros(F, dtype=torch.int32, device="cuda")
    C.Frames_Scatter(got[7].contiguous(), idx, it)
    assert torch.equal(it[idx.long()], got[7]) and int((it != 0).sum()) <= Fa


def test_device_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError, lib
    rm = C.RateMatch.circular(N1, [0], [1], 5, 3000)
    F = 2
    rx = torch.ones((rm.E, F), device="cuda")
    acc = torch.zeros((N1, F), device="cuda")
    done = torch.zeros(F, dtype=torch.int32, device="cuda")
    seed = np.array([173, 173, 173], np.int32)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="short_llr"):
            C.RM_Combine(rm, rx, acc, done, bad)
        with pytest.raises(ValueError, match="short_llr"):
            C.AWGNChannel_RM_Combine_GPU(rm, seed, 0.7, acc, done, short_llr=bad)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp = seed.ctypes.data_as(ctypes.c_void_p)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    one, sig = ctypes.c_float(1.0), ctypes.c_float(0.7)
    assert lib.bldpc_rm_combine(rm._h, P(rx), F, ctypes.c_float(float("inf")), None, P(acc), st) == -1 and b"short_llr" in lib.bldpc_last_error()
    assert lib.bldpc_rm_combine(rm._h, None, F, one, None, P(acc), st) == -1 and lib.bldpc_rm_combine(rm._h, P(rx), F, one, None, None, st) == -1
    assert lib.bldpc_rm_combine(None, P(rx), F, one, None, P(acc), st) == -1 and lib.bldpc_rm_combine(rm._h, P(rx), 0, one, None, P(acc), st) == -1
    assert lib.bldpc_rm_awgn_combine_device(rm._h, sp, sig, None, F, ctypes.c_float(0.0), None, P(acc), st) == -1
    assert lib.bldpc_rm_awgn_combine_device(rm._h, sp, sig, None, 0, one, None, P(acc), st) == -1
    assert lib.bldpc_rm_awgn_combine_device(rm._h, None, sig, None, F, one, None, P(acc), st) == -1
    assert lib.bldpc_rm_awgn_combine_device(rm._h, sp, sig, None, F, one, None, None, st) == -1
    assert lib.bldpc_rm_awgn_combine_device(None, sp, sig, None, F, one, None, P(acc), st) == -1
    with pytest.raises(LdpcError, match="seed"):
        C.AWGNChannel_RM_Combine_GPU(rm, np.array([173, 173, 63599], np.int32), 0.7, acc, done)
    assert not acc.any(), "a refused call writes nothing"
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    for fn in (lib.bldpc_frames_gather, lib.bldpc_frames_scatter):
        assert fn(P(acc), N1, F, P(idx), 0, P(acc), st) == -1 and b"Fa=0" in lib.bldpc_last_error()
        assert fn(P(acc), N1, F, P(idx), 3, P(acc), st) == -1 and fn(P(acc), 0, F, P(idx), 2, P(acc), st) == -1
        assert fn(None, N1, F, P(idx), 2, P(acc), st) == -1 and fn(P(acc), N1, F, None, 2, P(acc), st) == -1 and fn(P(acc), N1, F, P(idx), 2, None, st) == -1
    with pytest.raises(ValueError):
        C.RM_Combine(rm, rx[:-1].contiguous(), acc)
    with pytest.raises(ValueError):
        C.RM_Combine(rm, rx, acc, done[:1])
    with pytest.raises(ValueError):
        C.Frames_Gather(acc, idx.long())
    with pytest.raises(ValueError):
        C.Frames_Gather(acc, torch.arange(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        C.Frames_Scatter(acc, idx[:1], acc.clone())


# ---- Simulation_HARQ_GPU ----------------------------------------------------------------------------------------------------------
class _Rank:
    """One rank of a world of `world` without a process group: the all-reduce is the sum the test makes."""

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


SIM_SNR = 2.7  # Es/N0 of test_harq_cpu.test_the_direction_of_the_effect
SIM_SHORT, SIM_PUNCT = range(0, 24), range(2188, 2260)  # Ncb = 2304 - 24 - 72 = 2208
# the head of the buffer; the rest of it; a start in the middle that wraps and sends 92 positions a second time
# With the host statements on the host channel, two batches of 256 acknowledge 83, 274 and 155 frames at the three transmissions
# (layered) and 35, 236 and 241 (normalised flooding, 20 iterations); a first transmission of 2100 positions acknowledges none.
SIM_RVS = [(0, 2160), (2160, 48), (500, 2300)]


@pytest.mark.parametrize("mode", ["layered-per-frame-pn", "normalised-fixed-syndrome-pn"])
def test_simulation_harq_equals_a_loop_of_the_primitives(C, mode):
    from cuda_ldpc_amd import sharding
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    rvs = [C.RateMatch.circular(N, SIM_SHORT, SIM_PUNCT, k0, E) for k0, E in SIM_RVS]
    assert rvs[0].Ncb == 2208 and [r.laps for r in rvs] == [1, 1, 2]
    F, batches, pn_seed, alpha, T = 256, 2, 31337, 0.75, len(rvs)
    sigma = C.sigma_of(SIM_SNR)
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, short_llr=SHORT_LLR, leastTestFrames=10 ** 9, PN_Message=1, pn_seed=pn_seed, alpha=alpha)
    if mode == "layered-per-frame-pn":
        maxIT = 25
        kw.update(maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, schedule="layered", stop_rule=C.STOP_SYNDROME)
    else:
        maxIT = 20
        kw.update(maxIT=maxIT, exit_mode=C.EXIT_FIXED)

    def decode(y):
        if mode == "layered-per-frame-pn":
            r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=maxIT, alpha=alpha, length=K, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
            return r["D"], r["iters"].cpu().numpy().astype(np.int64)
        r = C.LDPC_Decoder_GPU(code, y, max_iter=maxIT, length=K, exit_mode=C.EXIT_FIXED, alpha=alpha)
        C.Syndrome(code, r["D"], into_flag_row=True)
        return r["D"], np.full(y.shape[1], maxIT, np.int64)

    def run(dist, compact=True):
        SIM, seed, Ds = HarqCounters(), np.array([173, 173, 173], np.int32), []
        Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, dist=dist, compact=compact, keep_D=Ds, **kw)
        assert SIM.num_Frames == F * batches
        return [SIM.acked, SIM.undetected, SIM.never_acked, SIM.bits_sent, SIM.Total_Iteration], seed, Ds

    got, got_seed, got_D = run(None)
    # the loop written out: every transmission drawn for the whole batch and combined under the flag row, the whole batch decoded again
    seed = np.array([173, 173, 173], np.int32)
    acked_t, und_t, never, bits, its = [0] * T, [0] * T, 0, 0, 0
    want_D = []
    for b in range(batches):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F, rate_match=rvs[0])
        cwh = cw.cpu().numpy()
        ack = np.zeros(F, bool)
        for t, rm in enumerate(rvs):
            tx = C.RM_Select(rm, cw)
            rx = C.AWGNChannel_GPU(seed, sigma, rm.E, F, CodeWord=tx)  # the seed moves 2 E_t F draws whether any frame needs them or not
            if t == 0:
                y = C.RM_Recover(rm, rx, SHORT_LLR)
            elif ack.all():
                continue
            else:
                C.RM_Combine(rm, rx, y, torch.from_numpy(ack.astype(np.int32)).cuda(), SHORT_LLR)
            D, it = decode(y)
            Dh = D.cpu().numpy()
            now = (Dh[N] != 0) & ~ack
            wrong = (Dh[:K] != cwh[:K]).any(0)
            acked_t[t] += int(now.sum())
            und_t[t] += int((now & wrong).sum())
            bits += rm.E * int((~ack).sum())
            its += int(it[~ack].sum())
            ack |= now
        never += int((~ack).sum())
        want_D.append(Dh)
    want = [acked_t, und_t, never, bits, its]
    print("%s sigma %.5f: acked %s undetected %s never %d bits %d iterations %d" % (mode, sigma, *got))
    assert got == want and np.array_equal(got_seed, seed)
    assert np.array_equal(seed, sharding.lcg_jump([173, 173, 173], 2 * sum(E for _, E in SIM_RVS) * F * batches))
    assert all(np.array_equal(a.cpu().numpy(), w) for a, w in zip(got_D, want_D)), "D after the last decode of every batch"
    assert 0 < got[0][0] < F * batches and got[0][1] > 0, "pick a sigma at which the first transmission fails for some frames and not for all"
    whole, whole_seed, whole_D = run(None, compact=False)
    assert whole == got and np.array_equal(whole_seed, got_seed) and all(torch.equal(a, w) for a, w in zip(got_D, whole_D))
    parts = [run(_Rank(r, 2)) for r in range(2)]  # world size 2: each rank jumps 2 E_t draws per frame of the other in every transmission
    summed = [[a + b for a, b in zip(parts[0][0][i], parts[1][0][i])] for i in (0, 1)] + [parts[0][0][i] + parts[1][0][i] for i in (2, 3, 4)]
    assert summed == got
    assert np.array_equal(parts[0][1], got_seed) and np.array_equal(parts[1][1], got_seed)
    assert all(torch.equal(torch.cat([p0, p1], 1), d) for p0, p1, d in zip(parts[0][2], parts[1][2], got_D))
