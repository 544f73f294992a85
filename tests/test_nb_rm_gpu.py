"""Rate matching over GF(q) symbol vectors on the device: every device call of include/nbldpc.h, "rate matching", against its host
twin, uint32-exact, over the shared table of tests/nb_rm_cases.py; the fused calls against the composition of device calls; the done
mask; writes inside the outputs; the shortened encoder; the batch independence Simulation_HARQ_GPU rests on; and the two simulations
against hand-written loops of the unfused primitives."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import nb_rm_cases as K
from conftest import DATA

pytestmark = pytest.mark.gpu
NBD = os.path.join(DATA, "nb")
EINVAL = -1


@pytest.fixture(scope="module")
def nb():
    from cuda_ldpc_amd import nbldpc
    return nbldpc


@pytest.fixture(scope="module")
def RateMatch():
    from cuda_ldpc_amd.bldpc import RateMatch
    return RateMatch


@pytest.fixture(scope="module")
def bds(nb):
    mul, _, _ = nb.GFInitial(64, os.path.join(NBD, "GF", "Arith.Table.GF.64.txt"))
    return nb.NBCode(os.path.join(NBD, "BDS.576.288.GF.64.txt"), mul)


def u32(a):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


CASES = [(N, q, name) for N in K.NS for q in K.QS for name in K.profiles(N)]


@pytest.mark.parametrize("N,q,name", CASES, ids=["N%d-q%d-%s" % c for c in CASES])
def test_device_calls_equal_their_host_twins(nb, RateMatch, N, q, name):
    """select, recover, combine (normal and special-value inputs) and the four fused calls (sigma 0.7, output of the host channel),
    for B in 1, 3, 257 and every done mask; each fused call also against the composition of device calls."""
    spec = K.profiles(N)[name]
    t, rm = K.Tables(N, spec), K.make_rm(RateMatch, N, spec)
    V = q - 1
    for B in K.BS:
        masks = K.done_masks(B)
        cw = np.random.default_rng(N + q + B).integers(0, q, size=(B, N)).astype(np.int32)
        assert np.array_equal(nb.RM_Select(rm, dev(cw)).cpu().numpy(), nb.RM_Select_host(rm, cw))
        acc0 = K.normal((B, N, V), 11 * N + q + B)
        u32(acc0)[:] = 0x40000000 | (np.arange(acc0.size, dtype=np.uint32).reshape(acc0.shape) & 0xFFFFF)  # a bit pattern, floats in [2, 2.25)
        u32(acc0)[B // 2, N // 2, V // 2] = K.NAN_PAYLOAD  # survives where its frame is done
        for kind, Lrx in (("normal", K.normal((B, t.E, V), 7 * N + q + B)), ("special", K.special_lrx(t, V, B, 9 * N + q + B))):
            Lrxd = dev(Lrx)
            got = nb.RM_Recover(rm, q, Lrxd, K.SHORT_LLR)
            assert np.array_equal(u32(got), u32(nb.RM_Recover_host(rm, q, Lrx, K.SHORT_LLR))), (B, kind, "recover")
            for mname, done in masks.items():
                want = nb.RM_Combine_host(rm, q, Lrx, acc0.copy(), done, K.SHORT_LLR)
                got = nb.RM_Combine(rm, q, Lrxd, dev(acc0), dev(done), K.SHORT_LLR).cpu().numpy()
                same = (u32(got) == u32(want)) | (np.isnan(got) & np.isnan(want))  # NaN + x: the payload is not pinned
                assert same.all() and np.isnan(got).sum() <= 2, (B, kind, mname, "combine")
                if done is not None:
                    assert np.array_equal(u32(got)[done != 0], u32(acc0)[done != 0]), (B, kind, mname, "a done frame keeps every bit")
        for qam in (True, False):
            con = K.constellation(q) if qam else None
            cond = dev(con)
            rx = K.channel_output(nb, t, q, B, 13 * N + q + B, qam=qam)
            rxd = dev(rx)
            Lrxd = nb.Demodulate_NQ(t.E, q, rxd, K.SIGMA, CONSTELLATION=cond)
            assert np.array_equal(u32(Lrxd), u32(nb.Demodulate_NQ_host(t.E, q, rx, K.SIGMA, CONSTELLATION=con))), (B, qam, "demodulate at N := E")
            got = nb.RM_Demodulate_Recover(rm, q, rxd, K.SIGMA, K.SHORT_LLR, CONSTELLATION=cond)
            assert np.array_equal(u32(got), u32(nb.RM_Demodulate_Recover_host(rm, q, rx, K.SIGMA, K.SHORT_LLR, CONSTELLATION=con))), (B, qam, "fused recover")
            assert torch.equal(got.view(torch.int32), nb.RM_Recover(rm, q, Lrxd, K.SHORT_LLR).view(torch.int32)), (B, qam, "fused recover, composition")
            for mname, done in masks.items():
                want = nb.RM_Demodulate_Combine_host(rm, q, rx, K.SIGMA, acc0.copy(), done, K.SHORT_LLR, CONSTELLATION=con)
                got = nb.RM_Demodulate_Combine(rm, q, rxd, K.SIGMA, dev(acc0), dev(done), K.SHORT_LLR, CONSTELLATION=cond)
                comp = nb.RM_Combine(rm, q, Lrxd, dev(acc0), dev(done), K.SHORT_LLR)
                assert torch.equal(got.view(torch.int32), comp.view(torch.int32)), (B, qam, mname, "fused combine, composition")
                got = got.cpu().numpy()
                same = (u32(got) == u32(want)) | (np.isnan(got) & np.isnan(want))
                assert same.all() and np.isnan(got).sum() <= 1, (B, qam, mname, "fused combine")
                if done is not None:
                    assert np.array_equal(u32(got)[done != 0], u32(acc0)[done != 0]), (B, qam, mname)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("N,q,B", [(7, 4, 3), (96, 256, 257)])
def test_kernels_write_inside_their_outputs(nb, RateMatch, N, q, B):
    """Every output sits inside a larger tensor between two canary bands, one float past the band so that its base is only 4-byte
    aligned; the bands are intact afterwards and the result is the host twin's."""
    from cuda_ldpc_amd._lib import lib
    G, V, m = 64, q - 1, q.bit_length() - 1
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    llr, sig = ctypes.c_float(K.SHORT_LLR), ctypes.c_float(K.SIGMA)
    done = K.done_masks(B)["alternating"]
    doned, cond = dev(done), dev(K.constellation(q))
    for name in ("linear", "circ_twice", "circ_short", "circ_3laps_part"):
        spec = K.profiles(N)[name]
        t, rm = K.Tables(N, spec), K.make_rm(RateMatch, N, spec)

        def banded(n, fill, dtype):
            buf = torch.full((n + 2 * G + 1,), fill, dtype=dtype, device="cuda")
            return buf, buf[G + 1:G + 1 + n]

        def intact(buf, n, fill):
            torch.cuda.synchronize()
            return bool((buf[:G + 1] == fill).all() and (buf[G + 1 + n:] == fill).all())

        cw = np.random.default_rng(N + q).integers(0, q, size=(B, N)).astype(np.int32)
        buf, out = banded(B * t.E, -7, torch.int32)
        assert lib.nbldpc_rm_select(rm._h, P(dev(cw)), B, P(out), st) == 0
        assert intact(buf, B * t.E, -7) and np.array_equal(out.cpu().numpy().reshape(B, t.E), nb.RM_Select_host(rm, cw)), name
        Lrx, acc0 = K.normal((B, t.E, V), 3 * N + q), K.normal((B, N, V), 5 * N + q)
        rxq, rxb = K.channel_output(nb, t, q, B, 7 * N + q, qam=True), K.channel_output(nb, t, q, B, 9 * N + q, qam=False)
        Lrxd, rxqd, rxbd = dev(Lrx), dev(rxq), dev(rxb)
        n = B * N * V
        calls = {
            "recover": (lambda o: lib.nbldpc_rm_recover(rm._h, q, P(Lrxd), B, llr, P(o), st), nb.RM_Recover_host(rm, q, Lrx)),
            "combine": (lambda o: lib.nbldpc_rm_combine(rm._h, q, P(Lrxd), B, llr, P(doned), P(o), st), nb.RM_Combine_host(rm, q, Lrx, acc0.copy(), done)),
            "qam recover": (lambda o: lib.nbldpc_rm_demodulate_qam_recover(rm._h, q, P(rxqd), P(cond), sig, B, llr, P(o), st),
                            nb.RM_Demodulate_Recover_host(rm, q, rxq, K.SIGMA, CONSTELLATION=K.constellation(q))),
            "qam combine": (lambda o: lib.nbldpc_rm_demodulate_qam_combine(rm._h, q, P(rxqd), P(cond), sig, B, llr, P(doned), P(o), st),
                            nb.RM_Demodulate_Combine_host(rm, q, rxq, K.SIGMA, acc0.copy(), done, CONSTELLATION=K.constellation(q))),
            "bpsk recover": (lambda o: lib.nbldpc_rm_demodulate_bpsk_recover(rm._h, q, P(rxbd), sig, B, llr, P(o), st),
                             nb.RM_Demodulate_Recover_host(rm, q, rxb, K.SIGMA)),
            "bpsk combine": (lambda o: lib.nbldpc_rm_demodulate_bpsk_combine(rm._h, q, P(rxbd), sig, B, llr, P(doned), P(o), st),
                             nb.RM_Demodulate_Combine_host(rm, q, rxb, K.SIGMA, acc0.copy(), done)),
        }
        for what, (call, want) in calls.items():
            buf, out = banded(n, 123.0, torch.float32)
            assert out.data_ptr() % 8 == 4
            if "combine" in what:
                out.copy_(dev(acc0).reshape(-1))
            assert call(out) == 0, (name, what)
            assert intact(buf, n, 123.0), (name, what)
            assert np.array_equal(u32(out).reshape(B, N, V), u32(want)), (name, what)


def test_shortened_encoder(nb, RateMatch, bds):
    """nbldpc_rm_encode_random: the words satisfy nbldpc_syndrome, their shortened symbols are 0, they equal the Python composition
    (the message rule, the forcing step, Encode), and the two refusals."""
    info = bds.info_positions
    sh = info[[0, 5, 11, 17, 23, 30, 41, 47]]
    par = np.setdiff1d(np.arange(bds.N), info)
    rm = RateMatch(bds.N, sh, par[:3])
    for B, first in ((1, 0), (3, 5), (257, 1000)):
        cw, msg = nb.PN_CodeWords(bds, 99, B, first_frame=first, want_msg=True, rate_match=rm)
        syn = nb.Syndrome(bds, cw)
        assert bool((syn["flag"] == 1).all()) and bool((syn["unsat"] == 0).all())
        cwh = cw.cpu().numpy()
        assert (cwh[:, sh] == 0).all() and (cwh >= 0).all() and (cwh < 64).all()
        want_msg = nb.RM_Force_Shortened_host(rm, info, nb.pn_messages(99, len(info), 64, B, first_frame=first))
        assert np.array_equal(msg.cpu().numpy(), want_msg) and np.array_equal(cwh[:, info], want_msg)
        assert torch.equal(cw, nb.Encode(bds, dev(want_msg)))
        plain, pmsg = nb.PN_CodeWords(bds, 99, B, first_frame=first, want_msg=True)
        assert np.array_equal(pmsg.cpu().numpy(), nb.pn_messages(99, len(info), 64, B, first_frame=first)) and not torch.equal(plain, cw)
        none = RateMatch(bds.N, (), par[:3])  # nothing shortened: the words of nbldpc_encode_random
        assert torch.equal(nb.PN_CodeWords(bds, 99, B, first_frame=first, rate_match=none), plain)
    with pytest.raises(nb.LdpcError, match="N=95"):
        nb.PN_CodeWords(bds, 99, 2, rate_match=RateMatch(95, (), ()))
    with pytest.raises(nb.LdpcError, match="information set"):
        nb.PN_CodeWords(bds, 99, 2, rate_match=RateMatch(bds.N, [int(par[0])], ()))


def noisy_llr(nb, code, B, snr, seed=(173, 173, 173), pn_seed=3):
    cw = nb.PN_CodeWords(code, pn_seed, B)
    sigma = nb.sigma_of(snr, code.rate)
    return nb.Demodulate(code, nb.AWGNChannel_GPU(np.array(seed, np.int32), sigma, code, cw, B), sigma)


@pytest.mark.parametrize("method", ("ems", "layered_tmm"))
def test_decode_result_does_not_depend_on_batch_mates(nb, bds, method):
    """What Simulation_HARQ_GPU's compact decoding rests on: the odd-indexed frames of a batch decoded alone give the DecodeOutput,
    iter_number and ok they had inside the batch.  129 frames at Eb/N0 = 2.5 dB and 128 at 0 dB over BPSK, interleaved: frames that
    converge at different iterations and frames that fail."""
    B = 257
    Lch = torch.cat([noisy_llr(nb, bds, 129, 2.5), noisy_llr(nb, bds, 128, 0.0, seed=(5, 6, 7), pn_seed=4)])[torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()].contiguous()
    dec = (lambda L: nb.Decoding_EMS(bds, L, 2, 2, 20)) if method == "ems" else (lambda L: nb.Decoding_TMM(bds, L, 20, layered=True))
    full = dec(Lch)
    idx = torch.arange(1, B, 2, device="cuda")
    part = dec(Lch.index_select(0, idx))
    assert len(torch.unique(full["iter_number"])) >= 3 and 0 < int(full["ok"].sum()) < B, "the input must hold frames of every kind"
    for k in ("DecodeOutput", "iter_number", "ok"):
        assert torch.equal(full[k].index_select(0, idx), part[k]), k


# ---- the simulations against loops of the unfused primitives --------------------------------------------------------------------------
def lcg_jump(seed, draws):
    from cuda_ldpc_amd import sharding
    return sharding.lcg_jump(seed, draws)


def pn_words(nb, code, rm, pn_seed, B, first):
    """The Python composition of nbldpc_rm_encode_random."""
    _, msg = nb.PN_CodeWords(code, pn_seed, B, first_frame=first, want_msg=True)
    forced = np.isin(code.info_positions, rm.shorten)
    msg[:, torch.from_numpy(forced).cuda()] = 0
    return nb.Encode(code, msg)


def transmit(nb, code, rm, seed, sigma, words):
    """select -> the per-frame BPSK channel at N := E -> the demodulator at N := E: Lrx [B, E, q-1], from the unfused primitives."""
    B = int(words.shape[0])
    length = types.SimpleNamespace(N=rm.E, m=code.m, q=code.q)
    rx = nb.AWGNChannel_GPU(seed, sigma, length, nb.RM_Select(rm, words), B)
    return nb.Demodulate_NQ(rm.E, code.q, rx, sigma)


MAX_FRAMES = 960  # every loop below is bounded: a point that misses its error count ends here and fails its assertions


def test_simulation_equals_a_loop_of_the_primitives(nb, RateMatch, bds):
    """Over BPSK, by EMS and by layered TMM: the final counters and the final seed, roll-back included.  The simulations have no
    rate-matched QAM or fading chain, so the 64-QAM and the 64-QAM + Fading(8, ...) cases do not exist."""
    from cuda_ldpc_amd.nb_simulation import NBSim, Simulation_GPU
    info = bds.info_positions
    rm = RateMatch(bds.N, info[[1, 9, 33]], range(88, 96))
    sigma = nb.sigma_of(2.0, (len(info) - rm.n_short) / rm.E)  # frame error rate about 0.8 (the CPU oracle on the same chain)
    batch, least_err, least_frames, pn_seed = 48, 7, 200, 5
    for method in (0, 3):
        seed, SIM = np.array([173, 173, 173], np.int32), NBSim()
        stop = Simulation_GPU(bds, seed, sigma, SIM, None, maxIT=20, batch=batch, leastErrorFrames=least_err, leastTestFrames=least_frames,
                              max_frames=MAX_FRAMES, device_channel=True, decoder_method=method, PN_Message=1, pn_seed=pn_seed, rate_match=rm)
        assert stop == 1, "the point must reach its error count inside the frame cap"
        # the loop
        rseed = np.array([173, 173, 173], np.int32)
        frames = nerr = nsym = nit = 0
        stopped = False
        for first in range(0, MAX_FRAMES, batch):
            words = pn_words(nb, bds, rm, pn_seed, batch, first)
            seed0 = rseed.copy()
            Lch = nb.RM_Recover(rm, 64, transmit(nb, bds, rm, rseed, sigma, words), 1.0e4)
            r = nb.Decoding_EMS(bds, Lch, 2, 2, 20) if method == 0 else nb.Decoding_TMM(bds, Lch, 20, layered=True)
            errs = (r["DecodeOutput"] != words).sum(1).cpu().numpy()
            its = r["iter_number"].cpu().numpy()
            for b in range(batch):
                frames, nit, nsym, nerr = frames + 1, nit + int(its[b]), nsym + int(errs[b]), nerr + (1 if errs[b] else 0)
                if nerr >= least_err and frames >= least_frames:
                    stopped = True
                    rseed = lcg_jump(seed0, 4 * rm.E * bds.m * (b + 1))
                    break
            if stopped:
                break
        assert stopped
        assert (SIM.num_Frames, SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration) == (frames, nerr, nsym, nit), method
        assert frames % batch != 0, "the point must stop inside a batch, so that the roll-back is exercised"
        assert seed.tolist() == rseed.tolist(), (method, "noise seed")


def harq_profiles(RateMatch, code, kind):
    sh = code.info_positions[[2, 40]]
    if kind == "chase2":
        return [RateMatch.circular(code.N, sh, (), 0, code.N - 2), RateMatch.circular(code.N, sh, (), 0, code.N - 2)]
    return [RateMatch.circular(code.N, sh, (), 0, 72), RateMatch.circular(code.N, sh, (), 72, 48), RateMatch.circular(code.N, sh, (), 24, 96)]


@pytest.mark.parametrize("rvs_kind", ("chase2", "ir3"))
def test_harq_equals_a_loop_of_the_primitives(nb, RateMatch, bds, rvs_kind):
    """Over BPSK: one Chase repeat, and three redundancy versions with different k0; compact and whole-batch decoding, EMS and layered
    TMM.  max_batches bounds every run."""
    from cuda_ldpc_amd.nb_simulation import Simulation_HARQ_GPU
    from cuda_ldpc_amd.simulation import HarqCounters
    rvs = harq_profiles(RateMatch, bds, rvs_kind)
    sigma = nb.sigma_of({"chase2": 1.5, "ir3": 3.0}[rvs_kind], (len(bds.info_positions) - 2) / rvs[0].E)
    B, batches, pn_seed, T = 96, 3, 11, len(rvs)
    got = {}
    for compact in (True, False):
        for method in (0, 3):
            seed, SIM = np.array([173, 173, 173], np.int32), HarqCounters()
            Simulation_HARQ_GPU(bds, seed, sigma, SIM, rvs, maxIT=20, batch=B, leastErrorFrames=10 ** 9, max_batches=batches, decoder_method=method,
                                PN_Message=1, pn_seed=pn_seed, compact=compact, log=None)
            got[compact, method] = (SIM.num_Frames, SIM.acked, SIM.undetected, SIM.never_acked, SIM.bits_sent, SIM.Total_Iteration, seed.tolist())
    for method in (0, 3):
        assert got[True, method] == got[False, method], "compact and whole-batch decoding differ"
        rseed = np.array([173, 173, 173], np.int32)
        acked_t, undet_t, never, sent, nit = [0] * T, [0] * T, 0, 0, 0
        for i in range(batches):
            words = pn_words(nb, bds, rvs[0], pn_seed, B, i * B)
            ok = torch.zeros(B, dtype=torch.int32, device="cuda")
            acked = torch.zeros(B, dtype=torch.bool, device="cuda")
            for t, rm in enumerate(rvs):  # every transmission draws for every frame, used or not
                Lrx = transmit(nb, bds, rm, rseed, sigma, words)
                live = ~acked
                if not bool(live.any()):
                    continue
                acc = nb.RM_Recover(rm, 64, Lrx, 1.0e4) if t == 0 else nb.RM_Combine(rm, 64, Lrx, acc, ok, 1.0e4)
                r = nb.Decoding_EMS(bds, acc, 2, 2, 20) if method == 0 else nb.Decoding_TMM(bds, acc, 20, layered=True)
                now = (r["ok"] != 0) & live
                wrong = (r["DecodeOutput"] != words).any(1)
                acked_t[t] += int(now.sum())
                undet_t[t] += int((now & wrong).sum())
                sent += rm.E * bds.m * int(live.sum())
                nit += int(r["iter_number"][live].sum())
                acked |= now
                ok = acked.to(torch.int32)
            never += int((~acked).sum())
        assert got[True, method] == (B * batches, acked_t, undet_t, never, sent, nit, rseed.tolist()), (rvs_kind, method)
        assert sum(acked_t[1:]) > 0 and acked_t[0] > 0, "the point must acknowledge frames at the first and at a later transmission"


def test_receive_routing_gives_the_same_bits(nb, RateMatch):
    """_rm_receive: the fused call and the composition it routes to in the one case that measured slower (combine, q = 256, one lap, a
    mask with no frame done) give the same bits, and the rule picks the composition exactly there."""
    from cuda_ldpc_amd.nb_simulation import _fused_is_faster, _rm_receive
    q, N, B = 256, 12, 5
    rm = RateMatch.circular(N, (), (11,), 3, 11)
    assert not _fused_is_faster(rm, q, True, 0) and _fused_is_faster(rm, q, True, 2) and _fused_is_faster(rm, q, False, 0)
    assert _fused_is_faster(rm, 64, True, 0) and _fused_is_faster(RateMatch.circular(N, (), (11,), 3, 22), q, True, 0)
    t = K.Tables(N, dict(shorten=(), puncture=(11,), k0=3, E=11))
    rx = dev(K.channel_output(nb, t, q, B, 77, qam=False))
    acc0 = dev(K.normal((B, N, q - 1), 78))
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    a = _rm_receive(rm, q, rx, K.SIGMA, 1.0e4, acc=acc0.clone(), done=done, n_done=0)
    b = _rm_receive(rm, q, rx, K.SIGMA, 1.0e4, acc=acc0.clone(), done=done, n_done=0, fused=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, acc0)


def test_sweeps_run_the_simulations_at_the_derived_rate(nb, RateMatch, bds):
    """sweep(rate_match=) and sweep_harq run Simulation_GPU / Simulation_HARQ_GPU at the sigma of the derived rate, (K' - n_short) / E
    (HARQ: the first transmission's E), with the seeds reset at every point.  Every run is bounded by max_frames / max_batches."""
    from cuda_ldpc_amd.nb_simulation import NBSim, Simulation_GPU, Simulation_HARQ_GPU, sweep, sweep_harq
    from cuda_ldpc_amd.simulation import HarqCounters
    info = bds.info_positions
    rm = RateMatch(bds.N, info[[1, 9]], range(88, 96))
    kw = dict(maxIT=20, batch=64, max_frames=128, device_channel=True, PN_Message=1, pn_seed=5, leastErrorFrames=10 ** 9)
    sims = sweep(bds, None, 2.0, 2.5, 0.5, log=None, rate_match=rm, **kw)
    assert [s.SNR for s in sims] == [2.0, 2.5]
    for s in sims:
        one, seed = NBSim(), np.array([173, 173, 173], np.int32)
        Simulation_GPU(bds, seed, nb.sigma_of(s.SNR, np.float32(len(info) - 2) / np.float32(rm.E)), one, None, rate_match=rm, **kw)
        assert (s.num_Frames, s.num_Error_Frames, s.num_Error_Bits, s.Total_Iteration) == (128, one.num_Error_Frames, one.num_Error_Bits, one.Total_Iteration)
    rvs = harq_profiles(RateMatch, bds, "ir3")
    hkw = dict(maxIT=20, batch=64, max_batches=2, PN_Message=1, pn_seed=5, leastErrorFrames=10 ** 9)
    hs = sweep_harq(bds, rvs, None, 3.0, 3.5, 0.5, log=None, **hkw)
    assert [h.SNR for h in hs] == [3.0, 3.5]
    for h in hs:
        one, seed = HarqCounters(), np.array([173, 173, 173], np.int32)
        Simulation_HARQ_GPU(bds, seed, nb.sigma_of(h.SNR, np.float32(len(info) - 2) / np.float32(72)), one, rvs, log=None, **hkw)
        assert (h.num_Frames, h.acked, h.undetected, h.never_acked, h.bits_sent) == (128, one.acked, one.undetected, one.never_acked, one.bits_sent)


@pytest.mark.parametrize("extra", (["--puncture", "88:96"], ["--shorten", "0:2", "--puncture", "88:96", "--method", "3"], ["--harq", "0:72,72:48,24:96"]),
                         ids=("puncture", "shorten_puncture_ltmm", "harq"))
def test_sweep_command_line_prints_rows(extra):
    """`sweep.py nb --device-channel --pn-message` with the new options prints one row per point (two batches of 64 frames each)."""
    import subprocess
    import sys
    from conftest import ROOT
    cmd = [sys.executable, os.path.join(ROOT, "sweep.py"), "nb", "--device-channel", "--pn-message", "--start", "2", "--stop", "2.5", "--step", "0.5",
           "--batch", "64", "--max-batches", "2"] + extra
    r = subprocess.run(cmd, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    rows = [line for line in out.splitlines() if line.startswith(" 2.")]
    assert r.returncode == 0 and len(rows) == 2 and all(int(row.split()[1]) == 128 for row in rows), out
