"""Block fading on the GPU: the gains kernel, the two channels that apply them and the two demappers with receiver CSI against
their host statements and against the AWGN kernels at all-ones gains, at the smallest shapes at which they can still go wrong
(tests/fading_cases.py); the three sweep drivers with fading against loops of the primitives, cut in halves, compacted and not; and
the three drivers without fading against the counters they gave before fading existed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fading_cases as K
from fading_cases import IL_NONE, IL_ROWCOL, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def seed_of(t=K.FADE_SEED):
    return np.array(t, np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- gains ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Lc,F", K.GAIN_SHAPES)
def test_gains_against_host(C, S, Lc, F):
    from cuda_ldpc_amd import sharding
    sh, sd = seed_of(), seed_of()
    h = C.Fading_Gains_host(sh, Lc, S, F)
    d = C.Fading_Gains(sd, Lc, S, F)
    assert np.array_equal(sh, sd), "seeds equal the host's"
    assert d.shape == (F, S) and d.dtype == torch.float32
    s = torch.arange(S, device="cuda")
    assert same_bits(d, d[:, (s // Lc) * Lc]), "the block structure is exact on the device array"
    g = d.cpu().numpy()
    same = float((bits(g) == bits(h)).mean())
    print("gains (S=%d, Lc=%d, F=%d): %.2f %% bit-identical to the host, max |d - h| = %.3g" % (S, Lc, F, 100 * same, np.abs(g - h).max()))
    assert np.abs(g - h).max() < 1e-6
    if F * -(-S // Lc) >= 5000:  # enough draws for a share to mean something
        # measured: 79.89 % at (77, 1, 70), 79.76 % at (2304, 16, 257); the device's logf and sqrtf against the host's, without the
        # sine and the double arithmetic that round most of that away in the AWGN sample (91.5 % there).  The same margin of 1.5 points.
        assert same > 0.78, same
    if F > 1:  # two half batches with a jumped seed are one batch, device against device
        hF = F // 2
        s2 = seed_of()
        a = C.Fading_Gains(s2, Lc, S, hF)
        assert np.array_equal(s2, sharding.lcg_jump(K.FADE_SEED, hF * sharding.fading_draws_per_frame(S, Lc)))
        b = C.Fading_Gains(s2, Lc, S, F - hF)
        assert same_bits(torch.cat([a, b]), d) and np.array_equal(s2, sd)


# ---- BPSK channel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", K.BPSK_SHAPES)
def test_bpsk_channel(C, N, F):
    sigma = 0.7
    gain = C.Fading_Gains(seed_of(), 5, N, F)
    ones = torch.ones((F, N), dtype=torch.float32, device="cuda")
    cw = np.random.default_rng(N + F).integers(0, 2, (N, F)).astype(np.int32)
    for word in (None, cw):
        wd = None if word is None else dev(word)
        s1, s2, s3, s4 = (np.array([173, 173, 173], np.int32) for _ in range(4))
        a = C.AWGNChannel_GPU(s1, sigma, N, F, CodeWord=wd)
        b = C.AWGNChannel_Fading_GPU(s2, sigma, ones, N, F, CodeWord=wd)
        assert same_bits(a, b) and np.array_equal(s1, s2), "all-ones gains: the AWGN kernel's bits and seed"
        d = C.AWGNChannel_Fading_GPU(s3, sigma, gain, N, F, CodeWord=wd).cpu().numpy()
        h = C.AWGNChannel_Fading_CPU(s4, sigma, gain.cpu().numpy(), N, F, CodeWord=word)
        assert np.array_equal(s3, s4) and np.array_equal(s3, s1)
        assert (np.abs(d - h) <= 1e-6 * np.maximum(1.0, np.abs(h))).all(), np.abs(d - h).max()


# ---- QAM channel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns,q,F", K.QAM_SHAPES)
def test_qam_channel(C, Ns, q, F):
    sigma = 0.3
    con = K.con_of(C, q.bit_length() - 1)
    cond = dev(con)
    sym = np.random.default_rng(Ns + q).integers(0, q, (F, Ns)).astype(np.int32)
    symd = dev(sym)
    gain = C.Fading_Gains(seed_of(), 5, Ns, F)
    ones = torch.ones((F, Ns), dtype=torch.float32, device="cuda")
    s1, s2, s3, s4 = (np.array([173, 173, 173], np.int32) for _ in range(4))
    a = C.AWGNChannel_QAM_GPU(s1, sigma, symd, cond)  # nbldpc_awgn_channel_device_qam_frames
    b = C.AWGNChannel_QAM_Fading_GPU(s2, sigma, symd, cond, ones)
    assert same_bits(a, b) and np.array_equal(s1, s2)
    d = C.AWGNChannel_QAM_Fading_GPU(s3, sigma, symd, cond, gain).cpu().numpy()
    h = C.AWGNChannel_QAM_Fading_CPU(s4, sigma, sym, con, gain.cpu().numpy())
    assert np.array_equal(s3, s4) and np.array_equal(s3, s1)
    assert (np.abs(d - h) <= 1e-6 * np.maximum(1.0, np.abs(h))).all(), np.abs(d - h).max()


# ---- demapper -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m,F", K.DEMAP_SHAPES)
def test_demapper_against_host(C, N, m, F):
    rx, gain, con = K.demap_inputs(C, N, m, F, N * 10 + m)
    rxd, gd, cond = dev(rx), dev(gain), dev(con)
    ones = torch.ones_like(gd)
    for il in K.RULES:
        for scale in (1.0, 1.0 / (2 * 0.2 * 0.2)):
            got = C.Demodulate_QAM_Fading(rxd, gd, cond, scale, N, interleave=il)
            want = C.Demodulate_QAM_Fading_host(rx, gain, con, scale, N, interleave=il)
            assert got.shape == (N, F) and np.array_equal(bits(got.cpu().numpy()), bits(want)), (il, scale)
        assert same_bits(C.Demodulate_QAM_Fading(rxd, ones, cond, 12.5, N, interleave=il), C.Demodulate_QAM(rxd, cond, 12.5, N, interleave=il)), \
            "all-ones gains: the plain demapper's bits"


@pytest.mark.parametrize("N,m,F", [(383, 6, 65), (2301, 7, 63), (7, 3, 63)])
def test_demapper_writes_nothing_outside_its_output(C, N, m, F):
    from cuda_ldpc_amd._lib import check, lib
    rx, gain, con = K.demap_inputs(C, N, m, F, 5)
    rxd, gd, cond = dev(rx), dev(gain), dev(con)
    row = max(F, 64)
    buf = torch.full((row + N * F + row,), float("nan"), dtype=torch.float32, device="cuda")  # a row of guard values on either side
    guard = buf.view(torch.int32).clone()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for il in K.RULES:
        check(lib.bldpc_qam_demap_fading(p(rxd), p(gd), p(cond), 1 << m, ctypes.c_float(1.0), N, F, il, p(buf[row:]), st), "demap")
        got = buf.view(torch.int32)
        assert torch.equal(got[:row], guard[:row]) and torch.equal(got[row + N * F:], guard[row + N * F:])
        assert np.array_equal(bits(buf[row:row + N * F].view(N, F).cpu().numpy()), bits(C.Demodulate_QAM_Fading_host(rx, gain, con, 1.0, N, interleave=il)))


# ---- GF(q) demodulator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,N,B", K.NB_SHAPES)
def test_nb_demodulator(C, q, N, B):
    from cuda_ldpc_amd._lib import lib
    rng = np.random.default_rng(q + N + B)
    con = K.con_of(C, q.bit_length() - 1)
    gain = C.Fading_Gains_host(seed_of(), 5, N, B)
    gain.reshape(-1)[::7] = 1.0
    gain.reshape(-1)[3::11] = 0.0
    rx = (gain[:, :, None] * con[rng.integers(0, q, (B, N))] + rng.normal(0.0, 0.2, (B, N, 2))).astype(np.float32)
    rxd, gd, cond = dev(rx), dev(gain), dev(con)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.empty((B, N, q - 1), dtype=torch.float32, device="cuda")
    assert lib.nbldpc_demodulate_qam_fading_nq(N, q, p(rxd), p(gd), p(cond), ctypes.c_float(0.2), B, p(out), st) == 0
    assert np.array_equal(bits(out.cpu().numpy()), bits(K.np_nb_demod(rx, con, 0.2, gain)))
    plain = torch.empty_like(out)
    lib.nbldpc_demodulate_qam_nq.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p]
    assert lib.nbldpc_demodulate_qam_nq(N, q, p(rxd), p(cond), ctypes.c_float(0.2), B, p(plain), st) == 0
    assert lib.nbldpc_demodulate_qam_fading_nq(N, q, p(rxd), p(torch.ones_like(gd)), p(cond), ctypes.c_float(0.2), B, p(out), st) == 0
    assert same_bits(out, plain), "all-ones gains: nbldpc_demodulate_qam_nq's bits"


# ---- sweeps -------------------------------------------------------------------------------------------------------------------------
_codes = {}


def j4(C):
    if "j4" not in _codes:
        _codes["j4"] = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", "J4_L24_Z96_BlockH.txt"), 4, 24, 96)
    return _codes["j4"]


def gf64(C):
    from cuda_ldpc_amd import nbldpc as nb
    if "nb" not in _codes:
        nbd = os.path.join(ROOT, "data", "nb")
        mul, _, _ = nb.GFInitial(64, os.path.join(nbd, "GF", "Arith.Table.GF.64.txt"))
        _codes["nb"] = nb.NBCode(os.path.join(nbd, "BDS.576.288.GF.64.txt"), mul)
    return _codes["nb"]


def counters(SIM):
    return [SIM.num_Frames, SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]


SWEEP = dict(maxIT=25, max_batches=1, log=None, device_channel=True, PN_Message=1, pn_seed=7, schedule="layered", alpha=0.75)


def qam_case(C):
    code = j4(C)
    rm = C.RateMatch(code.N, list(range(0, 24)), list(range(2200, 2250)))
    sigma = float(np.sqrt(0.5 / 10 ** 2.0))  # Es/N0 = 20 dB: fading leaves a part of the frames failing
    return dict(n_QAM=64, CONSTELLATION=K.constellation(C, 64), interleave=IL_ROWCOL, rate_match=rm), sigma


def primitives(C, code, F, first_frame, noise, fade, Lc, sigma, qam):
    """One batch as a loop of the primitives: (counters, D)."""
    cw = C.PN_CodeWords(code, 7, F, first_frame=first_frame, rate_match=qam.get("rate_match"))
    if qam:
        rm, con = qam["rate_match"], dev(qam["CONSTELLATION"])
        Ns = K.n_sym(rm.E, 6)
        gain = C.Fading_Gains(fade, Lc, Ns, F)
        rx = C.AWGNChannel_QAM_Fading_GPU(noise, sigma, C.RM_Modulate_QAM(rm, cw, 6, interleave=IL_ROWCOL), con, gain)
        y = C.RM_Recover(rm, C.Demodulate_QAM_Fading(rx, gain, con, 1.0 / (2 * sigma * sigma), rm.E, interleave=IL_ROWCOL))
    else:
        gain = C.Fading_Gains(fade, Lc, code.N, F)
        y = C.AWGNChannel_Fading_GPU(noise, sigma, gain, code.N, F, CodeWord=cw)
    r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=25, alpha=0.75, length=code.K, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    D = r["D"]
    err, flag = (D[:code.K] != cw[:code.K]).sum(0), D[code.N]
    return [F, int(((err != 0) | (flag == 0)).sum()), int(err.sum()), int(r["iters"].sum()), int(((err != 0) & (flag == 1)).sum()),
            int(((err == 0) & (flag == 0)).sum())], D


@pytest.mark.parametrize("chain", ["bpsk", "qam64_rowcol_rm"])
def test_simulation_equals_a_loop_of_the_primitives_and_its_halves(C, chain, monkeypatch):
    from cuda_ldpc_amd import simulation
    code = j4(C)
    F, Lc = 130, 16
    qam, sigma = qam_case(C) if chain != "bpsk" else ({}, C.sigma_of(6.0))
    kept = []
    real = simulation.LDPC_Decoder_Layered_GPU
    monkeypatch.setattr(simulation, "LDPC_Decoder_Layered_GPU", lambda *a, **kw: kept.append(kw["D"]) or real(*a, **kw))
    noise, fad, SIM = np.array([173, 173, 173], np.int32), C.Fading(Lc), C.SimCounters()
    simulation.Simulation_GPU(code, noise, sigma, SIM, Num_Frames_OneTime=F, exit_mode=C.EXIT_PER_FRAME, fading=fad, **SWEEP, **qam)
    n2, f2 = np.array([173, 173, 173], np.int32), seed_of()
    want, D = primitives(C, code, F, 0, n2, f2, Lc, sigma, qam)
    print(chain, "counters", counters(SIM))
    assert counters(SIM) == want and 0 < want[1] < F, "every counter; the point has failing and passing frames"
    assert torch.equal(kept[0][:code.N], D[:code.N]) and np.array_equal(noise, n2) and np.array_equal(fad.seed, f2)
    # the same batch cut in two halves with jumped seeds: what two ranks of a sharded sweep do
    from cuda_ldpc_amd import sharding
    S = K.n_sym(qam["rate_match"].E, 6) if qam else code.N
    per_noise = 4 * S if qam else 2 * S
    per_fade = sharding.fading_draws_per_frame(S, Lc)
    tot = [0] * 6
    for first, count in (sharding.shard_frames(F, 2, r) for r in range(2)):
        c, _ = primitives(C, code, count, first, sharding.lcg_jump((173, 173, 173), first * per_noise), sharding.lcg_jump(K.FADE_SEED, first * per_fade),
                          Lc, sigma, qam)
        tot = [a + b for a, b in zip(tot, c)]
    assert tot == want
    # and the driver itself in two batches of half the size continues both streams
    if F % 2 == 0:
        noise, fad, SIM2 = np.array([173, 173, 173], np.int32), C.Fading(Lc), C.SimCounters()
        simulation.Simulation_GPU(code, noise, sigma, SIM2, Num_Frames_OneTime=F // 2, exit_mode=C.EXIT_PER_FRAME, fading=fad,
                                  **dict(SWEEP, max_batches=2), **qam)
        assert counters(SIM2) == counters(SIM) and np.array_equal(noise, n2) and np.array_equal(fad.seed, f2)


HARQ_PROFILES = [(0, 2160), (2160, 48), (500, 2300)]


@pytest.mark.parametrize("n_QAM", [2, 64])
def test_harq_compact_equals_not_compact_and_the_fading_seed_after(C, n_QAM):
    from cuda_ldpc_amd import sharding, simulation
    code = j4(C)
    F, Lc = 130, 16
    rvs = [C.RateMatch.circular(code.N, (), (), k0, E) for k0, E in HARQ_PROFILES]
    qam = dict(n_QAM=64, CONSTELLATION=K.constellation(C, 64), interleave=IL_ROWCOL) if n_QAM != 2 else {}
    sigma = float(np.sqrt(0.5 / 10 ** 2.0)) if qam else C.sigma_of(7.5)
    got = []
    for compact in (True, False):
        noise, fad, H, keep = np.array([173, 173, 173], np.int32), C.Fading(Lc), simulation.HarqCounters(), []
        simulation.Simulation_HARQ_GPU(code, noise, sigma, H, rvs, Num_Frames_OneTime=F, maxIT=25, exit_mode=C.EXIT_PER_FRAME, max_batches=1, log=None,
                                       PN_Message=1, pn_seed=7, schedule="layered", alpha=0.75, compact=compact, keep_D=keep, fading=fad, **qam)
        got.append(([H.num_Frames, H.acked, H.undetected, H.never_acked, H.bits_sent, H.Total_Iteration], keep[0], noise, fad.seed))
    print("HARQ n_QAM=%d counters" % n_QAM, got[0][0])
    assert got[0][0] == got[1][0] and torch.equal(got[0][1], got[1][1])
    assert 0 < got[0][0][1][0] < F, "the first transmission acknowledges some frames and leaves some"
    uses = [K.n_sym(E, 6) if qam else E for _, E in HARQ_PROFILES]
    draws = sum(sharding.fading_draws_per_frame(S, Lc) * F for S in uses)
    for g in got:
        assert np.array_equal(g[3], sharding.lcg_jump(K.FADE_SEED, draws)), "the fading seed after the batch: the jump by sum_t nb_t * F"
        assert np.array_equal(g[2], sharding.lcg_jump((173, 173, 173), sum((4 if qam else 2) * S * F for S in uses)))


def test_nb_simulation_equals_a_loop_of_the_primitives(C):
    from cuda_ldpc_amd import nb_simulation as NS
    from cuda_ldpc_amd import nbldpc as nb
    code = gf64(C)
    con = K.constellation(C, 64)
    B, Lc = 70, 16
    sigma = nb.sigma_of(14.0, code.rate, 0, 64)
    noise, fad, SIM = np.array([173, 173, 173], np.int32), C.Fading(Lc), NS.NBSim(14.0)
    NS.Simulation_GPU(code, noise, sigma, SIM, None, maxIT=20, batch=B, max_frames=B, device_channel=True, CONSTELLATION=con, PN_Message=1, pn_seed=7,
                      fading=fad)
    n2, f2, cond = np.array([173, 173, 173], np.int32), seed_of(), dev(con)
    cw = nb.PN_CodeWords(code, 7, B)
    gain = C.Fading_Gains(f2, Lc, code.N, B)
    rx = nb.AWGNChannel_Fading_GPU(n2, sigma, code, cw, gain, cond)
    assert same_bits(rx, C.AWGNChannel_QAM_Fading_GPU(np.array([173, 173, 173], np.int32), sigma, cw, cond, gain)), "the shared QAM channel"
    r = nb.Decoding_EMS(code, nb.Demodulate_QAM_Fading(code, rx, gain, sigma, cond), 2, 2, 20)
    err = (r["DecodeOutput"] != cw).sum(1)
    want = [B, int((err != 0).sum()), int(err.sum()), int(r["iter_number"].sum())]
    got = [SIM.num_Frames, SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration]
    print("NB counters", got)
    assert got == want and 0 < want[1] < B
    assert np.array_equal(noise, n2) and np.array_equal(fad.seed, f2)
    # one word for all frames: expanded to [B, N], the draws where the per-frame channel puts them
    word = cw[0].cpu().numpy()
    noise, fad, SIM = np.array([173, 173, 173], np.int32), C.Fading(Lc), NS.NBSim(14.0)
    NS.Simulation_GPU(code, noise, sigma, SIM, word, maxIT=20, batch=B, max_frames=B, device_channel=True, CONSTELLATION=con, fading=fad)
    rx1 = nb.AWGNChannel_Fading_GPU(np.array([173, 173, 173], np.int32), sigma, code, cw[:1].expand(B, code.N).contiguous(), gain, cond)
    r = nb.Decoding_EMS(code, nb.Demodulate_QAM_Fading(code, rx1, gain, sigma, cond), 2, 2, 20)
    err = (r["DecodeOutput"] != cw[:1]).sum(1)
    assert [SIM.num_Frames, SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration] == [B, int((err != 0).sum()), int(err.sum()),
                                                                                                int(r["iter_number"].sum())]


def test_without_fading_the_drivers_count_what_they_counted_before(C):
    """fading=None takes the code path from before fading existed.  The numbers were taken by running the commit before this feature on
    an MI355X: one fixed seed per driver."""
    from cuda_ldpc_amd import nb_simulation as NS
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd import simulation
    code = j4(C)
    con = K.constellation(C, 64)
    seed, SIM = np.array([173, 173, 173], np.int32), C.SimCounters()
    simulation.Simulation_GPU(code, seed, C.sigma_of(2.5), SIM, Num_Frames_OneTime=130, exit_mode=C.EXIT_PER_FRAME, fading=None, **SWEEP)
    assert counters(SIM) == [130, 3, 85, 829, 0, 0] and seed.tolist() == [31684, 14901, 55962]
    rvs = [C.RateMatch.circular(code.N, (), (), k0, E) for k0, E in HARQ_PROFILES]
    seed, H = np.array([173, 173, 173], np.int32), simulation.HarqCounters()
    simulation.Simulation_HARQ_GPU(code, seed, nb.sigma_of(11.0, rvs[0].rate(code.K), 0, 64), H, rvs, Num_Frames_OneTime=130, maxIT=25,
                                   exit_mode=C.EXIT_PER_FRAME, max_batches=1, log=None, PN_Message=1, pn_seed=7, schedule="layered", alpha=0.75,
                                   n_QAM=64, CONSTELLATION=con, interleave=IL_ROWCOL, fading=None)
    assert [H.num_Frames, H.acked, H.undetected, H.never_acked, H.bits_sent, H.Total_Iteration] == [130, [49, 77, 4], [0, 0, 0], 0, 293888, 3238]
    assert seed.tolist() == [9478, 10129, 37199]
    ncode = gf64(C)
    seed, N = np.array([173, 173, 173], np.int32), NS.NBSim(11.0)
    NS.Simulation_GPU(ncode, seed, nb.sigma_of(11.0, ncode.rate, 0, 64), N, None, maxIT=20, batch=70, max_frames=70, device_channel=True,
                      CONSTELLATION=con, PN_Message=1, pn_seed=7, fading=None)
    assert [N.num_Frames, N.num_Error_Frames, N.num_Error_Bits, N.Total_Iteration] == [70, 42, 3430, 996] and seed.tolist() == [25324, 22829, 59548]
