"""Binary HARQ without a GPU: circular profiles (bldpc_rm_create_circular) and the host statements of include/bldpc.h, "HARQ" --
recover and combine on a circular profile, channel + combine, frame gather and scatter -- against numpy loops that follow the header's
words, as bit patterns; the direction of the effect of combining on a decoder; the refusals of Simulation_HARQ_GPU; and the host code
as a stand-alone program (tests/cpp/harq_host_test.hip) under the address + undefined sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import qc_variant_cases as Q

SHORT_LLR = 1.0e4
# (N, shortened, punctured): the size of the rate-matching guard test with its kind of lists (ranges that start and end inside a run
# of 32 and remove a whole one, the last position), and a small one whose buffer of 60 is two runs of 32, the second ragged
SHAPES = {
    2301: (list(range(0, 8)) + [55], list(range(40, 50)) + list(range(60, 100)) + list(range(1200, 1207)) + [2300]),
    70: ([3, 40], [10, 11, 12, 60, 61, 69, 0, 33]),
}
K0S = ("0", "37", "Ncb-1")
ES = ("1", "Ncb-9", "Ncb", "Ncb+1", "2*Ncb+5", "8*Ncb")


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ncb_of(N):
    return N - len(SHAPES[N][0]) - len(SHAPES[N][1])


def val(expr, Ncb):
    return int(eval(expr, {"Ncb": Ncb}))


def np_buffer(N):
    keep = np.ones(N, bool)
    keep[SHAPES[N][0]] = False
    keep[SHAPES[N][1]] = False
    return np.flatnonzero(keep).astype(np.int32)


def np_combine(tx_pos, shorten, rx, acc, done, short_llr, fresh):
    """The header's words: every position's contributions in ascending e, np.float32 additions; fresh (recover) starts from the bits of
    the first sample and zeroes what has no contribution, otherwise the sum starts from acc and done columns are passed over."""
    out = acc.copy()
    live = np.ones(rx.shape[1], bool) if done is None else np.asarray(done) == 0
    seen = np.zeros(out.shape[0], bool)
    if fresh:
        out.view(np.uint32)[:] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for e, n in enumerate(tx_pos):
            if fresh and not seen[n]:
                out.view(np.uint32)[n] = rx.view(np.uint32)[e]
            else:
                out[n, live] = out[n, live] + rx[e, live]
            seen[n] = True
    out[np.ix_(np.asarray(shorten, np.int64), live)] = np.float32(short_llr)
    return out


def test_create_circular_refusals(C):
    import ctypes
    from cuda_ldpc_amd._lib import LdpcError, lib
    N = 2301
    sh, pu = SHAPES[N]
    Ncb = ncb_of(N)
    for k0, E, text in ((-1, 10, "k0=-1 outside"), (Ncb, 10, "k0=%d outside" % Ncb), (0, 0, "E=0"), (0, -3, "E=-3"),
                        (0, 8 * Ncb + 1, "more than 8 laps")):
        with pytest.raises(LdpcError, match=text):
            C.RateMatch.circular(N, sh, pu, k0, E)
    big = C.RateMatch.circular(N, sh, pu, Ncb - 1, 8 * Ncb)
    assert (big.E, big.laps, big.Ncb, big.k0) == (8 * Ncb, 8, Ncb, Ncb - 1)
    with pytest.raises(LdpcError, match=r"E=2097121 outside \[1, 2097120\]"):  # the launch grid; 8 laps would allow it
        C.RateMatch.circular(300000, (), (), 0, 2097121)
    # everything bldpc_rm_create refuses, through the new entry
    for kw, text in ((dict(shorten=[5, 2301]), "shortened position 2301 out of range"), (dict(puncture=[-1]), "punctured position -1 out of range"),
                     (dict(shorten=[7, 9, 7]), "shortened position 7 repeated"), (dict(shorten=[11], puncture=[12, 11]), "position 11 is in both lists"),
                     (dict(shorten=range(0, 1000), puncture=range(1000, N)), "nothing is transmitted")):
        with pytest.raises(LdpcError, match="bldpc_rm_create_circular: .*" + text):
            C.RateMatch.circular(N, kw.get("shorten", ()), kw.get("puncture", ()), 0, 10)
    with pytest.raises(LdpcError, match="N=0 outside"):
        C.RateMatch.circular(0, (), (), 0, 1)
    h = ctypes.c_void_p()
    assert lib.bldpc_rm_create_circular(N, None, 2, None, 0, 0, 5, ctypes.byref(h)) == -1 and b"null list with a non-zero count" in lib.bldpc_last_error()
    assert lib.bldpc_rm_create_circular(N, None, 0, None, 0, 0, 5, None) == -1
    assert lib.bldpc_rm_circ(None, None) == -1


@pytest.mark.parametrize("N", list(SHAPES))
def test_positions_laps_and_rate(C, N):
    sh, pu = SHAPES[N]
    buf, Ncb = np_buffer(N), ncb_of(N)
    lin = C.RateMatch(N, sh, pu)
    assert np.array_equal(lin.tx_pos, buf) and (lin.Ncb, lin.k0, lin.laps, lin.is_circular) == (Ncb, 0, 1, False)
    for k0 in (val(k, Ncb) for k in K0S):
        for E in (val(e, Ncb) for e in ES):
            rm = C.RateMatch.circular(N, sh, pu, k0, E)
            assert rm.tx_pos.dtype == np.int32 and np.array_equal(rm.tx_pos, buf[(k0 + np.arange(E)) % Ncb]), (k0, E)
            assert (rm.N, rm.E, rm.n_short, rm.n_punct, rm.Ncb, rm.k0, rm.laps) == (N, E, len(sh), len(pu), Ncb, k0, -(-E // Ncb))
            assert rm.rate(1920) == (1920 - len(sh)) / E and rm.is_circular
            assert not np.isin(rm.tx_pos, pu).any() and not np.isin(rm.tx_pos, sh).any()


@pytest.mark.parametrize("N", list(SHAPES))
def test_the_circular_profile_from_the_start_is_the_linear_one(C, N):
    sh, pu = SHAPES[N]
    lin, circ = C.RateMatch(N, sh, pu), C.RateMatch.circular(N, sh, pu, 0, ncb_of(N))
    assert np.array_equal(lin.tx_pos, circ.tx_pos) and lin.E == circ.E
    rng = np.random.default_rng(N)
    F = 5
    cw = rng.integers(0, 2 ** 31 - 1, (N, F)).astype(np.int32)
    assert np.array_equal(C.RM_Select_host(lin, cw), C.RM_Select_host(circ, cw))
    rx = rng.standard_normal((lin.E, F)).astype(np.float32)
    rx.reshape(-1)[:4] = np.array([-0.0, np.inf, 1e-42, np.nan], np.float32)
    rx.view(np.uint32).reshape(-1)[3] = 0x7FC12345
    assert np.array_equal(bits(C.RM_Recover_host(lin, rx, SHORT_LLR)), bits(C.RM_Recover_host(circ, rx, SHORT_LLR)))
    s1, s2 = np.array([173, 2001, 40000], np.int32), np.array([173, 2001, 40000], np.int32)
    cw &= 1
    cw[sh] = 0
    assert np.array_equal(bits(C.AWGNChannel_RM_CPU(lin, s1, 0.73, F, CodeWord=cw)), bits(C.AWGNChannel_RM_CPU(circ, s2, 0.73, F, CodeWord=cw)))
    assert np.array_equal(s1, s2)
    # combine takes both kinds
    a1 = rng.standard_normal((N, F)).astype(np.float32)
    a2 = a1.copy()
    done = np.array([0, 1, 0, 0, 1], np.int32)
    assert np.array_equal(bits(C.RM_Combine_host(lin, rx, a1, done)), bits(C.RM_Combine_host(circ, rx, a2, done)))


DONES = {"null": None, "none": lambda F: np.zeros(F, np.int32), "all": lambda F: np.ones(F, np.int32),
         "alternating": lambda F: (np.arange(F) % 2 * 7).astype(np.int32)}  # any non-zero value means done


@pytest.mark.parametrize("N", list(SHAPES))
@pytest.mark.parametrize("k0", K0S)
def test_recover_and_combine_against_numpy(C, N, k0):
    sh, pu = SHAPES[N]
    Ncb, F = ncb_of(N), 6
    k0 = val(k0, Ncb)
    for E in (val(e, Ncb) for e in ES):
        rm = C.RateMatch.circular(N, sh, pu, k0, E)
        rng = np.random.default_rng(E)
        rx = rng.standard_normal((E, F)).astype(np.float32)
        rx.reshape(-1)[:3] = np.array([-0.0, np.inf, 1e-42], np.float32)[:rx.size]
        once = np.flatnonzero(np.bincount(rm.tx_pos, minlength=N)[rm.tx_pos] == 1)
        if once.size:  # a NaN payload on a position with a single contribution: recover moves it as 32 bits
            rx.view(np.uint32)[once[-1], F - 1] = 0x7FC12345
        zero = np.zeros((N, F), np.float32)
        got = C.RM_Recover_host(rm, rx, SHORT_LLR)
        want = np_combine(rm.tx_pos, sh, rx, zero, None, SHORT_LLR, fresh=True)
        assert np.array_equal(bits(got), bits(want)), ("recover", k0, E)
        if once.size:
            assert bits(got)[rm.tx_pos[once[-1]], F - 1] == 0x7FC12345
        unreached = np.setdiff1d(np.arange(N), np.r_[rm.tx_pos, sh])
        assert not bits(got)[unreached].any() and not bits(got)[pu].any() and (got[sh] == np.float32(SHORT_LLR)).all()
        for name, mk in DONES.items():
            done = None if mk is None else mk(F)
            acc = rng.standard_normal((N, F)).astype(np.float32)
            acc.view(np.uint32)[:, 1] = 0x7FC0BEEF  # a NaN-payload sentinel column: done with "all" and "alternating"
            acc[sh] = 3.0  # a shortened row that does not hold short_llr yet is reset
            before = acc.copy()
            want = np_combine(rm.tx_pos, sh, rx, before, done, SHORT_LLR, fresh=False)
            assert C.RM_Combine_host(rm, rx, acc, done) is acc
            assert np.array_equal(bits(acc), bits(want)), ("combine", name, k0, E)
            live = np.ones(F, bool) if done is None else done == 0
            assert np.array_equal(bits(acc)[:, ~live], bits(before)[:, ~live]), "done columns keep their bits"
            assert np.array_equal(bits(acc)[unreached], bits(before)[unreached]), "rows without a contribution are unchanged"
            assert (acc[np.ix_(sh, live)] == np.float32(SHORT_LLR)).all()


def test_recover_starts_from_the_first_sample_not_from_zero(C):
    rm = C.RateMatch.circular(4, (), (), 0, 8)  # every position twice
    rx = np.full((8, 2), -0.0, np.float32)
    assert (bits(C.RM_Recover_host(rm, rx)) == 0x80000000).all(), "-0.0 + -0.0 = -0.0"
    acc = np.zeros((4, 2), np.float32)
    assert not bits(C.RM_Combine_host(rm, rx, acc)).any(), "(+0.0 + -0.0) + -0.0 = +0.0"
    rx[2, 0], rx[6, 0] = 2.0e38, 3.0e38  # position 2: the sum overflows to +inf in fp32, as stated; nothing is reordered or widened
    assert C.RM_Recover_host(rm, rx)[2, 0] == np.inf


@pytest.mark.parametrize("N", list(SHAPES))
def test_channel_and_channel_combine_host(C, N):
    from cuda_ldpc_amd import sharding
    sh, pu = SHAPES[N]
    Ncb, F = ncb_of(N), 5
    rng = np.random.default_rng(3)
    cw = rng.integers(0, 2, (N, F)).astype(np.int32)
    cw[sh] = 0
    start = [173, 2001, 40000]
    for k0, E in ((0, Ncb), (37, Ncb - 9), (Ncb - 1, Ncb + 1), (37, 2 * Ncb + 5)):
        rm = C.RateMatch.circular(N, sh, pu, k0, E)
        for word in (cw, None):
            tx = None if word is None else C.RM_Select_host(rm, word)
            assert word is None or np.array_equal(tx, word[rm.tx_pos])
            seed, ref = np.array(start, np.int32), np.array(start, np.int32)
            got = C.AWGNChannel_RM_CPU(rm, seed, 0.73, F, CodeWord=word, short_llr=SHORT_LLR)
            rx = C.AWGNChannel_CPU(ref, 0.73, E, F, CodeWord=tx)
            assert np.array_equal(bits(got), bits(C.RM_Recover_host(rm, rx, SHORT_LLR))) and np.array_equal(seed, ref)
            for name, mk in DONES.items():
                done = None if mk is None else mk(F)
                acc = got.copy()
                acc2 = got.copy()
                seed, ref = np.array(start, np.int32), np.array(start, np.int32)
                C.AWGNChannel_RM_Combine_CPU(rm, seed, 0.73, acc, done, CodeWord=word, short_llr=SHORT_LLR)
                C.RM_Combine_host(rm, C.AWGNChannel_CPU(ref, 0.73, E, F, CodeWord=tx), acc2, done, SHORT_LLR)
                assert np.array_equal(bits(acc), bits(acc2)), (name, k0, E)
                assert np.array_equal(seed, ref) and np.array_equal(seed, sharding.lcg_jump(start, 2 * E * F)), "also with every frame done"
                if name == "all":
                    assert np.array_equal(bits(acc), bits(got))


def test_frames_gather_and_scatter_host(C):
    from cuda_ldpc_amd._lib import LdpcError
    rng = np.random.default_rng(9)
    rows, F = 71, 37
    for dtype in (np.int32, np.float32):
        src = rng.integers(-2 ** 31, 2 ** 31 - 1, (rows, F)).astype(np.int32).view(dtype)
        for idx in ([0], [F - 1], [3, 4, 20, 36], list(range(F))):
            got = C.Frames_Gather_host(src, idx)
            assert got.dtype == dtype and np.array_equal(got.view(np.int32), src.view(np.int32)[:, idx])
            dst = np.full((rows, F), -7, np.int32).view(dtype)
            assert C.Frames_Scatter_host(got, idx, dst) is dst
            want = np.full((rows, F), -7, np.int32)
            want[:, idx] = src.view(np.int32)[:, idx]
            assert np.array_equal(dst.view(np.int32), want)
    it = np.arange(F, dtype=np.int32)
    assert np.array_equal(C.Frames_Gather_host(it, [1, 5]), [1, 5])  # a single row, as iters
    for bad in ([4, 3], [3, 3], [-1, 2], [0, F]):
        with pytest.raises(LdpcError, match="strictly ascending"):
            C.Frames_Gather_host(src, bad)
        with pytest.raises(LdpcError, match="strictly ascending"):
            C.Frames_Scatter_host(src[:, :2].copy(), bad, src.copy())
    with pytest.raises(LdpcError, match="Fa=0"):
        C.Frames_Gather_host(src, [])
    with pytest.raises(LdpcError, match="Fa=%d" % (F + 1)):
        C.Frames_Gather_host(src, list(range(F + 1)))


# ---- what combining does to a decoder -------------------------------------------------------------------------------------------
DIRECTION_SNR, DIRECTION_E = 2.7, 2250  # Es/N0 in dB and the length of the first transmission of J4_L24_Z96 (N = Ncb = 2304)


def qc_syndrome_bad(H, J, L, Z, D):
    """Frames of the hard bits D [>= N, F] with an unsatisfied check of the QC code with shifts H (what bldpc_syndrome flags 0)."""
    d = D[:L * Z].reshape(L, Z, -1).astype(np.int64)
    bad = np.zeros(d.shape[2], bool)
    for j in range(J):
        acc = np.zeros((Z, d.shape[2]), np.int64)
        for l in range(L):
            if H[j, l] >= 0:
                acc += np.roll(d[l], -int(H[j, l]), axis=0)
        bad |= (acc % 2).any(0)
    return bad


def random_codewords(C, H, J, L, Z, F, pn_seed):
    gen = C.generator_host(H, J, L, Z)
    K, info = gen["K_info"], gen["info_pos"]
    par = np.setdiff1d(np.arange(L * Z), info)
    msg = C.pn_messages(pn_seed, K, F)
    P = ((gen["P"][:, np.arange(K) // 64] >> (np.arange(K) % 64).astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    cw = np.zeros((L * Z, F), np.int32)
    cw[info] = msg
    cw[par] = (P @ msg.astype(np.int64)) % 2
    return cw


def test_the_direction_of_the_effect(C):
    """J4_L24_Z96, 256 random codewords (message stream 4242) over the host channel at Es/N0 2.7 dB from the seed (173, 173, 173), 50
    fixed iterations of normalised_host at alpha 1.0.  First transmission: k0 = 0, E = 2250 of the 2304 positions; second: k0 = 2250,
    E = 54, which brings the rest.  An erased position decides 0, so on the all-zero word every frame would look decoded: the words are
    random and a frame counts as unflagged when H d != 0, which is what Syndrome(into_flag_row=True) leaves in the flag row on the
    device.  Unflagged frames, from the host statements alone: 106 after the first transmission, 9 after combining the second into it,
    256 (every frame) when the second is decoded on its own."""
    _, H, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    H = np.asarray(H, np.int32).reshape(J, L)
    N, F, E = L * Z, 256, DIRECTION_E
    cw = random_codewords(C, H, J, L, Z, F, 4242)
    assert not qc_syndrome_bad(H, J, L, Z, cw).any()
    sigma = C.sigma_of(DIRECTION_SNR)
    first, second = C.RateMatch.circular(N, (), (), 0, E), C.RateMatch.circular(N, (), (), E, N - E)
    seed = np.array([173, 173, 173], np.int32)
    y1 = C.AWGNChannel_RM_CPU(first, seed, sigma, F, CodeWord=cw)
    seed2 = seed.copy()
    y12 = C.AWGNChannel_RM_Combine_CPU(second, seed, sigma, y1.copy(), CodeWord=cw)
    y2 = C.AWGNChannel_RM_CPU(second, seed2, sigma, F, CodeWord=cw)
    assert np.array_equal(bits(y12)[second.tx_pos], bits(y2)[second.tx_pos]) and np.array_equal(bits(y12)[first.tx_pos], bits(y1)[first.tx_pos])
    u = [int(qc_syndrome_bad(H, J, L, Z, C.normalised_host(H, J, L, Z, y, max_iter=50, alpha=1.0, want_app=False)["D"]).sum()) for y in (y1, y12, y2)]
    print("unflagged frames of %d: first alone %d, combined %d, second alone %d" % (F, *u))
    assert u[1] <= u[0] and u[1] < u[2]
    assert u == [106, 9, 256]


# ---- Python-side refusals ---------------------------------------------------------------------------------------------------------
def test_simulation_harq_refusals_come_before_the_device(C):
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU
    N0 = 2304

    class Code:  # what the refusals read
        N, K = N0, 1920
        info_positions = np.arange(1920, dtype=np.int32)

    seed = np.array([173, 173, 173], np.int32)
    rm = C.RateMatch.circular(N0, [0], [N0 - 1], 5, 2000)
    with pytest.raises(ValueError, match="at least one profile"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [])
    with pytest.raises(ValueError, match=r"rvs\[1\] is over N=100 positions"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [rm, C.RateMatch(100)])
    with pytest.raises(ValueError, match="PN_Message=1 needs exit_mode=EXIT_FIXED"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [rm], PN_Message=1, exit_mode=C.EXIT_PER_FRAME)
    with pytest.raises(ValueError, match="PN_Message=1 needs exit_mode=EXIT_FIXED"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [rm], PN_Message=1, exit_mode=C.EXIT_PER_FRAME, alpha=0.75)
    with pytest.raises(ValueError, match="parity position"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [C.RateMatch.circular(N0, [2000], (), 0, 100)], PN_Message=1)
    with pytest.raises(ValueError, match="EXIT_BATCH_GLOBAL depend on the batch"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [rm], exit_mode=C.EXIT_BATCH_GLOBAL)
    with pytest.raises(ValueError, match="shortens other positions"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [rm, C.RateMatch(N0, [1])])
    with pytest.raises(ValueError, match="short_llr"):
        Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [rm], short_llr=float("inf"))
    assert np.array_equal(seed, [173, 173, 173])


def test_harq_counters_and_sweep_spec():
    import sweep
    from cuda_ldpc_amd.simulation import HarqCounters, format_harq_row
    assert sweep.parse_harq("0:2000, 2000:304,100:4608") == [(0, 2000), (2000, 304), (100, 4608)]
    for bad in ("3", "0:0", "a:b", "0:3,", "-1:5"):
        with pytest.raises(ValueError):
            sweep.parse_harq(bad)
    S = HarqCounters(num_Frames=100, acked=[50, 30, 10], undetected=[0, 1, 0], never_acked=10, bits_sent=100 * 1000 + 50 * 500 + 20 * 500)
    r = S.ratios(800)
    assert r["FER"] == [1 - 50 / 100, 1 - 79 / 100, 1 - 89 / 100] and r["MeanTx"] == (50 + 60 + 30 + 30) / 100
    assert r["Throughput"] == 800 * 89 / 135000 and "1.700" in format_harq_row(S, 800)


def test_sweep_harq_takes_sigma_from_the_first_transmission(C, monkeypatch):
    from cuda_ldpc_amd import simulation

    class Code:
        N, K = 2304, 1920

    seen = []
    monkeypatch.setattr(simulation, "Simulation_HARQ_GPU", lambda code, seed, sigma, SIM, rvs, **kw: seen.append(sigma))
    rvs = [C.RateMatch.circular(2304, range(0, 24), (), 0, 2000), C.RateMatch.circular(2304, range(0, 24), (), 2000, 280)]
    simulation.sweep_harq(Code, rvs, 3.0, 3.0, 1.0, snrtype=0, log=None)
    simulation.sweep_harq(Code, rvs, 3.0, 3.0, 1.0, snrtype=1, log=None)
    assert seen == [C.sigma_of(3.0, 0, (1920 - 24) / 2000), C.sigma_of(3.0, 1)]


# ---- the host code under the host sanitizers, stand-alone -------------------------------------------------------------------------
def test_host_statements_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/harq_host_test.hip with the two units that hold the host statements, built with -fsanitize=address,undefined on the host
    side, as test_enc_shapes_cpu.py builds encoder_host_test.hip.  The program checks the statements against loops of its own and
    prints OK; a sanitizer report ends it with a non-zero status."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "cuda_ldpc_amd", "csrc")
    exe = str(tmp_path / "harq_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "harq_host_test.hip"),
                           os.path.join(csrc, "bldpc_ratematch.hip"), os.path.join(csrc, "bldpc_channel.hip"), "-o", exe], cwd=str(tmp_path))
    r = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert out.strip().split("\n")[-1].startswith("OK"), out
