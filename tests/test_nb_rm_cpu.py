"""Rate matching over GF(q) symbol vectors on the host (no GPU): every host statement of include/nbldpc.h, "rate matching", against the
numpy restatement of tests/nb_rm_cases.py, exactly, over the shared table; the fused host twins against their compositions; every
refusal in C and in Python; the forcing rule of the shortened encoder; the host statements as a stand-alone program under the address +
undefined sanitizers; and three conditions on the inputs of the decode-level use, judged by the CPU oracle alone."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import nb_rm_cases as K
from conftest import DATA

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


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


CASES = [(N, name) for N in K.NS for name in K.profiles(N)]


@pytest.mark.parametrize("N,name", CASES, ids=["N%d-%s" % c for c in CASES])
def test_profile_tables_and_select(nb, RateMatch, N, name):
    spec = K.profiles(N)[name]
    t, rm = K.Tables(N, spec), K.make_rm(RateMatch, N, spec)
    assert (rm.N, rm.E, rm.Ncb, rm.k0) == (t.N, t.E, t.Ncb, t.k0) and np.array_equal(rm.tx_pos, t.tx_pos)
    assert max(len(c) for c in t.contrib) == rm.laps <= 8
    for B in (1, 3):
        cw = np.random.default_rng(N + B).integers(0, 256, size=(B, N)).astype(np.int32)
        assert np.array_equal(nb.RM_Select_host(rm, cw), K.np_select(t, cw))


@pytest.mark.parametrize("q", K.QS)
@pytest.mark.parametrize("N,name", CASES, ids=["N%d-%s" % c for c in CASES])
def test_recover_and_combine_host(nb, RateMatch, N, name, q):
    spec = K.profiles(N)[name]
    t, rm = K.Tables(N, spec), K.make_rm(RateMatch, N, spec)
    V, B = q - 1, 3
    for Lrx in (K.normal((B, t.E, V), 7 * N + q), K.special_lrx(t, V, B, 9 * N + q)):
        got = nb.RM_Recover_host(rm, q, Lrx, K.SHORT_LLR)
        assert np.array_equal(u32(got), u32(K.np_receive(t, V, Lrx))), "recover"
        for mname, done in K.done_masks(B).items():
            acc0 = K.normal((B, N, V), 11 * N + q)
            u32(acc0)[1, N // 2, V // 2] = K.NAN_PAYLOAD  # frame 1 is done under "one" and "alternating": the payload must stay
            acc = acc0.copy()
            nb.RM_Combine_host(rm, q, Lrx, acc, done, K.SHORT_LLR)
            want = K.np_receive(t, V, Lrx, acc=acc0, done=done)
            # NaN + x (the two planted NaNs, where their frame is live): a NaN on both sides whose payload is not pinned
            same = (u32(acc) == u32(want)) | (np.isnan(acc) & np.isnan(want))
            assert same.all() and np.isnan(acc).sum() <= 2, "combine under done=%s" % mname
            if done is not None:
                assert np.array_equal(u32(acc)[done != 0], u32(acc0)[done != 0]), "a done frame keeps every bit"


@pytest.mark.parametrize("q", K.QS)
@pytest.mark.parametrize("N", K.NS)
def test_demodulate_host_is_the_stated_expression(nb, N, q):
    B = 3
    rx = K.normal((B, N, 2), 3 * N + q)
    con = K.constellation(q)
    assert np.array_equal(u32(nb.Demodulate_NQ_host(N, q, rx, K.SIGMA, CONSTELLATION=con)), u32(K.np_demod_qam(rx, con, K.SIGMA)))
    m = q.bit_length() - 1
    rxb = K.normal((B, N * m), 5 * N + q)
    assert np.array_equal(u32(nb.Demodulate_NQ_host(N, q, rxb, K.SIGMA)), u32(K.np_demod_bpsk(rxb, q, K.SIGMA)))


@pytest.mark.parametrize("qam", (True, False), ids=("qam", "bpsk"))
@pytest.mark.parametrize("q", K.QS)
@pytest.mark.parametrize("N,name", CASES, ids=["N%d-%s" % c for c in CASES])
def test_fused_host_twins_are_their_compositions(nb, RateMatch, N, name, q, qam):
    spec = K.profiles(N)[name]
    t, rm = K.Tables(N, spec), K.make_rm(RateMatch, N, spec)
    V, B = q - 1, 3
    con = K.constellation(q) if qam else None
    rx = K.channel_output(nb, t, q, B, 13 * N + q, qam=qam)
    Lrx = nb.Demodulate_NQ_host(t.E, q, rx, K.SIGMA, CONSTELLATION=con)
    assert np.array_equal(u32(Lrx), u32(K.np_demod_qam(rx, con, K.SIGMA) if qam else K.np_demod_bpsk(rx, q, K.SIGMA)))
    got = nb.RM_Demodulate_Recover_host(rm, q, rx, K.SIGMA, K.SHORT_LLR, CONSTELLATION=con)
    assert np.array_equal(u32(got), u32(nb.RM_Recover_host(rm, q, Lrx, K.SHORT_LLR)))
    assert np.array_equal(u32(got), u32(K.np_receive(t, V, Lrx)))
    for mname, done in K.done_masks(B).items():
        acc0 = K.normal((B, N, V), 17 * N + q)
        a, b = acc0.copy(), acc0.copy()
        nb.RM_Demodulate_Combine_host(rm, q, rx, K.SIGMA, a, done, K.SHORT_LLR, CONSTELLATION=con)
        nb.RM_Combine_host(rm, q, Lrx, b, done, K.SHORT_LLR)
        assert np.array_equal(u32(a), u32(b)) and np.array_equal(u32(a), u32(K.np_receive(t, V, Lrx, acc=acc0, done=done))), mname


# ---- the shortened encoder's forcing rule ---------------------------------------------------------------------------------------------
def test_forcing_rule_against_pn_messages(nb, RateMatch):
    H = nb.NBMatrix(os.path.join(NBD, "BDS.576.288.GF.64.txt"))
    mul, _, _ = nb.GFInitial(64, os.path.join(NBD, "GF", "Arith.Table.GF.64.txt"))
    H.TableMultiply = mul
    info = nb.generator_host(H)["info_pos"]
    sh = info[[0, 3, 7, len(info) - 1]]
    pu = np.setdiff1d(np.arange(H.N), info)[:5]  # punctured positions play no part
    spec = dict(shorten=tuple(int(x) for x in sh), puncture=tuple(int(x) for x in pu), k0=0, E=None)
    rm, t = K.make_rm(RateMatch, H.N, spec), K.Tables(H.N, spec)
    msg = nb.pn_messages(12345, len(info), 64, 9, first_frame=4)
    got = nb.RM_Force_Shortened_host(rm, info, msg)
    want = K.np_force(t, info, msg)
    assert np.array_equal(got, want)
    forced = np.isin(info, sh)
    assert forced.sum() == 4 and (got[:, forced] == 0).all() and np.array_equal(got[:, ~forced], msg[:, ~forced]) and (msg[:, forced] != 0).any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_c(nb, RateMatch):
    from cuda_ldpc_amd._lib import lib
    rm = K.make_rm(RateMatch, 7, K.profiles(7)["linear"])
    q, B, V = 4, 2, 3
    f = np.zeros(B * 96 * 8, np.float32)  # large enough for every shape below; a refused call touches nothing anyway
    i = np.zeros(B * 96, np.int32)
    g, j = f.copy(), i.copy()  # outputs of the good calls
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fl = ctypes.c_float
    ok_llr, sig = fl(1e4), fl(0.7)
    host = {  # name -> (arguments of a good call, indices of the pointers that must not be null, index of q, of B, of short_llr, of sigma)
        "nbldpc_rm_select_host": ([rm._h, P(i), B, P(j)], (0, 1, 3), None, 2, None, None),
        "nbldpc_rm_recover_host": ([rm._h, q, P(f), B, ok_llr, P(g)], (0, 2, 5), 1, 3, 4, None),
        "nbldpc_rm_combine_host": ([rm._h, q, P(f), B, ok_llr, None, P(g)], (0, 2, 6), 1, 3, 4, None),
        "nbldpc_rm_demodulate_qam_recover_host": ([rm._h, q, P(f), P(f), sig, B, ok_llr, P(g)], (0, 2, 3, 7), 1, 5, 6, 4),
        "nbldpc_rm_demodulate_qam_combine_host": ([rm._h, q, P(f), P(f), sig, B, ok_llr, None, P(g)], (0, 2, 3, 8), 1, 5, 6, 4),
        "nbldpc_rm_demodulate_bpsk_recover_host": ([rm._h, q, P(f), sig, B, ok_llr, P(g)], (0, 2, 6), 1, 4, 5, 3),
        "nbldpc_rm_demodulate_bpsk_combine_host": ([rm._h, q, P(f), sig, B, ok_llr, None, P(g)], (0, 2, 7), 1, 4, 5, 3),
    }
    # the device entry points take the same arguments and a stream: every refusal comes before anything touches the device
    table = dict(host)
    for name, (args, ptrs, iq, iB, il, isg) in host.items():
        table[name[:-5]] = (args + [None], ptrs, iq, iB, il, isg)
    for name, (args, ptrs, iq, iB, il, isg) in table.items():
        fn = getattr(lib, name)
        if name.endswith("_host"):
            assert fn(*args) == 0, name + ": the good call"

        def refused(idx, val, why):
            a = list(args)
            a[idx] = val
            assert fn(*a) == EINVAL, "%s: %s" % (name, why)
            assert nb.lib.nbldpc_last_error(), name
        for p in ptrs:
            refused(p, None, "null pointer at %d" % p)
        for bad in (0, -1):
            refused(iB, bad, "B=%d" % bad)
        if iq is not None:
            for bad in (0, 1, 3, 6, 48, 512, -4):
                refused(iq, bad, "q=%d" % bad)
        if il is not None:
            for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
                refused(il, fl(bad), "short_llr=%r" % bad)
        if isg is not None:
            for bad in (0.0, -0.5, float("nan")):
                refused(isg, fl(bad), "sigma=%r" % bad)
    # N * V beyond 65535 * 1024 entries per frame: N = 300000, q = 256 -> 76 500 000
    big = RateMatch(300000)
    assert lib.nbldpc_rm_recover_host(big._h, 256, P(f), 1, ok_llr, P(f)) == EINVAL and b"67107840" in nb.lib.nbldpc_last_error()
    assert lib.nbldpc_rm_recover(big._h, 256, P(f), 1, ok_llr, P(f), None) == EINVAL
    assert lib.nbldpc_rm_demodulate_qam_combine(big._h, 256, P(f), P(f), sig, 1, ok_llr, None, P(f), None) == EINVAL
    wide = RateMatch.circular(40000, (), (), 0, 8 * 40000)  # E * V beyond it while N * V is not
    assert lib.nbldpc_rm_recover_host(wide._h, 256, P(f), 1, ok_llr, P(f)) == EINVAL
    # the forcing step and the encoder
    info = np.arange(4, dtype=np.int32)
    assert lib.nbldpc_rm_force_shortened_host(rm._h, P(info), 4, B, P(i)) == 0
    for a in ([None, P(info), 4, B, P(i)], [rm._h, None, 4, B, P(i)], [rm._h, P(info), 4, B, None], [rm._h, P(info), 0, B, P(i)],
              [rm._h, P(info), 4, 0, P(i)], [rm._h, P(np.array([0, 1, 2, 7], np.int32)), 4, B, P(i)]):
        assert lib.nbldpc_rm_force_shortened_host(*a) == EINVAL
    for a in ([None, rm._h, 1, 0, B, P(i), P(i), None], ):  # without a device no code object exists: the null code is what can be asked here
        assert lib.nbldpc_rm_encode_random(*a) == EINVAL
    for name in ("nbldpc_demodulate_qam_nq_host", "nbldpc_demodulate_bpsk_nq_host"):
        tail = [P(f), sig, B, P(g)]
        good = [7, q, P(f)] + tail if "qam" in name else [7, q] + tail
        assert getattr(lib, name)(*good) == 0
        for idx, bad in ((0, 0), (1, 3), (1, 512), (2, None), (len(good) - 1, None), (len(good) - 2, 0), (len(good) - 3, fl(0.0))):
            a = list(good)
            a[idx] = bad
            assert getattr(lib, name)(*a) == EINVAL, (name, idx)


def test_refusals_in_python(nb, RateMatch):
    rm = K.make_rm(RateMatch, 7, K.profiles(7)["linear"])
    q, B, V = 4, 2, 3
    Lrx, acc, cw = np.zeros((B, rm.E, V), np.float32), np.zeros((B, 7, V), np.float32), np.zeros((B, 7), np.int32)
    with pytest.raises(ValueError):
        nb.RM_Select_host(rm, cw[:, :6])
    with pytest.raises(ValueError):
        nb.RM_Recover_host(rm, q, Lrx[:, :-1])
    with pytest.raises(ValueError):
        nb.RM_Recover_host(rm, 6, Lrx)
    with pytest.raises(ValueError):
        nb.RM_Combine_host(rm, q, Lrx, acc[:1])
    with pytest.raises(ValueError):
        nb.RM_Combine_host(rm, q, Lrx, acc.astype(np.float64))
    with pytest.raises(ValueError):
        nb.RM_Combine_host(rm, q, Lrx, acc, done=np.zeros(B + 1, np.int32))
    with pytest.raises(ValueError):
        nb.RM_Demodulate_Recover_host(rm, q, np.zeros((B, rm.E, 2), np.float32), 0.7, CONSTELLATION=np.zeros((8, 2), np.float32))
    with pytest.raises(ValueError):
        nb.RM_Demodulate_Recover_host(rm, q, np.zeros((B, rm.E * 3), np.float32), 0.7)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(nb.LdpcError):
            nb.RM_Recover_host(rm, q, Lrx, bad)
        for dev_call in (lambda: nb.RM_Recover(rm, q, None, bad), lambda: nb.RM_Demodulate_Recover(rm, q, None, 0.7, bad)):
            with pytest.raises(ValueError):  # the tensor checks come first: nothing reaches the device
                dev_call()


# ---- the host statements under the host sanitizers, stand-alone -----------------------------------------------------------------------
def hash32(i):
    h = (np.asarray(i, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return h.astype(np.uint32)


def gen_floats(n, salt):
    h = hash32((np.arange(n, dtype=np.uint64) + np.uint64(salt)) & np.uint64(0xFFFFFFFF))
    return (((h >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -22)).astype(np.float32)


def gen_ints(n, salt, q):
    return (hash32((np.arange(n, dtype=np.uint64) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)) % np.uint32(q)).astype(np.int32)


def fnv64(*arrays):
    h = 0xcbf29ce484222325
    for a in arrays:
        for byte in np.ascontiguousarray(a).tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def rm_exe(tmp_path_factory):
    """tests/cpp/nb_rm_host_test.hip, built as test_quant_cpu.py builds quant_host_test.hip."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("nb_rm_host")
    exe = str(tmp / "nb_rm_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "nb_rm_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("N,name,q", [(7, "linear", 4), (7, "circ_8laps", 16), (96, "circ_twice", 64), (96, "circ_short", 256), (7, "circ_one", 2)],
                         ids=lambda v: str(v))
def test_host_statements_stand_alone(nb, RateMatch, rm_exe, N, name, q):
    spec = K.profiles(N)[name]
    t, rm = K.Tables(N, spec), K.make_rm(RateMatch, N, spec)
    B, V, m = 5, q - 1, q.bit_length() - 1
    cw = gen_ints(B * N, 11, q).reshape(B, N)
    done = (np.arange(B) & 1).astype(np.int32)
    Lrx, acc0 = gen_floats(B * t.E * V, 101).reshape(B, t.E, V), gen_floats(B * N * V, 202).reshape(B, N, V)
    rxq, rxb, con = gen_floats(B * t.E * 2, 303).reshape(B, t.E, 2), gen_floats(B * t.E * m, 404).reshape(B, t.E * m), gen_floats(q * 2, 505).reshape(q, 2)
    outs = [nb.RM_Select_host(rm, cw), nb.RM_Recover_host(rm, q, Lrx), nb.RM_Combine_host(rm, q, Lrx, acc0.copy(), done),
            nb.RM_Demodulate_Recover_host(rm, q, rxq, 0.7, CONSTELLATION=con), nb.RM_Demodulate_Combine_host(rm, q, rxq, 0.7, acc0.copy(), done, CONSTELLATION=con),
            nb.RM_Demodulate_Recover_host(rm, q, rxb, 0.7), nb.RM_Demodulate_Combine_host(rm, q, rxb, 0.7, acc0.copy(), None)]
    Kinfo = N - N // 3
    outs.append(nb.RM_Force_Shortened_host(rm, np.arange(Kinfo, dtype=np.int32), gen_ints(B * Kinfo, 606, q).reshape(B, Kinfo)))
    args = [N, q, B, 0 if spec["E"] is None else 1, spec["k0"], spec["E"] or 0, len(spec["shorten"]), *spec["shorten"], len(spec["puncture"]), *spec["puncture"]]
    r = subprocess.run([rm_exe] + [str(a) for a in args], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert int(out.strip().split("\n")[-1], 16) == fnv64(*outs), "the stand-alone program and the library differ"


# ---- decode-level sanity: conditions on the inputs, judged by the CPU oracle alone ----------------------------------------------------
@pytest.fixture(scope="module")
def bds(nb, orc):
    """BDS.576.288.GF.64 over 64-QAM at Eb/N0 = 11 dB: 100 random codewords from the host generator and two transmissions of each
    through the host channel (one noise stream: frames 0..99 are the first transmission, 100..199 the second)."""
    path, gf = os.path.join(NBD, "BDS.576.288.GF.64.txt"), os.path.join(NBD, "GF", "Arith.Table.GF.64.txt")
    H = nb.NBMatrix(path)
    mul, _, _ = nb.GFInitial(64, gf)
    H.TableMultiply = mul
    gen = nb.generator_host(H)
    con = K.constellation(64)
    sigma = nb.sigma_of(11.0, H.rate, 0, 64)

    def encode(msg):
        m64, P = mul.astype(np.int64), gen["P"].astype(np.int64)
        cw = np.zeros((msg.shape[0], H.N), np.int64)
        cw[:, gen["info_pos"]] = msg
        cw[:, np.setdiff1d(np.arange(H.N), gen["info_pos"])] = np.bitwise_xor.reduce(m64[msg[:, None, :].astype(np.int64), P[None, :, :]], axis=2)
        return cw.astype(np.int32)

    def channel(words, seed):
        length = lambda E: type("Len", (), dict(N=E, m=6))  # noqa: E731
        return np.stack([nb.AWGNChannel_CPU(seed, sigma, length(words.shape[1]), w, CONSTELLATION=con) for w in words])

    return dict(H=H, oc=orc.NBCode(path, gf), gen=gen, con=con, sigma=sigma, encode=encode, channel=channel, B=100)


def frame_errors(orc, s, Lch, cw):
    return int((orc.nb_ems_decode_batch(s["oc"], Lch)["out"] != cw).any(axis=1).sum())


def test_oracle_shortened_positions_decode_to_zero(nb, RateMatch, orc, bds):
    """Seen: 100 frames, 800 shortened symbols, all decoded to 0 (frame errors of the shortened code: see the assert message on change)."""
    s, info = bds, bds["gen"]["info_pos"]
    sh = info[[0, 5, 11, 17, 23, 30, 41, 47]]
    rm = RateMatch(s["H"].N, sh, ())
    msg = nb.RM_Force_Shortened_host(rm, info, nb.pn_messages(7, len(info), 64, s["B"]))
    cw = s["encode"](msg)
    assert (cw[:, sh] == 0).all()
    rx = s["channel"](nb.RM_Select_host(rm, cw), np.array([173, 173, 173], np.int32))
    Lch = nb.RM_Demodulate_Recover_host(rm, 64, rx, s["sigma"], K.SHORT_LLR, CONSTELLATION=s["con"])
    out = orc.nb_ems_decode_batch(s["oc"], Lch)["out"]
    assert (out[:, sh] == 0).all(), "a shortened position decoded to a non-zero symbol"


def test_oracle_puncturing_costs_and_chase_combining_gains(nb, RateMatch, orc, bds):
    """Seen at Eb/N0 = 11 dB (sigma 0.11506), 100 frames, seeds 173/173/173, message seed 7: the mother code 60 frame errors, 8 symbols
    punctured (88..95) on the same noise 85, two Chase transmissions combined 0."""
    s = bds
    N = s["H"].N
    cw = s["encode"](nb.pn_messages(7, s["gen"]["K_info"], 64, s["B"]))
    seed = np.array([173, 173, 173], np.int32)
    rx1, rx2 = s["channel"](cw, seed), s["channel"](cw, seed)
    ident, punct = RateMatch(N), RateMatch(N, (), tuple(range(88, 96)))
    L1 = nb.RM_Demodulate_Recover_host(ident, 64, rx1, s["sigma"], CONSTELLATION=s["con"])
    Lp = nb.RM_Demodulate_Recover_host(punct, 64, np.ascontiguousarray(rx1[:, punct.tx_pos]), s["sigma"], CONSTELLATION=s["con"])
    L2 = nb.RM_Demodulate_Combine_host(ident, 64, rx2, s["sigma"], L1.copy(), None, CONSTELLATION=s["con"])
    mother, punctured, chase = frame_errors(orc, s, L1, cw), frame_errors(orc, s, Lp, cw), frame_errors(orc, s, L2, cw)
    print("frame errors of 100: mother %d, punctured %d, chase %d" % (mother, punctured, chase))
    assert punctured >= mother + 5, (mother, punctured)
    assert chase <= mother - 5, (mother, chase)


# ---- the simulations' refusals, before the device is touched ---------------------------------------------------------------------------
def test_simulation_refusals_come_before_the_device(nb, RateMatch, bds):
    """The code argument is a host matrix (no code object exists without a device): a refusal that came late would fail on it."""
    from cuda_ldpc_amd.bldpc import Fading
    from cuda_ldpc_amd.nb_simulation import NBSim, Simulation_GPU, Simulation_HARQ_GPU
    from cuda_ldpc_amd.simulation import HarqCounters
    H, info = bds["H"], bds["gen"]["info_pos"]
    par = np.setdiff1d(np.arange(H.N), info)
    seed = np.array([173, 173, 173], np.int32)
    good = RateMatch(H.N, info[:2], par[:2])
    zero = np.zeros(H.N, np.int32)
    bad_word = zero.copy()
    bad_word[info[1]] = 5
    cases = [(dict(rate_match=good, device_channel=False), "device_channel"),
             (dict(rate_match=RateMatch(H.N - 1), device_channel=True), "N="),
             (dict(rate_match=RateMatch(H.N, [int(par[0])], ()), device_channel=True), "parity position"),
             (dict(rate_match=good, device_channel=True, short_llr=float("inf")), "short_llr"),
             (dict(rate_match=good, device_channel=True, short_llr=0.0), "short_llr"),
             (dict(rate_match=good, device_channel=True, CONSTELLATION=bds["con"]), "runs over BPSK"),
             (dict(rate_match=good, device_channel=True, CONSTELLATION=bds["con"], fading=Fading(8, np.array([1, 2, 3], np.int32))), "runs over BPSK")]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            Simulation_GPU(H, seed, 0.7, NBSim(), zero, **kw)
    with pytest.raises(ValueError, match="not 0 at every shortened"):
        Simulation_GPU(H, seed, 0.7, NBSim(), bad_word, rate_match=good, device_channel=True, PN_Message=0)
    circ = lambda k0, E, sh=info[:2]: RateMatch.circular(H.N, sh, par[:2], k0, E)  # noqa: E731
    for rvs, kw, text in (([], {}, "at least one"), ([circ(0, 50), circ(0, 50, info[1:3])], {}, "shortens other positions"),
                          ([circ(0, 50)], dict(short_llr=-1.0), "short_llr"),
                          ([RateMatch(H.N, [int(par[0])], ())], {}, "parity position"), ([circ(0, 50)], dict(PN_Message=0), "needs CodeWord_sym"),
                          ([circ(0, 50)], dict(PN_Message=0, CodeWord_sym=bad_word), "not 0 at every shortened")):
        with pytest.raises(ValueError, match=text):
            Simulation_HARQ_GPU(H, seed, 0.7, HarqCounters(), rvs, **kw)
    assert seed.tolist() == [173, 173, 173]
