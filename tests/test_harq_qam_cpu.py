"""Binary HARQ over QAM without a GPU: the index rules of the modem (BLDPC_IL_NONE, BLDPC_IL_ROWCOL) and the host statements
bldpc_qam_map_il_host / bldpc_qam_demap_il_host against a numpy restatement of include/bldpc.h, as bit patterns; the three fused host
calls bldpc_rm_qam_*_host against the composition of the host statements they are said to be; every new refusal, in C and in Python,
with no device present; sweep_harq's sigma over QAM; the direction of the effect of combining a second transmission over 64-QAM; and
the host code as a stand-alone program (tests/cpp/harq_qam_host_test.hip) under the address + undefined sanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import harq_qam_cases as K
import qc_variant_cases as Q
from harq_qam_cases import IL_NONE, IL_ROWCOL, bits

SHORT_LLR = K.SHORT_LLR


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def test_the_cases_are_what_they_are_there_for(C):
    assert (C.IL_NONE, C.IL_ROWCOL) == (IL_NONE, IL_ROWCOL) == (0, 1)
    ns = [K.n_sym(N, m) for N, m in K.MODEM_SHAPES]
    assert any(n % 32 and n % 64 and n > 64 for n in ns), "a symbol count that is no multiple of either tile, over more than one tile"
    assert any(n < 4 for n in ns)
    e = K.bit_index(7, 3, IL_ROWCOL)
    assert len(set(np.argwhere(e >= 7)[:, 0])) == 2, "ROWCOL at (7, 3): pads in two different symbols"
    assert K.NCB == 2234 and K.NCB % 6, "a lap boundary and the wrap each fall inside a symbol at m = 6"
    assert [C.RateMatch.circular(K.N1, K.CH_SHORT, K.CH_PUNCT, k0, E).laps for k0, E in K.CASES] == K.LAPS
    for N, m in K.MODEM_SHAPES + [(E, 6) for _, E in K.CASES]:
        for il in K.RULES:
            e = K.bit_index(N, m, il)
            assert np.array_equal(np.sort(e[e < N]), np.arange(N)), "a bijection from {(s, b)} minus pads onto [0, N)"
            assert (e >= N).sum() == K.n_sym(N, m) * m - N
    assert sorted(K.CON_NAMES) == [2, 4, 8, 64, 128, 256] and all(K.constellation(C, q).shape == (q, 2) for q in K.CON_NAMES)


@pytest.mark.parametrize("N,m", K.MODEM_SHAPES)
def test_host_modem_against_numpy(C, N, m):
    """Every shape, both rules, every constellation of 2^m points the table has (m = 1, 3, 6, 7, 8 here; 2 in the fused test)."""
    rng = np.random.default_rng(N * 10 + m)
    F = 3
    cw = rng.integers(0, 2 ** 31 - 1, (N, F)).astype(np.int32)  # only bit 0 is read
    con = K.constellation(C, 1 << m)
    for il in K.RULES:
        sym = C.Modulate_QAM_host(cw, N, m, interleave=il)
        assert sym.dtype == np.int32 and np.array_equal(sym, K.np_map(cw, N, m, il)), ("map", il)
        assert not C.Modulate_QAM_host(None, N, m, F=F, interleave=il).any()
        rx = (con[sym] + rng.normal(0.0, 0.2, sym.shape + (2,))).astype(np.float32)
        rx[0, 0] = con[5 % len(con)]  # exactly on a point
        rx[F - 1, -1] = (con[0] + con[1]) / 2  # equidistant from two (up to the rounding of the midpoint)
        for scale in (1.0, 1.0 / (2 * 0.2 * 0.2)):
            got = C.Demodulate_QAM_host(rx, con, scale, N, interleave=il)
            assert np.array_equal(bits(got), bits(K.np_demap(rx, con, scale, N, il))), ("demap", il, scale)
        if il == IL_NONE:  # the entry points from before the interleaver, through ctypes: their own bits
            from cuda_ldpc_amd._lib import lib
            P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            old_sym, old = np.empty_like(sym), np.empty_like(got)
            assert lib.bldpc_qam_map_host(P(cw), N, F, m, P(old_sym)) == 0 and np.array_equal(old_sym, sym)
            assert lib.bldpc_qam_demap_host(P(rx), P(con), len(con), ctypes.c_float(scale), N, F, P(old)) == 0
            assert np.array_equal(bits(old), bits(got))
        elif m > 1 and N > m:
            assert not np.array_equal(sym, C.Modulate_QAM_host(cw, N, m)), "the two rules differ"


HOST_DONES = {"null": None, "all": lambda F: np.ones(F, np.int32), "none": lambda F: np.zeros(F, np.int32),
              "alternating": lambda F: (np.arange(F) % 2 * 7).astype(np.int32)}


@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_fused_host_calls_are_the_composition(C, case):
    k0, E = case
    rm = C.RateMatch.circular(K.N1, K.CH_SHORT, K.CH_PUNCT, k0, E)
    F = 4
    rng = np.random.default_rng(E)
    cw = rng.integers(0, 2, (K.N1, F)).astype(np.int32)
    for q, il in ((64, IL_ROWCOL), (64, IL_NONE), (4, IL_ROWCOL), (256, IL_NONE), (128, IL_ROWCOL), (2, IL_NONE)):
        m = q.bit_length() - 1
        con = K.constellation(C, q)
        sym = C.RM_Modulate_QAM_host(rm, cw, m, interleave=il)
        assert np.array_equal(sym, C.Modulate_QAM_host(C.RM_Select_host(rm, cw), E, m, interleave=il)), (q, il)
        assert np.array_equal(sym, K.np_map(cw[rm.tx_pos], E, m, il))
        assert not C.RM_Modulate_QAM_host(rm, None, m, F=F, interleave=il).any()
        rx = (con[sym] + rng.normal(0.0, 0.25, sym.shape + (2,))).astype(np.float32)
        rx[0, 0] = con[q - 1]  # exactly on a point
        rx[1, -1] = (con[0] + con[1]) / 2  # equidistant from two
        scale = 1.0 / (2 * 0.25 * 0.25)
        tmp = C.Demodulate_QAM_host(rx, con, scale, E, interleave=il)
        got = C.RM_Demodulate_QAM_Recover_host(rm, rx, con, scale, SHORT_LLR, interleave=il)
        assert np.array_equal(bits(got), bits(C.RM_Recover_host(rm, tmp, SHORT_LLR))), ("recover", q, il)
        for name, mk in HOST_DONES.items():
            done = None if mk is None else mk(F)
            acc = rng.standard_normal((K.N1, F)).astype(np.float32)
            acc[3, :] = -0.0
            acc[100, :] = 3.0e38
            want = C.RM_Combine_host(rm, tmp, acc.copy(), done, SHORT_LLR)
            before = acc.copy()
            assert C.RM_Demodulate_QAM_Combine_host(rm, rx, con, scale, acc, done, SHORT_LLR, interleave=il) is acc
            assert np.array_equal(bits(acc), bits(want)), ("combine", name, q, il)
            if name == "all":
                assert np.array_equal(bits(acc), bits(before))


def test_refusals_come_before_the_device(C):
    """No GPU here: a call that reached the device would fail with a HIP error (-3), not BLDPC_EINVAL (-1)."""
    from cuda_ldpc_amd._lib import lib
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_GPU, Simulation_HARQ_GPU
    x = np.zeros(64, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    p, one = P(x), ctypes.c_float(1.0)
    rm = C.RateMatch.circular(40, [0], [1], 5, 60)
    h, inf = rm._h, ctypes.c_float(float("inf"))
    err = lambda: lib.bldpc_last_error().decode()  # noqa: E731
    # the index rule, host and device entry points alike
    for il in (-1, 2):
        assert lib.bldpc_qam_map_il_host(p, 4, 1, 2, il, p) == -1 and "interleave=%d" % il in err()
        assert lib.bldpc_qam_demap_il_host(p, p, 4, one, 4, 1, il, p) == -1 and "interleave=%d" % il in err()
        assert lib.bldpc_qam_map_il(p, 4, 1, 2, il, p, None) == -1 and "bldpc_qam_map_il: interleave" in err()
        assert lib.bldpc_qam_demap_il(p, p, 4, one, 4, 1, il, p, None) == -1 and "bldpc_qam_demap_il: interleave" in err()
        assert lib.bldpc_rm_qam_map_host(h, p, 1, 2, il, p) == -1 and "interleave" in err()
        assert lib.bldpc_rm_qam_map(h, p, 1, 2, il, p, None) == -1 and "bldpc_rm_qam_map: interleave" in err()
        for fn in (lib.bldpc_rm_qam_recover_host, lib.bldpc_rm_qam_recover):
            assert fn(h, p, p, 4, one, il, 1, one, p, *([None] if fn is lib.bldpc_rm_qam_recover else [])) == -1 and "interleave" in err()
        for fn in (lib.bldpc_rm_qam_combine_host, lib.bldpc_rm_qam_combine):
            assert fn(h, p, p, 4, one, il, 1, one, None, p, *([None] if fn is lib.bldpc_rm_qam_combine else [])) == -1 and "interleave" in err()
    # what the old modem calls refuse, through the new ones
    assert lib.bldpc_qam_map_il(p, 0, 1, 2, 0, p, None) == -1 and lib.bldpc_qam_map_il(p, 4, 0, 2, 0, p, None) == -1
    assert lib.bldpc_qam_map_il(p, 4, 1, 9, 0, p, None) == -1 and "m=9" in err()
    assert lib.bldpc_qam_map_il(p, 4, 1, 2, 0, None, None) == -1 and "sym is NULL" in err()
    assert lib.bldpc_qam_demap_il(p, p, 3, one, 4, 1, 0, p, None) == -1 and "q=3" in err()
    assert lib.bldpc_qam_demap_il(p, p, 4, inf, 4, 1, 0, p, None) == -1 and "scale" in err()
    assert lib.bldpc_qam_demap_il(None, p, 4, one, 4, 1, 0, p, None) == -1 and lib.bldpc_qam_demap_il(p, p, 4, one, 4, 1, 0, None, None) == -1
    # the fused calls: profile, F, m, q, scale, short_llr, pointers
    for dev in (False, True):
        st = [None] if dev else []
        fmap = lib.bldpc_rm_qam_map if dev else lib.bldpc_rm_qam_map_host
        frec = lib.bldpc_rm_qam_recover if dev else lib.bldpc_rm_qam_recover_host
        fcom = lib.bldpc_rm_qam_combine if dev else lib.bldpc_rm_qam_combine_host
        assert fmap(None, p, 1, 2, 0, p, *st) == -1 and "null profile" in err()
        assert fmap(h, p, 0, 2, 0, p, *st) == -1 and fmap(h, p, 1, 0, 0, p, *st) == -1 and fmap(h, p, 1, 2, 0, None, *st) == -1
        for f, tail in ((frec, [p]), (fcom, [None, p])):
            assert f(None, p, p, 4, one, 0, 1, one, *tail, *st) == -1 and "null profile" in err()
            assert f(h, p, p, 4, one, 0, 0, one, *tail, *st) == -1
            assert f(h, p, p, 5, one, 0, 1, one, *tail, *st) == -1 and "q=5" in err()
            assert f(h, p, p, 4, inf, 0, 1, one, *tail, *st) == -1 and "scale" in err()
            for bad in (0.0, -1.0, float("inf"), float("nan")):
                assert f(h, p, p, 4, one, 0, 1, ctypes.c_float(bad), *tail, *st) == -1 and "short_llr" in err()
            assert f(h, None, p, 4, one, 0, 1, one, *tail, *st) == -1 and f(h, p, None, 4, one, 0, 1, one, *tail, *st) == -1
            assert f(h, p, p, 4, one, 0, 1, one, *tail[:-1], None, *st) == -1
    # Python
    con = K.constellation(C, 4)
    for bad in (2, -1, None, "rowcol"):
        with pytest.raises(ValueError, match="interleave"):
            C.Modulate_QAM_host(np.zeros((4, 1), np.int32), 4, 2, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.Demodulate_QAM_host(np.zeros((1, 2, 2), np.float32), con, 1.0, 4, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.Modulate_QAM(None, 4, 2, F=1, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.Demodulate_QAM(None, con, 1.0, 4, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.RM_Modulate_QAM(rm, None, 2, F=1, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.RM_Modulate_QAM_host(rm, None, 2, F=1, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.RM_Demodulate_QAM_Recover(rm, None, con, 1.0, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.RM_Demodulate_QAM_Recover_host(rm, np.zeros((1, 30, 2), np.float32), con, 1.0, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.RM_Demodulate_QAM_Combine(rm, None, con, 1.0, None, interleave=bad)
        with pytest.raises(ValueError, match="interleave"):
            C.RM_Demodulate_QAM_Combine_host(rm, np.zeros((1, 30, 2), np.float32), con, 1.0, np.zeros((40, 1), np.float32), interleave=bad)
    with pytest.raises(ValueError, match="m must be in 1..8"):
        C.RM_Modulate_QAM_host(rm, None, 9, F=1)
    with pytest.raises(ValueError, match=r"ceil\(E / m\) = 30"):
        C.RM_Demodulate_QAM_Recover_host(rm, np.zeros((1, 29, 2), np.float32), con, 1.0)
    with pytest.raises(ValueError, match="short_llr"):
        C.RM_Demodulate_QAM_Recover(rm, None, con, 1.0, short_llr=0.0)
    with pytest.raises(ValueError, match="rx holds 2 frames"):
        C.RM_Demodulate_QAM_Combine_host(rm, np.zeros((2, 30, 2), np.float32), con, 1.0, np.zeros((40, 1), np.float32))

    class Code:  # what the refusals read
        N, K = 2304, 1920
        info_positions = np.arange(1920, dtype=np.int32)

    seed = np.array([173, 173, 173], np.int32)
    con64 = K.constellation(C, 64)
    big = C.RateMatch.circular(2304, [0], [2303], 5, 2000)
    with pytest.raises(ValueError, match="interleave belongs to n_QAM != 2"):
        Simulation_GPU(Code, seed, 0.7, C.SimCounters(), device_channel=True, interleave=IL_ROWCOL)
    with pytest.raises(ValueError, match="interleave must be"):
        Simulation_GPU(Code, seed, 0.7, C.SimCounters(), device_channel=True, PN_Message=1, exit_mode=C.EXIT_FIXED, n_QAM=64, CONSTELLATION=con64,
                       interleave=3)
    harq = lambda **kw: Simulation_HARQ_GPU(Code, seed, 0.7, HarqCounters(), [big], **kw)  # noqa: E731
    with pytest.raises(ValueError, match="interleave belongs to n_QAM != 2"):
        harq(interleave=IL_ROWCOL)
    with pytest.raises(ValueError, match="interleave must be"):
        harq(n_QAM=64, CONSTELLATION=con64, PN_Message=1, interleave=2)
    with pytest.raises(ValueError, match="n_QAM=64 needs PN_Message=1: a QAM channel is not symmetric"):
        harq(n_QAM=64, CONSTELLATION=con64)
    with pytest.raises(ValueError, match=r"n_QAM=64 needs CONSTELLATION \(float32 \[n_QAM, 2\], Get_CONSTELLATION\)"):
        harq(n_QAM=64, PN_Message=1)
    with pytest.raises(ValueError, match="CONSTELLATION must be float32"):
        harq(n_QAM=64, PN_Message=1, CONSTELLATION=con)
    with pytest.raises(ValueError, match="CONSTELLATION belongs to n_QAM != 2"):
        harq(CONSTELLATION=con64)
    assert np.array_equal(seed, [173, 173, 173])


def test_sweep_harq_over_qam_takes_sigma_from_the_first_transmission(C, monkeypatch):
    from cuda_ldpc_amd import simulation
    from cuda_ldpc_amd.nbldpc import sigma_of as nb_sigma_of

    class Code:
        N, K = 2304, 1920

    seen = []
    monkeypatch.setattr(simulation, "Simulation_HARQ_GPU", lambda code, seed, sigma, SIM, rvs, **kw: seen.append((sigma, kw.get("n_QAM"), kw.get("interleave"))))
    rvs = [C.RateMatch.circular(2304, range(0, 24), (), 0, 2000), C.RateMatch.circular(2304, range(0, 24), (), 2000, 280)]
    rate = (1920 - 24) / 2000
    simulation.sweep_harq(Code, rvs, 9.0, 9.0, 1.0, snrtype=0, log=None, n_QAM=64, CONSTELLATION="con", interleave=IL_ROWCOL)
    simulation.sweep_harq(Code, rvs, 9.0, 9.0, 1.0, snrtype=1, log=None, n_QAM=256, CONSTELLATION="con")
    simulation.sweep_harq(Code, rvs, 3.0, 3.0, 1.0, snrtype=0, log=None)
    assert seen == [(nb_sigma_of(9.0, rate, 0, 64), 64, IL_ROWCOL), (nb_sigma_of(9.0, rate, 1, 256), 256, None), (C.sigma_of(3.0, 0, rate), None, None)]
    assert nb_sigma_of(9.0, rate, 0, 64) != nb_sigma_of(9.0, 1920 / 2304, 0, 64), "the rate of the first transmission enters"


# ---- what combining does to a decoder, over 64-QAM with the interleaver -----------------------------------------------------------
DIRECTION_SIGMA = 0.105


def test_the_direction_of_the_effect(C):
    """J4_L24_Z96, 128 random codewords (message stream 4242) over 64-QAM (the shipped Gray constellation, unit mean energy) with the
    row-column interleaver, numpy noise of DIRECTION_SIGMA per dimension, 20 iterations of layered_host at alpha 0.75.  First transmission:
    k0 = 0, E = 2000 of the 2304 positions, rate 0.96; second: k0 = 2000, E = 1200, which brings the rest and repeats 896.  The sigma was
    picked on the CPU so that the first transmission leaves most frames with H d != 0; only the direction is asserted."""
    from test_harq_cpu import qc_syndrome_bad, random_codewords
    _, H, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    H = np.asarray(H, np.int32).reshape(J, L)
    N, F = L * Z, 128
    cw = random_codewords(C, H, J, L, Z, F, 4242)
    con = K.constellation(C, 64)
    rvs = [C.RateMatch.circular(N, (), (), 0, 2000), C.RateMatch.circular(N, (), (), 2000, 1200)]
    rng = np.random.default_rng(7)
    scale = 1.0 / (2 * DIRECTION_SIGMA ** 2)
    rx = []
    for rm in rvs:
        pts = con[C.RM_Modulate_QAM_host(rm, cw, 6, interleave=IL_ROWCOL)]
        rx.append((pts + rng.normal(0.0, DIRECTION_SIGMA, pts.shape)).astype(np.float32))
    y1 = C.RM_Demodulate_QAM_Recover_host(rvs[0], rx[0], con, scale, interleave=IL_ROWCOL)
    y12 = C.RM_Demodulate_QAM_Combine_host(rvs[1], rx[1], con, scale, y1.copy(), interleave=IL_ROWCOL)
    assert not bits(y1)[2000:].any() and bits(y12)[2000:].all() and np.array_equal(bits(y12)[896:2000], bits(y1)[896:2000])
    u = [int(qc_syndrome_bad(H, J, L, Z, C.layered_host(H, J, L, Z, y, max_iter=20, alpha=0.75, want_app=False)["D"]).sum()) for y in (y1, y12)]
    print("frames of %d with an unsatisfied check: first transmission alone %d, second combined into it %d" % (F, *u))
    assert u[0] > F // 2, "the first transmission leaves most frames failing the syndrome"
    assert u[1] < u[0]


# ---- the host code under the host sanitizers, stand-alone -------------------------------------------------------------------------
def test_host_statements_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/harq_qam_host_test.hip with the three units that hold the host statements, built with -fsanitize=address,undefined on
    the host side, as test_harq_cpu.py builds harq_host_test.hip.  The program checks the statements against loops of its own and prints
    OK; a sanitizer report ends it with a non-zero status."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "cuda_ldpc_amd", "csrc")
    exe = str(tmp_path / "harq_qam_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "harq_qam_host_test.hip"),
                           os.path.join(csrc, "bldpc_modem.hip"), os.path.join(csrc, "bldpc_ratematch.hip"), os.path.join(csrc, "bldpc_channel.hip"),
                           "-o", exe], cwd=str(tmp_path))
    r = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert out.strip().split("\n")[-1].startswith("OK"), out
