"""Shortened and punctured binary codes without a GPU: the profile object and the host statements of include/bldpc.h
(bldpc_rm_select_host, bldpc_rm_recover_host, bldpc_rm_awgn_channel_host) against numpy indexing, as bit patterns; the noise stream
against AWGNChannel_CPU on the E transmitted bits; the direction of the effect on a decoder; the Python-side refusals."""
import numpy as np
import pytest

import qc_variant_cases as Q

N0 = 2304  # J4_L24_Z96


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scattered(N, n, seed, exclude=()):
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(N), np.asarray(exclude, np.int64))
    return rng.permutation(pool)[:n]


def profiles(N):
    """name -> (shorten, puncture): none, first and last positions of either kind, scattered ones, both kinds, given unsorted."""
    sc = scattered(N, 41, 1)
    sh = np.r_[0, scattered(N, 30, 2, exclude=[0, N - 1])]
    pu = np.r_[N - 1, scattered(N, 50, 3, exclude=np.r_[sh, N - 1])]
    return {
        "identity": ((), ()),
        "short-first-last": ([N - 1, 0], ()),
        "punct-first-last": ((), [N - 1, 0]),
        "short-scattered": (sc, ()),
        "punct-scattered": ((), sc),
        "both": (sh, pu),
        "ranges": (range(0, 480), range(1920, 2016)),
    }


def np_tx_pos(N, shorten, puncture):
    keep = np.ones(N, bool)
    keep[np.asarray(list(shorten), np.int64)] = False
    keep[np.asarray(list(puncture), np.int64)] = False
    return np.flatnonzero(keep).astype(np.int32)


def test_create_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    for kw, text in ((dict(shorten=[5, 2304]), "shortened position 2304 out of range"), (dict(puncture=[-1]), "punctured position -1 out of range"),
                     (dict(shorten=[7, 9, 7]), "shortened position 7 repeated"), (dict(puncture=[3, 3]), "punctured position 3 repeated"),
                     (dict(shorten=[11], puncture=[12, 11]), "position 11 is in both lists"),
                     (dict(shorten=range(0, 1000), puncture=range(1000, N0)), "E = N - n_short - n_punct = 0"),
                     (dict(shorten=range(0, N0)), "nothing is transmitted")):
        with pytest.raises(LdpcError, match=text):
            C.RateMatch(N0, **kw)
    with pytest.raises(LdpcError, match="N=0 outside"):
        C.RateMatch(0)
    # through the C ABI: a null list with a non-zero count, a negative count, a null result pointer
    import ctypes
    from cuda_ldpc_amd._lib import lib
    h = ctypes.c_void_p()
    pos = np.array([1, 2], np.int32)
    p = pos.ctypes.data_as(ctypes.c_void_p)
    assert lib.bldpc_rm_create(N0, None, 2, None, 0, ctypes.byref(h)) == -1 and b"null list with a non-zero count" in lib.bldpc_last_error()
    assert lib.bldpc_rm_create(N0, None, 0, None, 1, ctypes.byref(h)) == -1 and b"null list with a non-zero count" in lib.bldpc_last_error()
    assert lib.bldpc_rm_create(N0, p, -1, None, 0, ctypes.byref(h)) == -1 and b"negative count" in lib.bldpc_last_error()
    assert lib.bldpc_rm_create(N0, p, 2, None, 0, None) == -1 and not h.value
    assert lib.bldpc_rm_create(N0, p, 2, None, 0, ctypes.byref(h)) == 0 and h.value
    assert lib.bldpc_rm_destroy(h) == 0 and lib.bldpc_rm_destroy(None) == 0
    one = C.RateMatch(3, shorten=[0], puncture=[2])  # E = 1 is the least that is taken
    assert one.E == 1 and one.tx_pos.tolist() == [1]


def test_identity_profile(C):
    rm = C.RateMatch(N0)
    assert (rm.N, rm.E, rm.n_short, rm.n_punct) == (N0, N0, 0, 0) and np.array_equal(rm.tx_pos, np.arange(N0))
    assert rm.rate(1920) == 1920 / N0
    rng = np.random.default_rng(5)
    cw = rng.integers(0, 2, (N0, 5)).astype(np.int32)
    y = rng.standard_normal((N0, 5)).astype(np.float32)
    assert np.array_equal(C.RM_Select_host(rm, cw), cw) and np.array_equal(bits(C.RM_Recover_host(rm, y)), bits(y))
    s1, s2 = np.array([173, 173, 173], np.int32), np.array([173, 173, 173], np.int32)
    assert np.array_equal(bits(C.AWGNChannel_RM_CPU(rm, s1, 0.7, 5, CodeWord=cw)), bits(C.AWGNChannel_CPU(s2, 0.7, N0, 5, CodeWord=cw)))
    assert np.array_equal(s1, s2)


@pytest.mark.parametrize("name", list(profiles(N0)))
def test_tx_pos_and_rate(C, name):
    sh, pu = profiles(N0)[name]
    rm = C.RateMatch(N0, sh, pu)
    want = np_tx_pos(N0, sh, pu)
    assert rm.tx_pos.dtype == np.int32 and np.array_equal(rm.tx_pos, want) and np.all(np.diff(rm.tx_pos) > 0)
    assert (rm.N, rm.E, rm.n_short, rm.n_punct) == (N0, len(want), len(list(sh)), len(list(pu)))
    assert rm.rate(1920) == (1920 - rm.n_short) / rm.E
    assert np.array_equal(rm.shorten, np.sort(np.asarray(list(sh), np.int32))) and np.array_equal(rm.puncture, np.sort(np.asarray(list(pu), np.int32)))


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("name", list(profiles(N0)))
def test_select_and_recover_against_numpy(C, name, F):
    sh, pu = profiles(N0)[name]
    sh, pu = np.asarray(list(sh), np.int64), np.asarray(list(pu), np.int64)
    rm = C.RateMatch(N0, sh, pu)
    rng = np.random.default_rng(100 + F)
    cw = rng.integers(0, 2 ** 31 - 1, (N0, F)).astype(np.int32)  # a gather moves whole words
    assert np.array_equal(C.RM_Select_host(rm, cw), cw[rm.tx_pos])
    rx = rng.standard_normal((rm.E, F)).astype(np.float32)
    rx.reshape(-1)[:4] = np.array([-0.0, np.inf, 1e-42, -3e38], np.float32)[:rx.size]
    for short_llr in (1.0e4, 3.5):
        got = C.RM_Recover_host(rm, rx, short_llr)
        want = np.empty((N0, F), np.uint32)
        want[rm.tx_pos] = bits(rx)
        want[pu] = 0x00000000  # +0.0f, not -0.0f
        want[sh] = np.float32(short_llr).view(np.uint32)
        assert got.dtype == np.float32 and np.array_equal(bits(got), want)


def test_recover_refuses_bad_short_llr(C):
    from cuda_ldpc_amd._lib import LdpcError
    rm = C.RateMatch(N0, [0], [1])
    rx = np.ones((rm.E, 2), np.float32)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(LdpcError, match="short_llr"):
            C.RM_Recover_host(rm, rx, bad)
        with pytest.raises(LdpcError, match="short_llr"):
            C.AWGNChannel_RM_CPU(rm, np.array([173, 173, 173], np.int32), 0.7, 2, short_llr=bad)
    with pytest.raises(ValueError):
        C.RM_Recover_host(rm, rx[:-1])
    with pytest.raises(ValueError):
        C.RM_Select_host(rm, np.zeros((N0 + 1, 2), np.int32))


@pytest.mark.parametrize("F", [1, 5, 64])  # 64 frames of this N: bldpc_awgn_channel_host cuts the frames over two threads
@pytest.mark.parametrize("name", ["identity", "short-scattered", "punct-first-last", "both", "ranges"])
def test_channel_host_is_the_plain_channel_on_the_transmitted_bits(C, name, F):
    from cuda_ldpc_amd import sharding
    sh, pu = profiles(N0)[name]
    sh, pu = np.asarray(list(sh), np.int64), np.asarray(list(pu), np.int64)
    rm = C.RateMatch(N0, sh, pu)
    cw = np.random.default_rng(F).integers(0, 2, (N0, F)).astype(np.int32)
    cw[sh] = 0
    start = [173, 2001, 40000]
    for word in (cw, None):
        seed, seed_ref = np.array(start, np.int32), np.array(start, np.int32)
        got = C.AWGNChannel_RM_CPU(rm, seed, 0.73, F, CodeWord=word, short_llr=1.0e4)
        rx = C.AWGNChannel_CPU(seed_ref, 0.73, rm.E, F, CodeWord=None if word is None else word[rm.tx_pos])
        want = np.empty((N0, F), np.uint32)
        want[rm.tx_pos] = bits(rx)
        want[pu] = 0
        want[sh] = np.float32(1.0e4).view(np.uint32)
        assert np.array_equal(bits(got), want), "with a codeword" if word is not None else "all-zero word"
        assert np.array_equal(seed, seed_ref) and np.array_equal(seed, sharding.lcg_jump(start, 2 * rm.E * F))
        more = C.AWGNChannel_RM_CPU(rm, seed, 0.73, F, CodeWord=word)  # the stream goes on where the first call left it
        assert np.array_equal(bits(more)[rm.tx_pos], bits(C.AWGNChannel_CPU(seed_ref, 0.73, rm.E, F, CodeWord=None if word is None else word[rm.tx_pos])))


def test_the_direction_of_the_effect(C, orc):
    """J4_L24_Z96 at Es/N0 2.7 dB, 1024 frames of the seed (173, 173, 173), 50 fixed iterations of the flooding min-sum (alpha 1.0), the
    same noise on the shared positions: frames left unflagged by the mother code (the figure of test_normalised_cpu.test_the_gain_is_real),
    with positions 0..479 shortened at 1.0e4, with positions 1920..2015 punctured, and with both.  The CPU oracle gives 63, 2, 857 and
    216; normalised_host gives the same here: mother 63, shortened 2, punctured 857, both 216.  Known zeros help, erased parity bits hurt."""
    spec = ("shipped", "J4_L24_Z96")
    _, H, J, L, Z = Q.matrix(spec)
    N, F = L * Z, 1024
    assert N == N0
    y = Q.channel(orc, spec, 2.7, F).reshape(N, F)
    cases = {"mother": ((), ()), "shortened": (range(0, 480), ()), "punctured": ((), range(1920, 2016)), "both": (range(0, 480), range(1920, 2016))}
    u = {}
    for name, (sh, pu) in cases.items():
        rm = C.RateMatch(N, sh, pu)
        yin = C.RM_Recover_host(rm, y[rm.tx_pos], 1.0e4)
        assert np.array_equal(bits(yin)[rm.tx_pos], bits(y)[rm.tx_pos])
        r = C.normalised_host(H, J, L, Z, yin, max_iter=50, alpha=1.0)
        assert not np.isnan(r["app"]).any(), name + ": NaN among the a-posteriori values"
        assert not r["D"][rm.shorten].any(), name + ": a shortened position decided 1"
        u[name] = int((r["D"][N] == 0).sum())
    print("unflagged frames of %d: %s" % (F, u))
    assert u["shortened"] < u["mother"] < u["punctured"]


def test_sweep_position_spec():
    import sweep
    assert sweep.parse_positions("0:3,10:12") == [0, 1, 2, 10, 11] and sweep.parse_positions(" 5:6 , 2:4", 6) == [2, 3, 5]
    for bad in ("3", "4:4", "a:b", "0:3,", "2:7"):
        with pytest.raises(ValueError):
            sweep.parse_positions(bad, 6)


def test_simulation_refusals_come_before_the_device(C):
    """Simulation_GPU(rate_match=...) refuses on the host what it cannot run: these raise on a machine without a GPU."""
    from cuda_ldpc_amd.simulation import Simulation_GPU

    class Code:  # what the refusals read
        N, K = N0, 1920

    rm = C.RateMatch(N0, [0], [N0 - 1])
    seed = np.array([173, 173, 173], np.int32)
    with pytest.raises(ValueError, match="device_channel"):
        Simulation_GPU(Code, seed, 0.7, C.SimCounters(), rate_match=rm)
    with pytest.raises(ValueError, match="N=100 positions"):
        Simulation_GPU(Code, seed, 0.7, C.SimCounters(), rate_match=C.RateMatch(100), device_channel=True)
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="short_llr"):
            Simulation_GPU(Code, seed, 0.7, C.SimCounters(), rate_match=rm, short_llr=bad, device_channel=True)


def test_sweep_takes_sigma_from_the_derived_rate(C, monkeypatch):
    """Eb/N0 (snrtype 0): sigma of the rate (K - n_short) / E, over BPSK and over QAM; Es/N0 does not look at the rate."""
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd import simulation

    class Code:
        N, K = N0, 1920

    seen = []
    monkeypatch.setattr(simulation, "Simulation_GPU", lambda code, seed, sigma, SIM, **kw: seen.append(sigma))
    rm = C.RateMatch(N0, range(0, 24), range(2188, 2260))
    rate = (1920 - 24) / (N0 - 24 - 72)
    assert rm.rate(Code.K) == rate and rate != Code.K / Code.N
    simulation.sweep(Code, 3.0, 3.0, 1.0, snrtype=0, log=None, rate_match=rm)
    simulation.sweep(Code, 3.0, 3.0, 1.0, snrtype=0, log=None)
    simulation.sweep(Code, 3.0, 3.0, 1.0, snrtype=1, log=None, rate_match=rm)
    simulation.sweep(Code, 3.0, 3.0, 1.0, snrtype=0, log=None, n_QAM=64, CONSTELLATION=None, rate_match=rm)
    assert seen == [C.sigma_of(3.0, 0, rate), C.sigma_of(3.0, 0, Code.K / Code.N), C.sigma_of(3.0, 1), nb.sigma_of(3.0, rate, 0, 64)]
    assert seen[0] != seen[1]
