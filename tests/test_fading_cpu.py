"""Block fading without a GPU: the host statements of include/bldpc.h ("block fading") and include/nbldpc.h -- the gains, the two
channels that apply them, the two demappers with receiver CSI -- against their AWGN counterparts at all-ones gains (as 32-bit words),
against float32 numpy restatements, and against the draw indexing the headers state; every refusal, in C and in Python, with no device
present; the gains of a global frame at any world size; what fading does to a decoder and what a second transmission does about it;
and the host code as a stand-alone program (tests/cpp/fading_host_test.hip) under the address + undefined sanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fading_cases as K
import qc_variant_cases as Q
from fading_cases import IL_NONE, IL_ROWCOL, bits


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def seed_of(t=K.FADE_SEED):
    return np.array(t, np.int32)


def jumped(C, seed, draws):
    s = np.array(seed, np.int32)
    assert C._lib.lib.nbldpc_seed_jump(s.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulonglong(draws)) == 0
    return s


def random_module_draws(seed, n):
    """RandomModule in numpy float32, as common_lcg.hpp writes the host form."""
    s, out = [int(x) for x in seed], []
    for _ in range(n):
        s = [(s[i] * a) % m for i, (a, m) in enumerate(((249, 61967), (251, 63443), (252, 63599)))]
        t = np.float32(s[0]) / np.float32(61967.0) + np.float32(s[1]) / np.float32(63443.0) + np.float32(s[2]) / np.float32(63599.0)
        out.append(t - np.float32(int(t)))
    return np.array(out, np.float32)


# ---- gains ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Lc,F", K.GAIN_SHAPES)
def test_gains_block_structure_seed_and_range(C, S, Lc, F):
    from cuda_ldpc_amd import sharding
    seed = seed_of()
    g = C.Fading_Gains_host(seed, Lc, S, F)
    nb = -(-S // Lc)
    assert sharding.fading_draws_per_frame(S, Lc) == nb
    assert g.shape == (F, S) and g.dtype == np.float32
    s = np.arange(S)
    assert np.array_equal(bits(g), bits(g[:, (s // Lc) * Lc])), "constant over every block"
    assert np.array_equal(seed, jumped(C, K.FADE_SEED, nb * F)) and np.array_equal(seed, sharding.lcg_jump(K.FADE_SEED, nb * F))
    assert np.isfinite(g).all() and g.min() >= 0.0 and g.max() <= 4.1, "1 - u >= 2^-24, so a <= sqrt(24 ln 2) = 4.08"
    # the draws themselves: block j of frame f is draw f * nb + j of the stream
    u = random_module_draws(K.FADE_SEED, min(nb * F, 200))
    want = np.sqrt(-np.log(np.float32(1.0) - u))
    got = g[:, ::Lc].reshape(-1)[:want.size] if Lc <= S else g[:, 0][:want.size]
    assert np.abs(got - want).max() < 1e-6
    # two half batches, the second from the jumped seed, are one batch
    if F > 1:
        h = F // 2
        sa = seed_of()
        a = C.Fading_Gains_host(sa, Lc, S, h)
        assert np.array_equal(sa, jumped(C, K.FADE_SEED, nb * h))
        b = C.Fading_Gains_host(sa, Lc, S, F - h)
        assert np.array_equal(bits(np.concatenate([a, b])), bits(g)) and np.array_equal(sa, seed)


def test_gains_lc_above_s_is_one_block(C):
    a = C.Fading_Gains_host(seed_of(), 77, 77, 70)
    for Lc in (78, 100, 1 << 30):
        s = seed_of()
        assert np.array_equal(bits(C.Fading_Gains_host(s, Lc, 77, 70)), bits(a))
        assert np.array_equal(s, jumped(C, K.FADE_SEED, 70))


def test_gains_have_unit_mean_power(C):
    """a^2 = -ln(1 - u) is exponential with mean 1 and variance 1: over n draws the mean of a^2 is within five standard errors of 1.  The
    seed is the sweeps' default."""
    F, S = 400, 256
    n = F * S
    assert n >= 10 ** 5
    g = C.Fading_Gains_host(seed_of(), 1, S, F).astype(np.float64)
    m = float((g * g).mean())
    print("mean(a^2) over %d draws: %.5f (bound %.5f)" % (n, m, 5 / np.sqrt(n)))
    assert abs(m - 1.0) <= 5 / np.sqrt(n)


# ---- identity with all-ones gains ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,F", K.BPSK_SHAPES)
def test_bpsk_channel_with_unit_gains_is_the_awgn_channel(C, N, F):
    rng = np.random.default_rng(N + F)
    ones = np.ones((F, N), np.float32)
    for cw in (None, rng.integers(0, 2, (N, F)).astype(np.int32)):
        sa, sb = np.array([173, 173, 173], np.int32), np.array([173, 173, 173], np.int32)
        a = C.AWGNChannel_CPU(sa, 0.7, N, F, CodeWord=cw)
        b = C.AWGNChannel_Fading_CPU(sb, 0.7, ones, N, F, CodeWord=cw)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa, sb)


def test_bpsk_channel_applies_the_gain_twice(C):
    """r = a x + n and the output is a r: with sigma 0 the value is exactly a * float(a * (1 - 2c))."""
    N, F = 77, 5
    g = C.Fading_Gains_host(seed_of(), 5, N, F)
    cw = np.random.default_rng(3).integers(0, 2, (N, F)).astype(np.int32)
    y = C.AWGNChannel_Fading_CPU(np.array([1, 2, 3], np.int32), 0.0, g, N, F, CodeWord=cw)
    x = (1 - 2 * cw).astype(np.float32)
    assert np.array_equal(bits(y), bits(g.T * (g.T * x)))


@pytest.mark.parametrize("Ns,q,F", K.QAM_SHAPES)
def test_qam_channel_with_unit_gains_is_the_awgn_channel_per_frame(C, Ns, q, F):
    from cuda_ldpc_amd import nbldpc as nb
    rng = np.random.default_rng(Ns + q)
    con = K.con_of(C, q.bit_length() - 1)
    sym = rng.integers(0, q, (F, Ns)).astype(np.int32)
    sa, sb = np.array([173, 173, 173], np.int32), np.array([173, 173, 173], np.int32)
    got = C.AWGNChannel_QAM_Fading_CPU(sa, 0.3, sym, con, np.ones((F, Ns), np.float32))

    class Code:
        N = Ns
    want = np.stack([nb.AWGNChannel_CPU(sb, 0.3, Code, sym[f], CONSTELLATION=con) for f in range(F)])
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(sa, sb)
    assert np.array_equal(sa, jumped(C, (173, 173, 173), 4 * Ns * F))
    # symbols are masked with q - 1, as the per-frame device call masks them
    sc = np.array([173, 173, 173], np.int32)
    assert np.array_equal(bits(C.AWGNChannel_QAM_Fading_CPU(sc, 0.3, sym + q, con, np.ones((F, Ns), np.float32))), bits(got))
    # the gain scales the point, not the noise
    g = C.Fading_Gains_host(seed_of(), 5, Ns, F)
    sd = np.array([173, 173, 173], np.int32)
    faded = C.AWGNChannel_QAM_Fading_CPU(sd, 0.0, sym, con, g)
    assert np.array_equal(bits(faded), bits((g[:, :, None].astype(np.float64) * con[sym].astype(np.float64)).astype(np.float32)))


# ---- demappers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m,F", K.DEMAP_SHAPES)
def test_demapper_against_numpy_and_the_plain_demapper(C, N, m, F):
    rx, gain, con = K.demap_inputs(C, N, m, F, N * 10 + m)
    ones = np.ones_like(gain)
    Ns = K.n_sym(N, m)
    for il in K.RULES:
        for scale in (1.0, 1.0 / (2 * 0.2 * 0.2)):
            got = C.Demodulate_QAM_Fading_host(rx, gain, con, scale, N, interleave=il)
            assert np.array_equal(bits(got), bits(K.np_demap_fading(rx, gain, con, scale, N, il))), (il, scale)
            assert np.array_equal(bits(C.Demodulate_QAM_Fading_host(rx, ones, con, scale, N, interleave=il)),
                                  bits(C.Demodulate_QAM_host(rx, con, scale, N, interleave=il))), "a = 1 is the plain demapper"
            e = K.bit_index(N, m, il)
            f, s = np.nonzero(gain == 0.0)
            assert f.size, "the inputs hold erased symbols"
            for b in range(m):
                keep = e[s, b] < N
                assert not bits(got)[e[s[keep], b], f[keep]].any(), "a zero gain gives +0.0 on all its bits, as bit patterns"
    assert gain.shape == (F, Ns)


@pytest.mark.parametrize("q,N,B", K.NB_SHAPES)
def test_nb_demodulator_against_numpy(C, q, N, B):
    from cuda_ldpc_amd import nbldpc as nb
    rng = np.random.default_rng(q + N + B)
    con = K.con_of(C, q.bit_length() - 1)
    gain = C.Fading_Gains_host(seed_of(), 5, N, B)
    gain.reshape(-1)[::7] = 1.0
    gain.reshape(-1)[3::11] = 0.0
    sym = rng.integers(0, q, (B, N))
    rx = (gain[:, :, None] * con[sym] + rng.normal(0.0, 0.2, (B, N, 2))).astype(np.float32)
    got = nb.Demodulate_QAM_Fading_host(N, q, rx, gain, con, 0.2)
    assert got.shape == (B, N, q - 1)
    assert np.array_equal(bits(got), bits(K.np_nb_demod(rx, con, 0.2, gain)))
    assert np.array_equal(bits(nb.Demodulate_QAM_Fading_host(N, q, rx, np.ones_like(gain), con, 0.2)), bits(K.np_nb_demod(rx, con, 0.2))), \
        "a = 1 is k_nb_demod_qam's expression"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_c_refusals(C):
    lib = C._lib.lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    f32 = ctypes.c_float
    g, out, rx, con = np.ones(64, np.float32), np.zeros(4096, np.float32), np.zeros(64, np.float32), np.zeros((4, 2), np.float32)
    sym = np.zeros(16, np.int32)
    good = lambda: np.array([1, 2, 3], np.int32)  # noqa: E731
    bad_seeds = [np.array([61967, 2, 3], np.int32), np.array([1, -1, 3], np.int32), np.array([1, 2, 63599], np.int32)]
    EINVAL = -1
    for fn, dev in ((lib.bldpc_fading_gains_host, ()), (lib.bldpc_fading_gains_device, (None,))):
        assert fn(p(good()), 0, 4, 4, p(g), *dev) == EINVAL and b"Lc" in lib.bldpc_last_error()
        assert fn(p(good()), -3, 4, 4, p(g), *dev) == EINVAL
        assert fn(p(good()), 1, 0, 4, p(g), *dev) == EINVAL
        assert fn(p(good()), 1, 4, 0, p(g), *dev) == EINVAL
        assert fn(None, 1, 4, 4, p(g), *dev) == EINVAL
        assert fn(p(good()), 1, 4, 4, None, *dev) == EINVAL
        for s in bad_seeds:
            keep = s.copy()
            assert fn(p(s), 1, 4, 4, p(g), *dev) == EINVAL and b"seed" in lib.bldpc_last_error() and np.array_equal(s, keep)
    for fn, dev in ((lib.bldpc_awgn_fading_channel_host, ()), (lib.bldpc_awgn_fading_channel_device, (None,))):
        assert fn(p(good()), f32(1.0), None, p(out), None, 4, 4, *dev) == EINVAL and b"gain" in lib.bldpc_last_error()
        assert fn(p(good()), f32(1.0), p(g), None, None, 4, 4, *dev) == EINVAL
        assert fn(None, f32(1.0), p(g), p(out), None, 4, 4, *dev) == EINVAL
        assert fn(p(good()), f32(1.0), p(g), p(out), None, 0, 4, *dev) == EINVAL
        assert fn(p(good()), f32(1.0), p(g), p(out), None, 4, -1, *dev) == EINVAL
        assert fn(p(bad_seeds[0]), f32(1.0), p(g), p(out), None, 4, 4, *dev) == EINVAL
    for fn, dev in ((lib.nbldpc_fading_channel_host_qam_frames, ()), (lib.nbldpc_fading_channel_device_qam_frames, (None,))):
        args = lambda **k: [k.get("seed", p(good())), f32(1.0), k.get("cw", p(sym)), k.get("N", 4), k.get("con", p(con)), k.get("q", 4),  # noqa: E731
                            k.get("gain", p(g)), k.get("B", 4), k.get("rx", p(out))] + list(dev)
        for k in (dict(seed=None), dict(cw=None), dict(con=None), dict(gain=None), dict(rx=None), dict(N=0), dict(B=0), dict(q=3), dict(q=1),
                  dict(seed=p(bad_seeds[2]))):
            assert fn(*args(**k)) == EINVAL, k
            assert lib.nbldpc_last_error()
    for fn, dev in ((lib.bldpc_qam_demap_fading_host, ()), (lib.bldpc_qam_demap_fading, (None,))):
        args = lambda **k: [k.get("rx", p(rx)), k.get("gain", p(g)), k.get("con", p(con)), k.get("q", 4), f32(k.get("scale", 1.0)), k.get("N", 8),  # noqa: E731
                            k.get("F", 4), k.get("il", 0), k.get("out", p(out))] + list(dev)
        for k in (dict(rx=None), dict(gain=None), dict(con=None), dict(out=None), dict(q=3), dict(q=512), dict(q=1), dict(scale=float("inf")),
                  dict(scale=float("nan")), dict(N=0), dict(F=0), dict(il=2), dict(il=-1)):
            assert fn(*args(**k)) == EINVAL, k
    for fn, dev in ((lib.nbldpc_demodulate_qam_fading_host, ()), (lib.nbldpc_demodulate_qam_fading_nq, (None,))):
        args = lambda **k: [k.get("N", 4), k.get("q", 4), k.get("rx", p(rx)), k.get("gain", p(g)), k.get("con", p(con)), f32(k.get("sigma", 0.5)),  # noqa: E731
                            k.get("B", 2), k.get("Lch", p(out))] + list(dev)
        for k in (dict(N=0), dict(q=1), dict(rx=None), dict(gain=None), dict(con=None), dict(sigma=0.0), dict(sigma=float("nan")), dict(B=0),
                  dict(Lch=None)):
            assert fn(*args(**k)) == EINVAL, k
    assert lib.nbldpc_demodulate_qam_fading(None, p(rx), p(g), p(con), f32(0.5), 2, p(out), None) == EINVAL


def test_python_refusals(C):
    """Every refusal of section "fading" of the three drivers is raised before anything touches the device: none of the objects below is
    a real code, and there is no GPU here."""
    from cuda_ldpc_amd import nb_simulation, simulation

    class Code:
        N, K = 2304, 1920

    con = K.constellation(C, 64)
    seed = np.array([173, 173, 173], np.int32)
    ok = C.Fading(16)
    assert ok.seed.dtype == np.int32 and ok.seed.tolist() == list(K.FADE_SEED) and ok.Lc == 16
    ok.check()
    C.Fading(C.QUASI_STATIC).check()
    bin_kw = dict(device_channel=True, exit_mode=C.EXIT_PER_FRAME, schedule="layered")
    for kw, word in ((dict(bin_kw, device_channel=False, fading=ok), "device_channel"),
                     (dict(bin_kw, exit_mode=C.EXIT_BATCH_GLOBAL, schedule="flooding", fading=ok), "EXIT_BATCH_GLOBAL"),
                     (dict(bin_kw, fading=C.Fading(0)), "Lc"),
                     (dict(bin_kw, fading=C.Fading(-2)), "Lc"),
                     (dict(bin_kw, fading=C.Fading(1.5)), "Lc"),
                     (dict(bin_kw, fading=C.Fading(4, (61967, 1, 1))), "seed"),
                     (dict(bin_kw, fading=C.Fading(4, (1, -1, 1))), "seed"),
                     (dict(bin_kw, fading=C.Fading(4, (1, 2))), "seed"),
                     (dict(bin_kw, fading=16), "Fading")):
        with pytest.raises(ValueError, match=word):
            simulation.Simulation_GPU(Code, seed, 0.5, C.SimCounters(), **kw)
    rvs = [C.RateMatch.circular(2304, (), (), 0, 2000)]
    for kw, word in ((dict(fading=C.Fading(0)), "Lc"), (dict(fading=C.Fading(4, (1, 2, 63599))), "seed"), (dict(fading="16"), "Fading")):
        with pytest.raises(ValueError, match=word):
            simulation.Simulation_HARQ_GPU(Code, seed, 0.5, simulation.HarqCounters(), rvs, exit_mode=C.EXIT_PER_FRAME, schedule="layered", **kw)
    with pytest.raises(ValueError, match="EXIT_BATCH_GLOBAL"):
        simulation.Simulation_HARQ_GPU(Code, seed, 0.5, simulation.HarqCounters(), rvs, exit_mode=C.EXIT_BATCH_GLOBAL, fading=ok)

    class NbCode:
        N, q, m = 96, 64, 6

    dev = "cpu"  # never reached
    for kw, word in ((dict(device_channel=False, CONSTELLATION=con, fading=ok), "device_channel"),
                     (dict(device_channel=True, CONSTELLATION=None, fading=ok), "BPSK"),
                     (dict(device_channel=True, CONSTELLATION=con, fading=C.Fading(0)), "Lc"),
                     (dict(device_channel=True, CONSTELLATION=con, fading=C.Fading(2, (1, 2, 70000))), "seed"),
                     (dict(device_channel=True, CONSTELLATION=con, fading=3), "Fading")):
        with pytest.raises(ValueError, match=word):
            nb_simulation.Simulation_GPU(NbCode, seed, 0.5, nb_simulation.NBSim(), np.zeros(96, np.int32), device=dev, **kw)
    # the primitives' own argument checks, host side
    with pytest.raises(ValueError):
        C.Fading_Gains_host(seed_of(), 0, 4, 4)
    with pytest.raises(ValueError):
        C.Fading_Gains_host(np.array([1, 2, 3], np.int64), 1, 4, 4)
    with pytest.raises(ValueError):
        C.AWGNChannel_Fading_CPU(seed_of(), 0.5, np.ones((4, 5), np.float32), 4, 4)
    with pytest.raises(ValueError):
        C.Demodulate_QAM_Fading_host(np.zeros((3, 2, 2), np.float32), np.ones((3, 3), np.float32), con, 1.0, 12)
    with pytest.raises(ValueError):
        C.AWGNChannel_QAM_Fading_CPU(seed_of(), 0.5, np.zeros((3, 2), np.int32), con, np.ones((2, 3), np.float32))
    with pytest.raises(C._lib.LdpcError, match="seed"):
        C.Fading_Gains_host(np.array([61967, 1, 1], np.int32), 1, 4, 4)


def test_sweeps_restart_the_fading_stream_at_every_point(C, monkeypatch):
    from cuda_ldpc_amd import simulation

    class Code:
        N, K = 2304, 1920

    seen = []

    def fake(code, seed, sigma, SIM, *a, **kw):
        seen.append(kw["fading"].seed.tolist())
        kw["fading"].seed[:] = (9, 9, 9)  # a driver advances it in place

    monkeypatch.setattr(simulation, "Simulation_GPU", fake)
    monkeypatch.setattr(simulation, "Simulation_HARQ_GPU", fake)
    simulation.sweep(Code, 1.0, 3.0, 1.0, log=None, fading=C.Fading(4, (5, 6, 7)))
    simulation.sweep_harq(Code, [C.RateMatch.circular(2304, (), (), 0, 2000)], 1.0, 2.0, 1.0, log=None, fading=C.Fading(4))
    assert seen == [[5, 6, 7]] * 3 + [list(K.FADE_SEED)] * 2


# ---- world-size invariance ----------------------------------------------------------------------------------------------------------
def test_the_gains_of_a_global_frame_do_not_depend_on_the_world_size(C):
    """As tests/test_sharding_cpu.py does for the noise: every rank jumps the fading seed by first_frame * fading_draws_per_frame and
    draws its own frames; global frame g gets the same gains at world sizes 1, 2, 3, 5, over two batches."""
    from cuda_ldpc_amd import sharding
    F, S = 23, 77
    for Lc in (1, 5, 100):
        per = sharding.fading_draws_per_frame(S, Lc)
        base = None
        for world in (1, 2, 3, 5):
            seed = seed_of()
            batches = []
            for _ in range(2):
                parts = []
                for rank in range(world):
                    first, count = sharding.shard_frames(F, world, rank)
                    mine = sharding.lcg_jump(seed, first * per)
                    if count:
                        parts.append(C.Fading_Gains_host(mine, Lc, S, count))
                seed[:] = sharding.lcg_jump(seed, F * per)
                batches.append(np.concatenate(parts))
            got = np.concatenate(batches)
            if base is None:
                base = got
                assert np.array_equal(bits(base), bits(C.Fading_Gains_host(seed_of(), Lc, S, 2 * F))), "two batches are one stream"
            assert np.array_equal(bits(got), bits(base)), (Lc, world)


# ---- what fading does ---------------------------------------------------------------------------------------------------------------
DIRECTION_ESN0_DB = 18.0  # picked on the CPU: the AWGN channel leaves no frame of the 128 failing, 19 dB and 20 dB neither, 17 dB 44


def test_what_fading_does(C):
    """J4_L24_Z96 over 64-QAM (the shipped Gray constellation, unit mean energy, consecutive bits per point), 128 random codewords
    (message stream 4242), host statements only, 25 iterations of layered_host at alpha 0.75, sigma of Es/N0 = 18 dB per dimension
    (0.0890), noise seed 173/173/173, fading seed 4711/4712/4713.  Frames of 128 with an unsatisfied check:
        AWGN (all-ones gains)                                   0
        quasi-static fading, one transmission                  73
        a second transmission with fresh gains, Chase-combined 28
    Only the directions are asserted.  At such a point a large share of the frames has a^2 below what the code needs."""
    from test_harq_cpu import qc_syndrome_bad, random_codewords
    _, H, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    H = np.asarray(H, np.int32).reshape(J, L)
    N, F, m = L * Z, 128, 6
    Ns = N // m
    cw = random_codewords(C, H, J, L, Z, F, 4242)
    con = K.constellation(C, 64)
    sigma = float(np.sqrt(0.5 / 10 ** (DIRECTION_ESN0_DB / 10)))
    sym = C.Modulate_QAM_host(cw, N, m)
    rm = C.RateMatch(N)

    def receive(noise_seed, gain):
        rx = C.AWGNChannel_QAM_Fading_CPU(noise_seed, sigma, sym, con, gain)
        return C.Demodulate_QAM_Fading_host(rx, gain, con, 1.0 / (2 * sigma * sigma), N)

    def failures(y):
        return int(qc_syndrome_bad(H, J, L, Z, C.layered_host(H, J, L, Z, y, max_iter=25, alpha=0.75, want_app=False)["D"]).sum())

    awgn = failures(receive(np.array([173, 173, 173], np.int32), np.ones((F, Ns), np.float32)))
    noise, fade = np.array([173, 173, 173], np.int32), seed_of()
    y1 = receive(noise, C.Fading_Gains_host(fade, C.QUASI_STATIC, Ns, F))
    first = failures(y1)
    y2 = receive(noise, C.Fading_Gains_host(fade, C.QUASI_STATIC, Ns, F))  # fresh gains, fresh noise: both seeds have moved on
    both = failures(C.RM_Combine_host(rm, y2, C.RM_Recover_host(rm, y1)))
    print("frames of %d with an unsatisfied check: AWGN %d, quasi-static fading %d, second transmission combined %d" % (F, awgn, first, both))
    assert awgn <= F * 5 // 100, "the operating point: AWGN leaves at most 5 % of the frames failing"
    assert first > awgn, "strictly more failures with fading"
    assert both < first, "strictly fewer after a second transmission with fresh gains"


# ---- the host code under the host sanitizers, stand-alone -------------------------------------------------------------------------
def test_host_statements_stand_alone_under_sanitizers(tmp_path):
    """tests/cpp/fading_host_test.hip with the unit that holds the five host statements (and bldpc_channel.hip, whose AWGN channel the BPSK one is compared with), built with -fsanitize=address,undefined on the
    host side, as test_harq_cpu.py builds harq_host_test.hip.  The program calls the statements at the odd shapes of fading_cases.py with
    buffers of exactly the stated sizes, checks them against loops of its own and prints OK; a sanitizer report ends it with a non-zero
    status.  Nothing is preloaded and nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "cuda_ldpc_amd", "csrc")
    exe = str(tmp_path / "fading_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(here, "cpp", "fading_host_test.hip"),
                           os.path.join(csrc, "bldpc_fading.hip"), os.path.join(csrc, "bldpc_channel.hip"), "-o", exe], cwd=str(tmp_path))
    r = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert out.strip().split("\n")[-1].startswith("OK"), out
