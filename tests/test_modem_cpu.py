"""The QAM bit mapper and max-log demapper without a GPU: bldpc_qam_map_host / bldpc_qam_demap_host (plain C++, the statement of
the semantics inside the product) against a numpy float32 restatement of include/bldpc.h written here, bit for bit; ties, pad bits,
the all-zero word, a noise-free round trip; every argument check of the four entry points (the device ones refuse before they touch
a device); the draw count the sharded sweep jumps by; the refusals of Simulation_GPU and of sweep.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT

CON = os.path.join(DATA, "nb", "Constellation")
BLDPC_EINVAL = -1


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def np_demap(rx, con, scale, N):
    """include/bldpc.h restated in numpy float32: broadcast dx*dx + dy*dy, np.minimum.reduce over the index masks, subtract, multiply."""
    rx, con = np.asarray(rx, np.float32), np.asarray(con, np.float32)
    q = con.shape[0]
    m = q.bit_length() - 1
    F, Ns, _ = rx.shape
    dx = rx[:, :, None, 0] - con[None, None, :, 0]
    dy = rx[:, :, None, 1] - con[None, None, :, 1]
    d = dx * dx + dy * dy
    assert d.dtype == np.float32
    p = np.arange(q)
    out = np.full((N, F), np.nan, np.float32)
    for b in range(m):
        m0 = np.minimum.reduce(d[:, :, ((p >> b) & 1) == 0], axis=2)
        m1 = np.minimum.reduce(d[:, :, ((p >> b) & 1) == 1], axis=2)
        v = (m1 - m0) * np.float32(scale)  # [F, Ns]
        n = np.arange(Ns) * m + b
        out[n[n < N]] = v[:, n < N].T
    assert not np.isnan(out).any()
    return out


def np_map(cw, N, F, m):
    Ns = (N + m - 1) // m
    bits = np.zeros((Ns * m, F), np.int64)
    if cw is not None:
        bits[:N] = np.asarray(cw) & 1
    return (bits.reshape(Ns, m, F) << np.arange(m)[None, :, None]).sum(1).T.astype(np.int32)


QPSK = np.array([[1, 1], [-1, 1], [1, -1], [-1, -1]], np.float32)  # bit 0: sign of x, bit 1: sign of y


def constellation(C, name):
    if name == "gray64":
        return C.Get_CONSTELLATION(os.path.join(CON, "GRAY_64QAM.txt"), 64)
    if name == "gray256":
        return C.Get_CONSTELLATION(os.path.join(CON, "GRAY_256QAM.txt"), 256)
    if name == "bpsk":
        return C.Get_CONSTELLATION(os.path.join(CON, "BPSK.txt"), 2)
    if name == "qpsk":
        return QPSK.copy()
    q = int(name[4:])  # "rand8", "rand256": seeded, no product structure
    return np.random.default_rng(1000 + q).normal(0.0, 0.75, (q, 2)).astype(np.float32)


def make_rx(con, Ns, F, seed):
    """Seeded Gaussian points, the leading ones replaced by exact constellation points (ties m0 = 0)."""
    rx = np.random.default_rng(seed).normal(0.0, 0.9, (F, Ns, 2)).astype(np.float32)
    flat = rx.reshape(-1, 2)
    k = min(len(con), len(flat))
    flat[:k] = con[:k]
    return rx


# (N, m, F) with the constellations of 2^m points that go with them; the first five shapes are the issue's
DEMAP_CASES = [(1, 8, 1, "gray256"), (1, 8, 1, "rand256"), (7, 3, 5, "rand8"), (2304, 6, 3, "gray64"), (4096, 6, 2, "gray64"),
               (2304, 8, 2, "gray256"), (2304, 8, 2, "rand256"), (5, 1, 3, "bpsk"), (2304, 1, 2, "bpsk"), (7, 2, 3, "qpsk"),
               (11, 4, 3, "rand16"), (11, 5, 3, "rand32"), (15, 7, 2, "rand128")]


@pytest.mark.parametrize("N,m,F,name", DEMAP_CASES)
def test_demap_host_equals_numpy_restatement(C, N, m, F, name):
    con = constellation(C, name)
    assert con.shape == (1 << m, 2)
    Ns = (N + m - 1) // m
    rx = make_rx(con, Ns, F, seed=N * 31 + m)
    for scale in (1.0, 1.0 / (2 * 0.3 * 0.3)):
        got = C.Demodulate_QAM_host(rx, con, scale, N)
        want = np_demap(rx, con, scale, N)
        assert got.shape == (N, F) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, m, F, name, scale)


def test_demap_host_ties(C):
    """An exact constellation point gives m0 or m1 = 0; a point equidistant from the two nearest points gives +0.0f, not -0.0f."""
    rx = np.array([[[0.0, 1.0], [1.0, 1.0], [0.0, 0.0], [-1.0, 0.0]]], np.float32)  # F = 1, Ns = 4, N = 8
    out = C.Demodulate_QAM_host(rx, QPSK, 2.5, 8).reshape(4, 2)  # [symbol][bit]
    assert np.array_equal(out.view(np.uint32), np_demap(rx, QPSK, 2.5, 8).reshape(4, 2).view(np.uint32))
    pz = np.float32(0.0).view(np.uint32)
    assert out[0, 0].view(np.uint32) == pz and out[0, 1] == np.float32(4.0 * 2.5)   # (0, 1): x undecided, y = +1 -> bit 1 is 0
    assert out[1, 0] == np.float32(4.0 * 2.5) and out[1, 1] == np.float32(4.0 * 2.5)  # the point (1, 1) itself: m0 = 0 for both bits
    assert out[2, 0].view(np.uint32) == pz and out[2, 1].view(np.uint32) == pz     # the origin: all four points tie
    assert out[3, 0] == np.float32(-4.0 * 2.5) and out[3, 1].view(np.uint32) == pz


MAP_CASES = [(1, 8, 1), (7, 3, 5), (2304, 6, 3), (4096, 6, 2), (2304, 8, 2), (2304, 1, 2), (9, 2, 4)]


@pytest.mark.parametrize("N,m,F", MAP_CASES)
def test_map_host_equals_formula(C, N, m, F):
    cw = np.random.default_rng(N + m).integers(0, 2, (N, F)).astype(np.int32)
    Ns = (N + m - 1) // m
    sym = C.Modulate_QAM_host(cw, N, m)
    assert sym.shape == (F, Ns) and sym.dtype == np.int32 and np.array_equal(sym, np_map(cw, N, F, m))
    pad = Ns * m - N
    if pad:  # the pad bits of the last symbol are sent as 0
        assert (sym[:, -1] >> (m - pad) == 0).all()
        ones = C.Modulate_QAM_host(np.ones((N, F), np.int32), N, m)
        assert (ones[:, :-1] == (1 << m) - 1).all() and (ones[:, -1] == (1 << (m - pad)) - 1).all()
    assert np.array_equal(C.Modulate_QAM_host(cw | 6, N, m), sym), "only bit 0 of an entry is read"
    zero = C.Modulate_QAM_host(None, N, m, F=F)  # CodeWord == NULL: the all-zero word
    assert zero.shape == (F, Ns) and not zero.any()


@pytest.mark.parametrize("N,m,F,name", [(7, 3, 5, "rand8"), (2304, 6, 3, "gray64"), (4096, 6, 2, "gray64"), (2304, 8, 2, "gray256"),
                                        (2304, 8, 2, "rand256"), (5, 1, 3, "bpsk")])
def test_noise_free_round_trip(C, N, m, F, name):
    con = constellation(C, name)
    cw = np.random.default_rng(7 * N + m).integers(0, 2, (N, F)).astype(np.int32)
    rx = con[C.Modulate_QAM_host(cw, N, m)]  # [F, Ns, 2]
    out = C.Demodulate_QAM_host(rx, con, 1.0, N)
    assert np.array_equal(out < 0, cw == 1) and (out != 0).all()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_checks(C):
    """Every refusal returns BLDPC_EINVAL with a message.  The device entry points check before they touch a device, so they are
    refused here too (the pointers are never followed)."""
    from cuda_ldpc_amd._lib import lib
    cw, sym = np.zeros((8, 2), np.int32), np.zeros((2, 4), np.int32)
    rx, con, out = np.zeros((2, 4, 2), np.float32), QPSK.copy(), np.zeros((8, 2), np.float32)
    f = ctypes.c_float

    def refused(rc, word):
        msg = lib.bldpc_last_error().decode()
        assert rc == BLDPC_EINVAL and word in msg, (rc, msg)

    for dev in (False, True):
        tail = (None,) if dev else ()
        fmap = lib.bldpc_qam_map if dev else lib.bldpc_qam_map_host
        fdem = lib.bldpc_qam_demap if dev else lib.bldpc_qam_demap_host
        name = "bldpc_qam_map" if dev else "bldpc_qam_map_host"
        refused(fmap(_ptr(cw), 8, 2, 2, None, *tail), "sym")
        refused(fmap(_ptr(cw), 0, 2, 2, _ptr(sym), *tail), "N=0")
        refused(fmap(_ptr(cw), 8, -1, 2, _ptr(sym), *tail), "F=-1")
        refused(fmap(_ptr(cw), 8, 2, 0, _ptr(sym), *tail), "m=0")
        refused(fmap(_ptr(cw), 8, 2, 9, _ptr(sym), *tail), "m=9")
        assert name + ":" in lib.bldpc_last_error().decode()
        refused(fdem(None, _ptr(con), 4, f(1), 8, 2, _ptr(out), *tail), "NULL")
        refused(fdem(_ptr(rx), None, 4, f(1), 8, 2, _ptr(out), *tail), "NULL")
        refused(fdem(_ptr(rx), _ptr(con), 4, f(1), 8, 2, None, *tail), "NULL")
        refused(fdem(_ptr(rx), _ptr(con), 4, f(1), 0, 2, _ptr(out), *tail), "N=0")
        refused(fdem(_ptr(rx), _ptr(con), 4, f(1), 8, 0, _ptr(out), *tail), "F=0")
        for q in (0, 1, 3, 48, 512, -4):
            refused(fdem(_ptr(rx), _ptr(con), q, f(1), 8, 2, _ptr(out), *tail), "q=%d" % q)
        for s in (np.inf, -np.inf, np.nan):
            refused(fdem(_ptr(rx), _ptr(con), 4, f(s), 8, 2, _ptr(out), *tail), "scale")
    assert lib.bldpc_qam_map_host(_ptr(cw), 8, 2, 2, _ptr(sym)) == 0
    assert lib.bldpc_qam_demap_host(_ptr(rx), _ptr(con), 4, f(1), 8, 2, _ptr(out)) == 0
    with pytest.raises(ValueError):
        C.Demodulate_QAM_host(rx, con[:3], 1.0, 8)
    with pytest.raises(ValueError):
        C.Demodulate_QAM_host(rx, con, 1.0, 9)  # 5 symbols needed, 4 given
    with pytest.raises(ValueError):
        C.Modulate_QAM_host(cw, 8, 9)


@pytest.mark.parametrize("N,m", [(2304, 6), (4096, 6), (2304, 8), (7, 3), (1, 8)])
def test_qam_draws_per_frame_is_what_the_channel_draws(C, N, m):
    """One frame of the QAM channel is Ns = ceil(N / m) samples of AWGNChannel_CPU: jumping a seed by qam_draws_per_frame gives the
    seed nbldpc_awgn_channel_host_sym leaves behind."""
    from cuda_ldpc_amd import sharding
    from cuda_ldpc_amd._lib import lib
    Ns = (N + m - 1) // m
    assert sharding.qam_draws_per_frame(N, m) == 4 * Ns
    seed = np.array([173, 4711, 99], np.int32)
    want = sharding.lcg_jump(seed, 3 * sharding.qam_draws_per_frame(N, m))
    tx, rx = np.zeros((Ns, 2), np.float32), np.zeros((Ns, 2), np.float32)
    for _ in range(3):  # three frames
        assert lib.nbldpc_awgn_channel_host_sym(_ptr(seed), ctypes.c_float(0.5), _ptr(tx), Ns, _ptr(rx)) == 0
    assert np.array_equal(seed, want)


def test_simulation_refuses_before_touching_a_device(C):
    """The ValueErrors of Simulation_GPU(n_QAM != 2) come before the first use of the code object or of a device: no GPU here."""
    from cuda_ldpc_amd.simulation import Simulation_GPU
    con = constellation(C, "gray64")
    seed = np.array([173, 173, 173], np.int32)
    base = dict(Num_Frames_OneTime=16, max_batches=1, log=None, schedule="layered", exit_mode=C.EXIT_PER_FRAME)
    with pytest.raises(ValueError, match="not symmetric"):
        Simulation_GPU(None, seed, 0.3, C.SimCounters(), n_QAM=64, CONSTELLATION=con, PN_Message=0, device_channel=True, **base)
    with pytest.raises(ValueError, match="device_channel"):
        Simulation_GPU(None, seed, 0.3, C.SimCounters(), n_QAM=64, CONSTELLATION=con, PN_Message=1, device_channel=False, **base)
    with pytest.raises(ValueError, match="CONSTELLATION"):
        Simulation_GPU(None, seed, 0.3, C.SimCounters(), n_QAM=64, CONSTELLATION=None, PN_Message=1, device_channel=True, **base)
    with pytest.raises(ValueError, match="CONSTELLATION"):
        Simulation_GPU(None, seed, 0.3, C.SimCounters(), n_QAM=64, CONSTELLATION=con[:16], PN_Message=1, device_channel=True, **base)
    with pytest.raises(ValueError, match="CONSTELLATION"):
        Simulation_GPU(None, seed, 0.3, C.SimCounters(), n_QAM=256, CONSTELLATION=con, PN_Message=1, device_channel=True, **base)
    assert np.array_equal(seed, [173, 173, 173])


def test_sweep_binary_qam_needs_pn_message():
    """sweep.py binary --qam 64 used to ignore the flag; now it refuses, before any device is opened, unless random codewords and the
    device channel are asked for."""
    for extra in ([], ["--layered", "--per-frame", "--device-channel"], ["--fixed", "--pn-message"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "sweep.py"), "binary", "--qam", "64"] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "error:" in r.stderr and "--pn-message" in r.stderr and "--device-channel" in r.stderr, (extra, r.stderr)
