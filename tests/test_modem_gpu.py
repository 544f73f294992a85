"""GPU tests of the QAM bit mapper and max-log demapper (bldpc_qam_map / bldpc_qam_demap): every output bit against the host
statements, which tests/test_modem_cpu.py holds against a numpy restatement of include/bldpc.h; the noise-free chain through both
decoders; Simulation_GPU over 64-QAM against the same calls in a plain loop, unsharded and as two ranks."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
CON = os.path.join(DATA, "nb", "Constellation")


def constellation(C, name):
    """float32 [q, 2]: "gray64" / "gray256" / "bpsk" from the shipped files, "qpsk", or "rand<q>": seeded, no product structure."""
    if name.startswith("gray"):
        return C.Get_CONSTELLATION(os.path.join(CON, "GRAY_%sQAM.txt" % name[4:]), int(name[4:]))
    if name == "bpsk":
        return C.Get_CONSTELLATION(os.path.join(CON, "BPSK.txt"), 2)
    if name == "qpsk":
        return np.array([[1, 1], [-1, 1], [1, -1], [-1, -1]], np.float32)
    q = int(name[4:])
    return np.random.default_rng(1000 + q).normal(0.0, 0.75, (q, 2)).astype(np.float32)


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes = {}


def _code(C, fn):
    if fn not in _codes:
        J, L, Z = (int(x[1:]) for x in fn.split("_")[:3])
        _codes[fn] = C.BinaryCode.from_blockh(os.path.join(BL, fn), J, L, Z)
    return _codes[fn]


# (N, m) of the issue with every constellation of 2^m points that is tested: tile interiors, tails, pad bits, one symbol, one bit per symbol
SHAPES = [(1, 8, "gray256"), (1, 8, "rand256"), (7, 3, "rand8"), (2304, 6, "gray64"), (4096, 6, "gray64"), (2304, 8, "gray256"),
          (2304, 8, "rand256"), (2304, 1, "bpsk")]


# the sizes of q the list above leaves out, each with its own kernel instance; q = 128 is the two-chunk case with one upper index bit.
# N = 2303 is no multiple of any of these m (pad bits) and spans three symbol tiles; F = 65 is a full frame tile and a tail of one.
OTHER_Q = [(2303, 2, "qpsk"), (2303, 4, "rand16"), (2303, 5, "rand32"), (2303, 7, "rand128")]


@pytest.mark.parametrize("N,m,name,F", [s + (F,) for s in SHAPES for F in (1, 63, 65, 257)] + [s + (65,) for s in OTHER_Q])
def test_kernels_equal_host_statements(C, N, m, name, F):
    from cuda_ldpc_amd import sharding
    con = constellation(C, name)
    cond = torch.from_numpy(con).cuda()
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + m * 10 + F)
    cw = torch.randint(0, 2, (N, F), generator=g, device="cuda", dtype=torch.int32)
    sym = C.Modulate_QAM(cw, N, m)
    want_sym = C.Modulate_QAM_host(cw.cpu().numpy(), N, m)
    assert sym.shape == want_sym.shape and np.array_equal(sym.cpu().numpy(), want_sym), "map"
    seed = np.array([173, 173, 173], np.int32)
    Ns = (N + m - 1) // m
    rx = C.AWGNChannel_QAM_GPU(seed, 0.25, sym, cond)  # moderate noise: a good share of the points leave their decision region
    assert np.array_equal(seed, sharding.lcg_jump([173, 173, 173], sharding.qam_draws_per_frame(N, m) * F))
    rxh = rx.cpu().numpy()
    assert rxh.shape == (F, Ns, 2)
    for scale in (1.0, 1.0 / (2 * 0.25 * 0.25)):
        got = C.Demodulate_QAM(rx, cond, scale, N)
        torch.cuda.synchronize()
        want = C.Demodulate_QAM_host(rxh, con, scale, N)
        g_ = got.cpu().numpy()
        assert g_.shape == (N, F) and np.array_equal(g_.view(np.uint32), want.view(np.uint32)), "demap scale=%g" % scale


def test_map_all_zero_word_and_guard_rows(C):
    """CodeWord = NULL gives index 0 everywhere; neither kernel writes outside its output (guard elements around both stay as set)."""
    N, m, F = 4096, 6, 65
    Ns = (N + m - 1) // m
    sym = C.Modulate_QAM(None, N, m, F=F)
    assert sym.shape == (F, Ns) and sym.dtype == torch.int32 and not sym.any()
    assert np.array_equal(C.Modulate_QAM_host(None, N, m, F=F), sym.cpu().numpy())
    from cuda_ldpc_amd._lib import check, lib
    import ctypes
    cw = torch.ones((N, F), dtype=torch.int32, device="cuda")
    buf = torch.full((F * Ns + 128,), -7, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.bldpc_qam_map(ctypes.c_void_p(cw.data_ptr()), N, F, m, ctypes.c_void_p(buf[64:].data_ptr()), st), "map")
    assert (buf[:64] == -7).all() and (buf[64 + F * Ns:] == -7).all()
    assert np.array_equal(buf[64:64 + F * Ns].reshape(F, Ns).cpu().numpy(), C.Modulate_QAM_host(np.ones((N, F), np.int32), N, m))
    con = torch.from_numpy(constellation(C, "gray64")).cuda()
    rx = con[buf[64:64 + F * Ns].reshape(F, Ns).long()].contiguous()
    obuf = torch.full((N * F + 128,), 123.0, device="cuda")
    check(lib.bldpc_qam_demap(ctypes.c_void_p(rx.data_ptr()), ctypes.c_void_p(con.data_ptr()), 64, ctypes.c_float(1.0), N, F,
                              ctypes.c_void_p(obuf[64:].data_ptr()), st), "demap")
    torch.cuda.synchronize()
    assert (obuf[:64] == 123.0).all() and (obuf[64 + N * F:] == 123.0).all() and (obuf[64:64 + N * F] < 0).all()


@pytest.mark.parametrize("fn,F,q", [("J4_L24_Z96_BlockH.txt", 130, 64), ("J32_L64_Z64_BlockH.txt", 66, 64), ("J4_L24_Z96_BlockH.txt", 66, 256)])
def test_end_to_end_without_noise(C, fn, F, q):
    code = _code(C, fn)
    m = q.bit_length() - 1
    con = constellation(C, "gray%d" % q)
    cond = torch.from_numpy(con).cuda()
    cw = C.PN_CodeWords(code, 99, F)
    sym = C.Modulate_QAM(cw, code.N, m)
    seed = np.array([173, 173, 173], np.int32)
    rx = C.AWGNChannel_QAM_GPU(seed, 0.0, sym, cond)
    assert torch.equal(rx, cond[sym.long()]), "sigma = 0: the constellation points themselves (0 * cos * amp + c is exact)"
    y = C.Demodulate_QAM(rx, cond, 1.0, code.N)
    assert torch.equal((y < 0).int(), cw) and bool((y != 0).all())
    r = C.LDPC_Decoder_GPU(code, y, max_iter=1, exit_mode=C.EXIT_FIXED)
    C.Syndrome(code, r["D"], into_flag_row=True)  # the flooding decoders' own flag tests for the all-zero word
    assert r["iteraTime"] == 1 and torch.equal(r["D"][:code.N], cw) and bool((r["D"][code.N] == 1).all())
    r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=25, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert torch.equal(r["D"][:code.N], cw) and bool((r["D"][code.N] == 1).all()) and bool((r["iters"] == 1).all())


class _Rank:
    """One rank of a world of `world`, without a process group: every rank runs in this process in turn and the all-reduce is the sum
    the test makes of their counters."""

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


SIM_EBN0 = 10.0  # dB: the middle of the waterfall of J4_L24_Z96 over 64-QAM (the host statements lose about 200 of these 512 frames, 17 at 10.5 dB)


def test_simulation_qam_counters_and_sharding(C):
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd.simulation import Simulation_GPU
    code = _code(C, "J4_L24_Z96_BlockH.txt")
    F, batches, maxIT, pn_seed, alpha, q, m = 256, 2, 25, 31337, 0.75, 64, 6
    con = constellation(C, "gray64")
    cond = torch.from_numpy(con).cuda()
    sigma = nb.sigma_of(SIM_EBN0, code.K / code.N, 0, q)
    kw = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=batches, log=None, PN_Message=1, pn_seed=pn_seed,
              schedule="layered", alpha=alpha, device_channel=True, n_QAM=q, CONSTELLATION=con, leastTestFrames=10 ** 9)

    def run(dist):
        SIM, seed = C.SimCounters(), np.array([173, 173, 173], np.int32)
        Simulation_GPU(code, seed, sigma, SIM, dist=dist, **kw)
        assert SIM.num_Frames == F * batches
        return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames], seed

    got, got_seed = run(None)
    seed = np.array([173, 173, 173], np.int32)
    tot = np.zeros(5, np.int64)
    for b in range(batches):  # the same batch from the primitive calls, counted in numpy
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
        rx = C.AWGNChannel_QAM_GPU(seed, sigma, C.Modulate_QAM(cw, code.N, m), cond)
        y = C.Demodulate_QAM(rx, cond, 1.0 / (2.0 * sigma * sigma), code.N)
        r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=maxIT, alpha=alpha, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        D, cwn, it = r["D"].cpu().numpy(), cw.cpu().numpy(), r["iters"].cpu().numpy()
        errs = (D[:code.K] != cwn[:code.K]).sum(0)
        ok = D[code.N] != 0
        tot += [np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)]
    print("64-QAM Eb/N0 %.2f dB sigma %.5f: counters %s" % (SIM_EBN0, sigma, got))
    assert got == tot.tolist() and np.array_equal(got_seed, seed)
    assert 0 < got[0] < F * batches and got[2] < maxIT * F * batches
    parts = [run(_Rank(r, 2)) for r in range(2)]  # world size 2: each rank decodes its half of every batch
    assert [a + b for a, b in zip(parts[0][0], parts[1][0])] == got
    assert np.array_equal(parts[0][1], got_seed) and np.array_equal(parts[1][1], got_seed)
