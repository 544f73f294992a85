"""GPU tests of the layered normalised min-sum decoder (bldpc_decode_layered): every output bit against
bldpc_decode_layered_host, which tests/test_layered_cpu.py holds against a numpy restatement of the specification."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA, GOLDEN
from test_layered_cpu import special_inputs

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
PON = ("PON_LDPC.txt", 12, 69, 256)


def _dims(fn):
    if fn == PON[0]:
        return PON[1:]
    return tuple(int(x[1:]) for x in fn.split("_")[:3])


ALL = sorted(f for f in os.listdir(BL) if f.endswith(".txt"))
BENCH = {"J4_L24_Z96_BlockH.txt": 65536, "J32_L64_Z64_BlockH.txt": 32768}  # bench.py's frames per GPU


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_cache = {}


def _code(C, fn):
    if fn not in _cache:
        J, L, Z = _dims(fn)
        H, _, _ = C.Get_H(os.path.join(BL, fn), J, L)
        _cache[fn] = (C.BinaryCode.from_shifts(H, J, L, Z), H)
    return _cache[fn]


def _noise(C, N, F, snr):
    return C.AWGNChannel_CPU(np.array([173, 173, 173], np.int32), C.sigma_of(snr), N, F)


def _both(C, fn, y, **kw):
    """The device and the host decoder on the same input: all outputs must carry the same bits."""
    code, H = _code(C, fn)
    r = C.LDPC_Decoder_Layered_GPU(code, torch.from_numpy(y).cuda(), want_app=True, **kw)
    torch.cuda.synchronize()
    want = C.layered_host(H, code.J, code.L, code.Z, y, **kw)
    what = "%s F=%d %s" % (fn, y.shape[1], kw)
    assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    D = r["D"].cpu().numpy()
    assert np.array_equal(D[code.N], want["D"][code.N]), "flag row: " + what
    assert np.array_equal(D[:code.N], want["D"][:code.N]), "hard bits: " + what
    assert np.array_equal(r["app"].cpu().numpy().view(np.uint32), want["app"].view(np.uint32)), "a-posteriori bits: " + what
    return r, want


SNR = {4: 2.6, 6: 1.5, 8: 0.5, 12: -0.5, 32: -0.5, 10: 2.5, 15: 0.0, 20: -1.0, 24: -1.5, 30: -2.0, 36: -2.5, 40: -3.0, 48: -3.5}


@pytest.mark.parametrize("fn", ALL)
def test_all_matrices_match_host(C, fn):
    code, _ = _code(C, fn)
    y = _noise(C, code.N, 5, SNR.get(code.J, 1.0))
    _both(C, fn, y, max_iter=6, alpha=0.75)
    r, want = _both(C, fn, y, max_iter=12, alpha=1.0, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert code.last_kernel in ("k_lay_reg", "k_lay", "k_lay_ws")
    if fn.startswith("J15_L30_Z1280"):
        assert code.last_kernel == "k_lay_ws"


@pytest.mark.parametrize("fn", list(BENCH))
def test_bench_codes_run_the_fused_kernel(C, fn):
    code, _ = _code(C, fn)
    _both(C, fn, _noise(C, code.N, 4, 3.0), max_iter=3)
    assert code.last_kernel in ("k_lay_reg", "k_lay"), code.last_kernel


@pytest.mark.parametrize("alpha", [1.0, 0.75, 0.8])
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("fn", list(BENCH))
def test_modes_rules_alphas_ragged_batches(C, fn, mode, rule, alpha):
    code, _ = _code(C, fn)
    for F in (1, 3, 37, 61):
        y = _noise(C, code.N, F, 2.6 if code.J == 4 else -0.5)
        r, want = _both(C, fn, y, max_iter=10, alpha=alpha, exit_mode=mode, stop_rule=rule)
    if mode == 2:
        it = want["iters"]
        assert (it < 10).any(), "the case must hold frames that stop early"


@pytest.mark.parametrize("fn", list(BENCH))
def test_one_more_than_a_multiple_of_the_workgroup(C, fn):
    code, _ = _code(C, fn)
    for F in (2520 + 1,):  # 2520 = lcm(1 .. 10): a multiple of any frames-per-workgroup up to 10
        y = np.ascontiguousarray(np.tile(_noise(C, code.N, 61, 2.6 if code.J == 4 else -0.5), (1, 42))[:, :F])
        r = C.LDPC_Decoder_Layered_GPU(code, torch.from_numpy(y).cuda(), max_iter=8, alpha=0.75, exit_mode=C.EXIT_PER_FRAME,
                                       stop_rule=C.STOP_SYNDROME, want_app=True)
        torch.cuda.synchronize()
        _, H = _code(C, fn)
        want = C.layered_host(H, code.J, code.L, code.Z, y[:, :61], max_iter=8, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        idx = np.arange(F) % 61
        assert np.array_equal(r["D"].cpu().numpy(), want["D"][:, idx])
        assert np.array_equal(r["iters"].cpu().numpy(), want["iters"][idx])
        assert np.array_equal(r["app"].cpu().numpy().view(np.uint32), want["app"].view(np.uint32)[:, idx])


@pytest.mark.parametrize("fn", list(BENCH) + ["J8_L24_Z96_BlockH.txt", "J15_L30_Z1280_BlockH.txt"])
def test_special_values(C, fn):
    code, _ = _code(C, fn)
    y = special_inputs(code.N, 8, np.random.default_rng(7))
    for alpha in (1.0, 0.75, 0.8):
        _both(C, fn, y, max_iter=5, alpha=alpha)
    _both(C, fn, y, max_iter=5, alpha=0.8, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)


@pytest.mark.parametrize("fn", list(BENCH))
def test_full_size_batch(C, fn):
    """bench.py's batch: the first tile against the host function, every other tile equal to it (the input is tiled)."""
    code, H = _code(C, fn)
    F, T = BENCH[fn], 256
    tile = _noise(C, code.N, T, 3.0 if code.J == 4 else 0.0)
    y = torch.from_numpy(tile).cuda().repeat(1, F // T).contiguous()
    for kw in (dict(max_iter=25, alpha=0.75), dict(max_iter=25, alpha=1.0, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)):
        r = C.LDPC_Decoder_Layered_GPU(code, y, want_app=True, **kw)
        torch.cuda.synchronize()
        want = C.layered_host(H, code.J, code.L, code.Z, tile, **kw)
        D = r["D"].view(code.N + 1, F // T, T)
        assert np.array_equal(D[:, 0].cpu().numpy(), want["D"])
        assert bool((D == D[:, :1]).all())
        app = r["app"].view(torch.int32).view(code.N, F // T, T)
        assert np.array_equal(app[:, 0].cpu().numpy().view(np.uint32), want["app"].view(np.uint32))
        assert bool((app == app[:, :1]).all())
        it = r["iters"].view(F // T, T)
        assert np.array_equal(it[0].cpu().numpy(), want["iters"]) and bool((it == it[:1]).all())


@pytest.mark.parametrize("fn", ["J4_L24_Z96_BlockH.txt", "J24_L60_Z160_BlockH.txt"])
def test_random_codewords_with_syndrome_stop(C, fn):
    code, H = _code(C, fn)
    F = 300  # Es/N0 2.8 dB (rate 5/6) and 2.0 dB (rate 0.6): both well inside the region where min-sum converges
    cw = C.PN_CodeWords(code, 77, F)
    y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), C.sigma_of(2.8 if code.J == 4 else 2.0), code.N, F, CodeWord=cw)
    r = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=20, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    flag = r["D"][code.N].clone()
    syn = C.Syndrome(code, r["D"].clone(), into_flag_row=False)
    torch.cuda.synchronize()
    assert torch.equal(flag, syn["flag"])
    ok = flag.bool()
    assert ok.sum() > F // 2
    it = r["iters"]
    assert bool((it[~ok] == 20).all()) and bool((it[ok] <= 20).all())
    good = (r["D"][:code.N] == cw).all(0)
    assert (good & ok).sum() > F // 2 and bool((good[ok].float().mean() > 0.9)), "converged frames are the sent words (up to undetected errors)"
    _both(C, fn, y.cpu().numpy(), max_iter=20, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)


def test_simulation_layered_pn_message_counters(C):
    from cuda_ldpc_amd.simulation import Simulation_GPU
    fn = "J4_L24_Z96_BlockH.txt"
    code, H = _code(C, fn)
    F, batches, maxIT, pn_seed, snr, alpha = 512, 3, 20, 4242, 2.4, 0.75
    sigma = C.sigma_of(snr, 1, code.K / code.N)
    SIM = C.SimCounters()
    Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, SIM, Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME,
                   max_batches=batches, log=None, PN_Message=1, pn_seed=pn_seed, schedule="layered", alpha=alpha)
    got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
    seed = np.array([173, 173, 173], np.int32)
    tot = np.zeros(5, np.int64)
    for b in range(batches):  # the same calls in a plain loop, counted in numpy
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
        y = C.AWGNChannel_CPU(seed, sigma, code.N, F, CodeWord=cw.cpu().numpy())
        r = C.LDPC_Decoder_Layered_GPU(code, torch.from_numpy(y).cuda(), max_iter=maxIT, alpha=alpha, exit_mode=C.EXIT_PER_FRAME,
                                       stop_rule=C.STOP_SYNDROME)
        D, cwn, it = r["D"].cpu().numpy(), cw.cpu().numpy(), r["iters"].cpu().numpy()
        errs = (D[:code.K] != cwn[:code.K]).sum(0)
        ok = D[code.N] != 0
        tot += [np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)]
    assert SIM.num_Frames == F * batches
    assert got == tot.tolist()
    assert 0 < got[0] < F * batches and got[2] < maxIT * F * batches


def test_refusals_on_the_device(C):
    from cuda_ldpc_amd._lib import LdpcError
    fn = "J4_L24_Z96_BlockH.txt"
    code, H = _code(C, fn)
    y = torch.ones((code.N, 4), device="cuda")
    for kw, rc in ((dict(max_iter=0), -1), (dict(alpha=0.0), -1), (dict(alpha=1.25), -1), (dict(alpha=float("nan")), -1),
                   (dict(stop_rule=3), -1), (dict(exit_mode=C.EXIT_BATCH_GLOBAL), -1), (dict(exit_mode=9), -1)):
        with pytest.raises(LdpcError, match=r"\(%d\): .*\S" % rc):
            C.LDPC_Decoder_Layered_GPU(code, y, **kw)
    J, L, Z = _dims(fn)
    _, wc, wv = C.Get_H(os.path.join(BL, fn), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    H1 = H.copy().reshape(J, L)
    H1[2, 1:] = -1
    H1[2, 0] = 0  # block row 2: weight 1
    thin = C.BinaryCode.from_shifts(H1.reshape(-1), J, L, Z)
    for bad, text in ((table, "address table"), (thin, r"weight 1\b")):  # the same answer on the second call
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(-5\): .*" + text) as e:
                C.LDPC_Decoder_Layered_GPU(bad, y)
            said.append(str(e.value))
        assert said[0] == said[1]
    import ctypes
    D = torch.empty((code.N + 1, 4), dtype=torch.int32, device="cuda")
    it = torch.empty(4, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(F, max_iter, alpha, length):  # past the wrapper's own checks: F = 0 never reaches C through it
        rc = C._lib.lib.bldpc_decode_layered(code._h, ctypes.c_void_p(y.data_ptr()), F, max_iter, ctypes.c_float(alpha), length, C.EXIT_FIXED,
                                             C.STOP_PREFIX, ctypes.c_void_p(D.data_ptr()), None, ctypes.c_void_p(it.data_ptr()), st)
        return rc, C._lib.lib.bldpc_last_error().decode()

    # two faults at once: the first one in the order of the checks is the one reported (F, max_iter, alpha, length)
    who = "bldpc_decode_layered"
    assert raw(0, 5, 0.0, 0) == (-1, who + ": F=0 must be positive")
    assert raw(4, 5, 2.0, -1) == (-1, who + ": alpha=2 outside (0, 1]")
    assert raw(4, 0, 2.0, -1) == (-1, who + ": max_iter=0 must be at least 1")
    with pytest.raises(ValueError):
        C.LDPC_Decoder_Layered_GPU(code, y, D=torch.empty((code.N, 4), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("fn", ["bldpc_J4_L24_Z96_3dB_cor.npz", "bldpc_J32_L64_Z64_-1dB_cor.npz"])
def test_flooding_unchanged_around_a_layered_call(C, fn):
    """The committed flooding fixture decoded before and after a layered call on the same code object."""
    g = np.load(os.path.join(GOLDEN, fn))
    J, L, Z, F = int(g["J"]), int(g["L"]), int(g["Z"]), int(g["F"])
    code = C.BinaryCode.from_blockh(os.path.join(BL, "J%d_L%d_Z%d_BlockH.txt" % (J, L, Z)), J, L, Z)
    yt = torch.from_numpy(np.ascontiguousarray(g["y"]).reshape(code.N, F)).cuda()
    want = np.unpackbits(g["D_bits"])[: code.N * F].astype(np.int32)

    def flood():
        r = C.LDPC_Decoder_GPU(code, yt, max_iter=50, exit_mode=C.EXIT_BATCH_GLOBAL, want_app=True)
        torch.cuda.synchronize()
        D = r["D"].cpu().numpy().reshape(-1)
        assert r["iteraTime"] == int(g["it"])
        assert np.array_equal(D[: code.N * F], want) and np.array_equal(D[code.N * F:], g["flags"])
        return r["app"].clone()

    a0 = flood()
    C.LDPC_Decoder_Layered_GPU(code, yt, max_iter=7, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
    a1 = flood()
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32))
    assert code.last_kernel.startswith("qc_lds")
