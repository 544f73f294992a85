"""GPU tests of bldpc_decode_layered_quant: the two kernel tiers against the host statement bldpc_decode_layered_quant_host, exactly,
on iters, flag row, hard bits and a-posteriori words, on the random block matrices of tests/test_layered_shapes_cpu.py with the inputs
and parameter sets of tests/quant_cases.py (tests/test_quant_cpu.py holds the host statement against the numpy restatement on the same
cases and checks that the inputs meet their conditions), on shipped matrices, with special values, a caller's D on a second stream,
scratch that shrinks and grows, the other decoders of a code object around a quantised call, the refusals the device makes, and
Simulation_GPU / Simulation_HARQ_GPU with schedule="quant" against their host twins."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from quant_cases import ACCEPTED, BY_DIMS, F_PAIR, FIXED_ITER, MAX_ITER, PARAMS, TIER, input_for, pair_input, special_input
from test_layered_shapes_cpu import matrix_of, shape_id

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
BATCHES = (1, F_PAIR)  # a lone frame; 37 leaves a half-empty pair and a partly filled last workgroup


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes, _inputs, _host = {}, {}, {}


def _code(C, s, fresh=False):
    J, L, Z = s[:3]
    if fresh:
        return C.BinaryCode.from_shifts(matrix_of(s), J, L, Z)
    if s[:3] not in _codes:
        _codes[s[:3]] = C.BinaryCode.from_shifts(matrix_of(s), J, L, Z)
    return _codes[s[:3]]


def _input(s, kind, F, name):
    """(host array, device tensor) of the shape's input: computed once, shared, never written to."""
    special = kind == "special"
    key = (s[:3], kind, F, name if special else None)
    if key not in _inputs:
        N = s[1] * s[2]
        y = special_input(N, F, PARAMS[name]) if special else input_for(s)[:, :F]
        y = np.ascontiguousarray(y)
        y.setflags(write=False)
        _inputs[key] = (y, torch.from_numpy(y.copy()).cuda())
    return _inputs[key]


def _want(C, s, kind, F, name, **kw):
    """The host decoder's result: computed once per case, shared among the tests."""
    key = (s[:3], kind, F, name, tuple(sorted(kw.items())))
    if key not in _host:
        J, L, Z = s[:3]
        _host[key] = C.quant_host(matrix_of(s), J, L, Z, _input(s, kind, F, name)[0], C.Quant(*PARAMS[name]), **kw)
    return _host[key]


def _same(code, r, want, what):
    assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    D = r["D"].cpu().numpy()
    assert np.array_equal(D[code.N], want["D"][code.N]), "flag row: " + what
    assert np.array_equal(D[:code.N], want["D"][:code.N]), "hard bits: " + what
    assert r["app"].dtype == torch.int32 and np.array_equal(r["app"].cpu().numpy(), want["app"]), "a-posteriori words: " + what


def _both(C, s, kind, F, name, code=None, **kw):
    """The device and the host decoder on the same input: all outputs must be equal."""
    code = code or _code(C, s)
    r = C.LDPC_Decoder_Quant_GPU(code, _input(s, kind, F, name)[1], C.Quant(*PARAMS[name]), want_app=True, **kw)
    torch.cuda.synchronize()
    want = _want(C, s, kind, F, name, **kw)
    _same(code, r, want, "%s %s F=%d %s %s" % (shape_id(s), kind, F, name, kw))
    return r, want


def _rules(C, s):
    return [dict(stop_rule=C.STOP_SYNDROME), dict(stop_rule=C.STOP_PREFIX, length=0), dict(stop_rule=C.STOP_PREFIX, length=s[1] * s[2])]


@pytest.mark.parametrize("s", ACCEPTED, ids=shape_id)
def test_random_shapes_match_host(C, s):
    code = _code(C, s)
    for name in ("P0", "P3"):
        for F in BATCHES:
            for mode, max_iter in ((C.EXIT_FIXED, FIXED_ITER), (C.EXIT_PER_FRAME, MAX_ITER)):
                for rule in _rules(C, s):
                    _both(C, s, "pair", F, name, max_iter=max_iter, exit_mode=mode, **rule)
                    assert code.last_kernel == TIER[s[:3]], "%s ran %s" % (shape_id(s), code.last_kernel)


@pytest.mark.parametrize("dims", [(3, 8, 1056), (5, 12, 32), (4, 27, 64)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_special_values_on_every_tier(C, dims):
    """Half-way products, zeros of both signs, denormals, the quantiser's edges, 2^100 and a frame of ties on one shape of each tier;
    on (4, 27, 64) they meet the block rows of weight 2, 3 and 26."""
    s = BY_DIMS[dims]
    code = _code(C, s)
    if dims == (4, 27, 64):
        assert {2, 3, 26} <= set((matrix_of(s) != -1).sum(1).tolist())
    for name in ("P1", "P2", "P4"):
        _both(C, s, "special", 8, name, max_iter=FIXED_ITER)
        _both(C, s, "special", 8, name, max_iter=MAX_ITER, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        assert code.last_kernel == TIER[dims]


def _shipped(C, name, J, L, Z, F, P, **kw):
    H, _, _ = C.Get_H(os.path.join(BL, name), J, L)
    code = C.BinaryCode.from_blockh(os.path.join(BL, name), J, L, Z)
    y = pair_input(L * Z, F)
    q = C.Quant(*P)
    r = C.LDPC_Decoder_Quant_GPU(code, torch.from_numpy(y).cuda(), q, want_app=True, **kw)
    torch.cuda.synchronize()
    want = C.quant_host(H, J, L, Z, y, q, **kw)
    _same(code, r, want, "%s %s" % (name, kw))
    return code, want


@pytest.mark.parametrize("name,J,L,Z", [("J4_L24_Z96_BlockH.txt", 4, 24, 96), ("J32_L64_Z64_BlockH.txt", 32, 64, 64)])
def test_shipped_codes(C, name, J, L, Z):
    code, want = _shipped(C, name, J, L, Z, 64, PARAMS["P1"], max_iter=MAX_ITER, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert code.last_kernel == "k_lq"
    assert np.unique(want["iters"]).size >= 3
    code.close()


def test_shipped_J15_L30_Z1280_runs_the_workspace_kernel(C):
    code, _ = _shipped(C, "J15_L30_Z1280_BlockH.txt", 15, 30, 1280, 3, PARAMS["P1"], max_iter=FIXED_ITER)
    assert code.last_kernel == "k_lq_ws"
    code.close()


def test_caller_provided_D_on_another_stream(C):
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s)
    kw = dict(max_iter=MAX_ITER, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    r0, want = _both(C, s, "pair", F_PAIR, "P0", **kw)
    yt = _input(s, "pair", F_PAIR, "P0")[1]
    D = torch.full((code.N + 1, F_PAIR), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # D is filled and yt uploaded on the current stream
    r = C.LDPC_Decoder_Quant_GPU(code, yt, C.Quant(*PARAMS["P0"]), D=D, want_app=True, stream=stream, **kw)
    stream.synchronize()
    assert r["D"] is D
    _same(code, r, want, "D= and stream=")
    assert torch.equal(r["D"], r0["D"]) and torch.equal(r["iters"], r0["iters"]) and torch.equal(r["app"], r0["app"])


@pytest.mark.parametrize("dims", [(5, 12, 32), (32, 34, 288)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_scratch_that_shrinks_and_grows(C, dims):
    """One code object of its own, whose scratch and row-state workspace are sized by the largest call: 37 frames, then 1, then 37."""
    s = BY_DIMS[dims]
    code = _code(C, s, fresh=True)
    for F in (F_PAIR, 1, F_PAIR):
        _both(C, s, "pair", F, "P0", code=code, max_iter=MAX_ITER, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        _both(C, s, "pair", F, "P0", code=code, max_iter=FIXED_ITER)
    assert code.last_kernel == TIER[dims]
    code.close()


def _thin(C):
    J, L, Z = 4, 24, 96
    H, _, _ = C.Get_H(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L)
    H = H.copy().reshape(J, L)
    H[2, 1:] = -1
    H[2, 0] = 0  # block row 2: weight 1
    return C.BinaryCode.from_shifts(H.reshape(-1), J, L, Z)


def test_other_decoders_unchanged_around_a_quantised_call(C):
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s, fresh=True)
    y = _input(s, "pair", F_PAIR, "P0")[1]

    def others(c, yy):
        a = C.LDPC_Decoder_GPU(c, yy, max_iter=8, exit_mode=C.EXIT_FIXED, want_app=True)
        out = [a["D"].clone(), a["app"].view(torch.int32).clone()]
        try:
            b = C.LDPC_Decoder_Layered_GPU(c, yy, max_iter=6, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
            out += [b["D"].clone(), b["app"].view(torch.int32).clone(), b["iters"].clone()]
            b = C.LDPC_Decoder_BP_GPU(c, yy, max_iter=6, llr_scale=2.0, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
            out += [b["D"].clone(), b["app"].view(torch.int32).clone(), b["iters"].clone()]
        except C._lib.LdpcError:
            out.append(None)  # the thin-row matrix: refused before and after alike
        torch.cuda.synchronize()
        return out

    def equal(p, q):
        return len(p) == len(q) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(p, q))

    before = others(code, y)
    assert len(before) == 8
    _both(C, s, "pair", F_PAIR, "P0", code=code, max_iter=MAX_ITER, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert equal(others(code, y), before)
    code.close()
    # and after a refused call
    thin = _thin(C)
    yt = torch.ones((thin.N, 5), device="cuda")
    before = others(thin, yt)
    assert before[-1] is None
    said = []
    for _ in range(2):
        with pytest.raises(C._lib.LdpcError, match=r"\(-5\): .*weight 1\b.*") as e:
            C.LDPC_Decoder_Quant_GPU(thin, yt, C.Quant())
        said.append(str(e.value))
    assert said[0] == said[1]
    assert equal(others(thin, yt), before)
    thin.close()


def test_refusals_on_the_device(C):
    from cuda_ldpc_amd._lib import LdpcError, bldpc_quant
    import ctypes
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s)
    y = torch.ones((code.N, 4), device="cuda")
    good = C.Quant()
    cases = [(good, dict(max_iter=0)), (good, dict(length=code.N + 1)), (good, dict(length=-1)), (good, dict(stop_rule=3)),
             (good, dict(exit_mode=C.EXIT_BATCH_GLOBAL)), (good, dict(exit_mode=9)), (None, {}),
             (bldpc_quant(0.0, 6, 8, 6, 6, 0), {}), (bldpc_quant(float("nan"), 6, 8, 6, 6, 0), {}), (bldpc_quant(16.0, 9, 8, 6, 6, 0), {}),
             (bldpc_quant(16.0, 6, 16, 6, 6, 0), {}), (bldpc_quant(16.0, 6, 8, 9, 6, 0), {}), (bldpc_quant(16.0, 6, 8, 6, 9, 0), {}),
             (bldpc_quant(16.0, 6, 8, 6, 6, 32), {}), (bldpc_quant(16.0, 1, 8, 6, 6, 0), {}), (bldpc_quant(16.0, 6, 8, 6, 0, 0), {}),
             (bldpc_quant(16.0, 6, 8, 6, 6, -1), {}), (bldpc_quant(16.0, 6, 5, 6, 6, 0), {}), (bldpc_quant(16.0, 6, 8, 1, 6, 0), {})]
    for q, kw in cases:
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(-1\): .*\S") as e:
                C.LDPC_Decoder_Quant_GPU(code, y, q, **kw)
            said.append(str(e.value))
        assert said[0] == said[1], kw
    D = torch.empty((code.N + 1, 4), dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = C._lib.lib.bldpc_decode_layered_quant(code._h, ctypes.c_void_p(y.data_ptr()), 4, 5, ctypes.byref(good.c_struct()), 0, C.EXIT_PER_FRAME,
                                               C.STOP_PREFIX, ctypes.c_void_p(D.data_ptr()), None, None, st)
    assert rc == -1 and b"iters" in C._lib.lib.bldpc_last_error()
    it = torch.empty(4, dtype=torch.int32, device="cuda")

    def raw(F, max_iter, q, length):  # past the wrapper's own checks: F = 0 never reaches C through it
        rc = C._lib.lib.bldpc_decode_layered_quant(code._h, ctypes.c_void_p(y.data_ptr()), F, max_iter, ctypes.byref(q), length, C.EXIT_FIXED,
                                                   C.STOP_PREFIX, ctypes.c_void_p(D.data_ptr()), None, ctypes.c_void_p(it.data_ptr()), st)
        return rc, C._lib.lib.bldpc_last_error().decode()

    # two faults at once: the quantiser's parameters are checked first, then F, max_iter, length
    who = "bldpc_decode_layered_quant"
    assert raw(0, 5, bldpc_quant(0.0, 6, 8, 6, 6, 0), 0) == (-1, who + ": llr_scale=0 must be finite and positive")
    assert raw(4, 5, bldpc_quant(16.0, 6, 8, 1, 6, 0), -1) == (-1, who + ": bits_msg=1 outside [2,8]")
    assert raw(0, 5, good.c_struct(), -1) == (-1, who + ": F=0 must be positive")
    assert raw(4, 0, good.c_struct(), -1) == (-1, who + ": max_iter=0 must be at least 1")
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    H, wc, wv = C.Get_H(os.path.join(BL, name), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    yt = torch.ones((table.N, 4), device="cuda")
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*address table") as e:
            C.LDPC_Decoder_Quant_GPU(table, yt, good)
        said.append(str(e.value))
    assert said[0] == said[1]
    with pytest.raises(ValueError):
        C.LDPC_Decoder_Quant_GPU(code, y, good, D=torch.empty((code.N, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        C.LDPC_Decoder_Quant_GPU(code, y, PARAMS["P1"])
    torch.cuda.synchronize()
    _both(C, s, "pair", F_PAIR, "P0", max_iter=FIXED_ITER)  # the code object decodes as before


# ---- the sweep drivers ------------------------------------------------------------------------------------------------------------------
def _counts(D, cwn, it, N, K):
    errs = (D[:K] != cwn[:K]).sum(0)
    ok = D[N] != 0
    return [int(x) for x in (np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok))]


def test_simulation_quant_equals_a_loop_over_the_host_statement(C):
    """Two batches of 64 random codewords over the device channel, per-frame exit on the syndrome: the counters recomputed with
    quant_host on the same channel draws."""
    from cuda_ldpc_amd.simulation import Simulation_GPU
    J, L, Z = 4, 24, 96
    path = os.path.join(BL, "J4_L24_Z96_BlockH.txt")
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    F, maxIT, pn_seed, snr, q = 64, 20, 4242, 2.2, C.Quant(*PARAMS["P1"])
    sigma = C.sigma_of(snr, 1, K / N)
    SIM = C.SimCounters()
    Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, SIM, Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME,
                   max_batches=2, log=None, PN_Message=1, pn_seed=pn_seed, schedule="quant", quant=q, device_channel=True,
                   stop_rule=C.STOP_SYNDROME, leastTestFrames=10 ** 9)
    got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
    seed = np.array([173, 173, 173], np.int32)
    want = np.zeros(5, np.int64)
    for b in range(2):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
        y = C.AWGNChannel_GPU(seed, sigma, N, F, CodeWord=cw)
        r = C.quant_host(H, J, L, Z, y.cpu().numpy(), q, max_iter=maxIT, length=K, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        want += _counts(r["D"], cw.cpu().numpy(), r["iters"], N, K)
    print("quantised P1 at %.1f dB: counters %s" % (snr, got))
    assert SIM.num_Frames == 2 * F and got == want.tolist()
    assert 0 < got[0] < 2 * F and got[2] < maxIT * 2 * F
    for bad in (dict(alpha=0.75), dict(exit_mode=C.EXIT_BATCH_GLOBAL), dict(quant=None), dict(schedule="layered")):
        kw = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=1, log=None, PN_Message=1, schedule="quant", quant=q,
                  device_channel=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, C.SimCounters(), **kw)
    code.close()


def test_simulation_harq_quant_equals_its_host_twin(C):
    """One batch of 256 random codewords, two transmissions: Simulation_HARQ_GPU(schedule="quant") against the loop written out from the
    primitives with quant_host as the decoder (combining in fp32, the decoder quantises the accumulated values)."""
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU
    J, L, Z = 4, 24, 96
    path = os.path.join(BL, "J4_L24_Z96_BlockH.txt")
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    short_llr, q = 1.0e4, C.Quant(*PARAMS["P1"])
    rvs = [C.RateMatch.circular(N, range(0, 24), range(2188, 2260), k0, E) for k0, E in ((0, 2160), (2160, 48))]
    F, pn_seed, maxIT, sigma = 256, 31337, 25, C.sigma_of(2.7)
    SIM, seed, Ds = HarqCounters(), np.array([173, 173, 173], np.int32), []
    Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, Num_Frames_OneTime=F, max_batches=1, log=None, short_llr=short_llr, leastTestFrames=10 ** 9,
                        PN_Message=1, pn_seed=pn_seed, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, schedule="quant", quant=q,
                        stop_rule=C.STOP_SYNDROME, keep_D=Ds)
    got = [SIM.acked, SIM.undetected, SIM.never_acked, SIM.bits_sent, SIM.Total_Iteration]
    seed2 = np.array([173, 173, 173], np.int32)
    cw = C.PN_CodeWords(code, pn_seed, F, first_frame=0, rate_match=rvs[0])
    cwh = cw.cpu().numpy()
    ack = np.zeros(F, bool)
    acked_t, und_t, bits, its = [0, 0], [0, 0], 0, 0
    for t, rm in enumerate(rvs):
        rx = C.AWGNChannel_GPU(seed2, sigma, rm.E, F, CodeWord=C.RM_Select(rm, cw))
        if t == 0:
            y = C.RM_Recover(rm, rx, short_llr)
        else:
            C.RM_Combine(rm, rx, y, torch.from_numpy(ack.astype(np.int32)).cuda(), short_llr)
        torch.cuda.synchronize()
        r = C.quant_host(H, J, L, Z, y.cpu().numpy(), q, max_iter=maxIT, length=K, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
        Dh, it = r["D"], r["iters"].astype(np.int64)
        Dfin = np.where(ack[None, :], Dfin, Dh) if t else Dh
        now = (Dh[N] != 0) & ~ack
        wrong = (Dh[:K] != cwh[:K]).any(0)
        acked_t[t] += int(now.sum())
        und_t[t] += int((now & wrong).sum())
        bits += rm.E * int((~ack).sum())
        its += int(it[~ack].sum())
        ack |= now
    want = [acked_t, und_t, int((~ack).sum()), bits, its]
    print("quantised HARQ sigma %.5f: acked %s undetected %s never %d bits %d iterations %d" % (sigma, *got))
    assert SIM.num_Frames == F and got == want and np.array_equal(seed, seed2)
    assert np.array_equal(Ds[0].cpu().numpy(), Dfin), "D after the last decode: an acknowledged frame keeps the D that acknowledged it"
    assert 0 < got[0][0] < F and got[0][1] > 0, "a sigma at which the first transmission fails for some frames and not for all"
    with pytest.raises(ValueError):
        Simulation_HARQ_GPU(code, seed, sigma, HarqCounters(), rvs, Num_Frames_OneTime=F, max_batches=1, log=None, PN_Message=1, schedule="quant",
                            exit_mode=C.EXIT_PER_FRAME)
    code.close()
