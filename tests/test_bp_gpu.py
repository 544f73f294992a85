"""GPU tests of bldpc_decode_layered_bp: the two kernel tiers against the host statement bldpc_decode_layered_bp_host, bit for bit
on iters, flag row, hard bits and a-posteriori values, on the random block matrices of tests/test_layered_shapes_cpu.py (plus the
one of tests/test_bp_cpu.py, which holds the host statement against the numpy restatement on the same matrices and the same
input), on shipped matrices, with special values, a caller's D on a second stream, scratch that shrinks and grows, several
llr_scale; the other decoders of a code object around a sum-product call; the refusals the device makes; and the counters of
Simulation_GPU / Simulation_HARQ_GPU with schedule="bp" against a loop of the primitives."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from test_bp_cpu import BP_SHAPES, FIXED_ITER, MAX_ITER, SCALE
from test_layered_cpu import special_inputs
from test_layered_shapes_cpu import SEVERAL_FRAMES_PER_WAVE, matrix_of, ramp_input, shape_id

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
# The tier bldpc_decode_layered_bp must pick, by the rule in include/bldpc.h: "k_lbp" when N is a multiple of 64, Z <= 1024 and one
# frame's 4 N + 4 E bytes fit the LDS a workgroup may ask for, "k_lbp_ws" otherwise (test_the_tier_table_follows_the_rule).
TIER = {
    (3, 5, 13): "k_lbp_ws",     # N = 65
    (4, 10, 7): "k_lbp_ws",     # N = 70
    (3, 7, 33): "k_lbp_ws",     # N = 231
    (3, 9, 50): "k_lbp_ws",     # N = 450
    (3, 9, 96): "k_lbp_ws",     # N = 864
    (6, 12, 500): "k_lbp_ws",   # N = 6000, Z = 500: uneven t loop
    (3, 8, 1056): "k_lbp_ws",   # Z above 1024
    (8, 16, 1000): "k_lbp_ws",  # N a multiple of 64, but 62 blocks: 312 000 bytes
    (32, 34, 288): "k_lbp_ws",  # N a multiple of 64, but 356 blocks: 449 280 bytes
    (4, 24, 8): "k_lbp",        # 8 frames in one wave; weights 2 and 23
    (32, 36, 16): "k_lbp",      # 4 frames in one wave, 32 layers
    (4, 10, 640): "k_lbp",      # 640-thread workgroups
    (4, 12, 1024): "k_lbp",     # 1024-thread workgroups, 143 360 bytes
    (3, 8, 1000): "k_lbp",      # Z no multiple of 32: 24 idle lanes in the last wave
    (3, 16, 4): "k_lbp",        # 16 frames in one wave
    (5, 8, 24): "k_lbp",        # frames straddle the wave boundaries
    (5, 12, 32): "k_lbp",       # two frames in one wave
    (5, 12, 96): "k_lbp",
    (3, 8, 1024): "k_lbp",      # 1024 threads
    (2, 27, 64): "k_lbp",       # weights 26 and 25
    (4, 27, 64): "k_lbp",       # weights 26, 2, 3, 25
}
LDS_BYTES = 160 * 1024 - 1024  # the CU's LDS less the kernel's static part (the table and the barrier's words)
ACCEPTED = [s for s in BP_SHAPES if s[:3] in TIER]  # all but the weight-27 matrix, of which no code object is made
BY_DIMS = {s[:3]: s for s in BP_SHAPES}
BATCHES = (1, 37)  # 37 leaves the last workgroup partly filled at 2, 4, 8 and 16 frames per workgroup


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


def _input(s, kind, F):
    """(host array, device tensor) of the shape's input: computed once, shared, never written to."""
    key = (s[:3], kind, F)
    if key not in _inputs:
        N = s[1] * s[2]
        y = ramp_input(N, F) if kind == "ramp" else special_inputs(N, F, np.random.default_rng(7))
        y.setflags(write=False)
        _inputs[key] = (y, torch.from_numpy(y.copy()).cuda())
    return _inputs[key]


def _want(C, s, kind, F, **kw):
    """The host decoder's result: computed once per case, shared among the tests."""
    key = (s[:3], kind, F, tuple(sorted(kw.items())))
    if key not in _host:
        J, L, Z = s[:3]
        _host[key] = C.bp_host(matrix_of(s), J, L, Z, _input(s, kind, F)[0], **kw)
    return _host[key]


def _same(code, r, want, what):
    assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    D = r["D"].cpu().numpy()
    assert np.array_equal(D[code.N], want["D"][code.N]), "flag row: " + what
    assert np.array_equal(D[:code.N], want["D"][:code.N]), "hard bits: " + what
    assert np.array_equal(r["app"].cpu().numpy().view(np.uint32), want["app"].view(np.uint32)), "a-posteriori bits: " + what


def _both(C, s, kind, F, code=None, **kw):
    """The device and the host decoder on the same input: all outputs must carry the same bits."""
    code = code or _code(C, s)
    r = C.LDPC_Decoder_BP_GPU(code, _input(s, kind, F)[1], want_app=True, **kw)
    torch.cuda.synchronize()
    want = _want(C, s, kind, F, **kw)
    _same(code, r, want, "%s %s F=%d %s" % (shape_id(s), kind, F, kw))
    return r, want


def _rules(C, s):
    N, K = s[1] * s[2], (s[1] - s[0]) * s[2]
    return [dict(stop_rule=C.STOP_SYNDROME)] + [dict(stop_rule=C.STOP_PREFIX, length=n) for n in (0, 1, K - 1, N)]


def test_the_tier_table_follows_the_rule():
    assert len(ACCEPTED) == len(TIER) == len(BP_SHAPES) - 1
    for s in ACCEPTED:
        J, L, Z = s[:3]
        H = matrix_of(s)
        assert (H != -1).sum(1).max() <= 26
        N, E = L * Z, int((H != -1).sum()) * Z
        on_chip = N % 64 == 0 and Z <= 1024 and 4 * N + 4 * E + 8 <= LDS_BYTES
        assert TIER[s[:3]] == ("k_lbp" if on_chip else "k_lbp_ws"), shape_id(s)
    ws = {d for d, t in TIER.items() if t == "k_lbp_ws"}
    assert {d[1] * d[2] for d in ws} >= {65, 70, 231, 450, 864} and {500, 1056} <= {d[2] for d in ws} and (32, 34, 288) in ws
    weights = set(np.concatenate([(matrix_of(BY_DIMS[d]) != -1).sum(1) for d, t in TIER.items() if t == "k_lbp"]).tolist())
    assert {2, 3, 25, 26} <= weights


@pytest.mark.parametrize("s", ACCEPTED, ids=shape_id)
def test_random_shapes_match_host(C, s):
    code = _code(C, s)
    N = code.N
    for F in BATCHES:
        for mode, max_iter in ((C.EXIT_FIXED, FIXED_ITER), (C.EXIT_PER_FRAME, MAX_ITER)):
            for rule in _rules(C, s):
                r, want = _both(C, s, "ramp", F, max_iter=max_iter, llr_scale=SCALE, exit_mode=mode, **rule)
                assert code.last_kernel == TIER[s[:3]], "%s ran %s" % (shape_id(s), code.last_kernel)
                if mode != C.EXIT_PER_FRAME or F == 1 or rule.get("length", 0) not in (0, N):
                    continue
                # conditions on the input, judged by the host statement: frames that stop and frames that never do; where
                # several frames share a wave, lanes of one wave that leave the loop at different times
                it = want["iters"]
                assert (it == max_iter).any() and (it < max_iter).any(), "%s %s: iters %s" % (shape_id(s), rule, it)
                if s[:3] in SEVERAL_FRAMES_PER_WAVE:
                    assert np.unique(it).size >= (2 if s[:3] in ((4, 24, 8), (3, 16, 4)) else 3), "%s %s: iters %s" % (shape_id(s), rule, it)


@pytest.mark.parametrize("dims", [(3, 9, 50), (5, 12, 32), (4, 27, 64)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_special_values_on_every_tier(C, dims):
    """Zeros of both signs, denormals, 2^100 and exact ties on one shape of each tier; on (4, 27, 64) they meet the block rows of
    weight 2 (no box-plus), 3 and 26.  llr_scale <= 1: |llr_scale * y| stays within 2^100."""
    s = BY_DIMS[dims]
    code = _code(C, s)
    if dims == (4, 27, 64):
        assert {2, 3, 26} <= set((matrix_of(s) != -1).sum(1).tolist())
    for scale in (1.0, 0.5):
        _both(C, s, "special", 8, max_iter=5, llr_scale=scale)
    _both(C, s, "special", 8, max_iter=5, llr_scale=1.0, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert code.last_kernel == TIER[dims]


def test_caller_provided_D_on_another_stream(C):
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s)
    kw = dict(max_iter=MAX_ITER, llr_scale=SCALE, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    r0, want = _both(C, s, "ramp", 37, **kw)
    yt = _input(s, "ramp", 37)[1]
    D = torch.full((code.N + 1, 37), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # D is filled and yt uploaded on the current stream
    r = C.LDPC_Decoder_BP_GPU(code, yt, D=D, want_app=True, stream=stream, **kw)
    stream.synchronize()
    assert r["D"] is D
    _same(code, r, want, "D= and stream=")
    assert torch.equal(r["D"], r0["D"]) and torch.equal(r["iters"], r0["iters"])
    assert torch.equal(r["app"].view(torch.int32), r0["app"].view(torch.int32))


@pytest.mark.parametrize("dims", [(3, 9, 96), (5, 12, 32)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_scratch_that_shrinks_and_grows(C, dims):
    """One code object of its own, whose scratch and R workspace are sized by the largest call: 37 frames, then 1, then 37 again."""
    s = BY_DIMS[dims]
    code = _code(C, s, fresh=True)
    kw = dict(max_iter=MAX_ITER, llr_scale=SCALE, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    for F in (37, 1, 37):
        _both(C, s, "ramp", F, code=code, **kw)
        _both(C, s, "ramp", F, code=code, max_iter=FIXED_ITER, llr_scale=SCALE)
    assert code.last_kernel == TIER[dims]
    code.close()


def test_llr_scales(C):
    s = BY_DIMS[(5, 12, 96)]
    outs = []
    for scale in (1.0, 2.0, 7.3964):  # 7.3964 = 2 / 0.52^2
        r, _ = _both(C, s, "ramp", 37, max_iter=FIXED_ITER, llr_scale=scale)
        outs.append(r["app"].clone())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]), "sum-product is not scale-invariant"


def _shipped(C, name, J, L, Z, F, **kw):
    H, _, _ = C.Get_H(os.path.join(BL, name), J, L)
    code = C.BinaryCode.from_blockh(os.path.join(BL, name), J, L, Z)
    y = ramp_input(L * Z, F)
    r = C.LDPC_Decoder_BP_GPU(code, torch.from_numpy(y).cuda(), want_app=True, **kw)
    torch.cuda.synchronize()
    _same(code, r, C.bp_host(H, J, L, Z, y, **kw), "%s %s" % (name, kw))
    return code


def test_shipped_J4_L24_Z96(C):
    for kw in (dict(max_iter=FIXED_ITER, llr_scale=SCALE),
               dict(max_iter=MAX_ITER, llr_scale=SCALE, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)):
        code = _shipped(C, "J4_L24_Z96_BlockH.txt", 4, 24, 96, 37, **kw)
        assert code.last_kernel == "k_lbp"


def test_shipped_J15_L30_Z1280(C):
    code = _shipped(C, "J15_L30_Z1280_BlockH.txt", 15, 30, 1280, 3, max_iter=5, llr_scale=SCALE)
    assert code.last_kernel == "k_lbp_ws"


def _thin(C):
    J, L, Z = 4, 24, 96
    H, _, _ = C.Get_H(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L)
    H = H.copy().reshape(J, L)
    H[2, 1:] = -1
    H[2, 0] = 0  # block row 2: weight 1 (the thin-row matrix of test_layered_shapes_gpu.test_refused_matrices)
    return C.BinaryCode.from_shifts(H.reshape(-1), J, L, Z)


def test_other_decoders_unchanged_around_a_sum_product_call(C):
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s, fresh=True)
    y = _input(s, "ramp", 37)[1]

    def others(c, yy):
        a = C.LDPC_Decoder_GPU(c, yy, max_iter=8, exit_mode=C.EXIT_FIXED, want_app=True)
        out = [a["D"].clone(), a["app"].view(torch.int32).clone()]
        try:
            b = C.LDPC_Decoder_Layered_GPU(c, yy, max_iter=6, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
            out += [b["D"].clone(), b["app"].view(torch.int32).clone(), b["iters"].clone()]
        except C._lib.LdpcError:
            out.append(None)  # the thin-row matrix: refused before and after alike
        torch.cuda.synchronize()
        return out

    def equal(p, q):
        return len(p) == len(q) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(p, q))

    before = others(code, y)
    assert len(before) == 5
    _both(C, s, "ramp", 37, code=code, max_iter=MAX_ITER, llr_scale=SCALE, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert equal(others(code, y), before)
    code.close()
    # and after a refused call
    thin = _thin(C)
    yt = torch.from_numpy(ramp_input(thin.N, 5)).cuda()
    before = others(thin, yt)
    assert before[-1] is None
    said = []
    for _ in range(2):
        with pytest.raises(C._lib.LdpcError, match=r"\(-5\): .*weight 1\b.*") as e:
            C.LDPC_Decoder_BP_GPU(thin, yt, llr_scale=SCALE)
        said.append(str(e.value))
    assert said[0] == said[1]
    assert equal(others(thin, yt), before)
    thin.close()


def test_refusals_on_the_device(C):
    from cuda_ldpc_amd._lib import LdpcError
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s)
    J, L, Z = s[:3]
    y = torch.ones((code.N, 4), device="cuda")
    for kw in (dict(llr_scale=0.0), dict(llr_scale=-1.0), dict(llr_scale=float("nan")), dict(llr_scale=float("inf")), dict(max_iter=0),
               dict(length=code.N + 1), dict(length=-1), dict(stop_rule=3), dict(exit_mode=C.EXIT_BATCH_GLOBAL), dict(exit_mode=9)):
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(-1\): .*\S") as e:
                C.LDPC_Decoder_BP_GPU(code, y, **kw)
            said.append(str(e.value))
        assert said[0] == said[1], kw
    import ctypes
    D = torch.empty((code.N + 1, 4), dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = C._lib.lib.bldpc_decode_layered_bp(code._h, ctypes.c_void_p(y.data_ptr()), 4, 5, ctypes.c_float(1.0), 0, C.EXIT_PER_FRAME, C.STOP_PREFIX,
                                            ctypes.c_void_p(D.data_ptr()), None, None, st)
    assert rc == -1 and b"iters" in C._lib.lib.bldpc_last_error()
    it = torch.empty(4, dtype=torch.int32, device="cuda")

    def raw(F, max_iter, llr_scale, length):  # past the wrapper's own checks: F = 0 never reaches C through it
        rc = C._lib.lib.bldpc_decode_layered_bp(code._h, ctypes.c_void_p(y.data_ptr()), F, max_iter, ctypes.c_float(llr_scale), length, C.EXIT_FIXED,
                                                C.STOP_PREFIX, ctypes.c_void_p(D.data_ptr()), None, ctypes.c_void_p(it.data_ptr()), st)
        return rc, C._lib.lib.bldpc_last_error().decode()

    # two faults at once: the first one in the order of the checks is the one reported (F, max_iter, llr_scale, length)
    who = "bldpc_decode_layered_bp"
    assert raw(0, 5, 0.0, 0) == (-1, who + ": F=0 must be positive")
    assert raw(4, 5, 0.0, -1) == (-1, who + ": llr_scale=0 must be finite and positive")
    assert raw(4, 0, 0.0, -1) == (-1, who + ": max_iter=0 must be at least 1")
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    H, wc, wv = C.Get_H(os.path.join(BL, name), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    yt = torch.ones((table.N, 4), device="cuda")
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*address table") as e:
            C.LDPC_Decoder_BP_GPU(table, yt)
        said.append(str(e.value))
    assert said[0] == said[1]
    with pytest.raises(ValueError):
        C.LDPC_Decoder_BP_GPU(code, y, D=torch.empty((code.N, 4), dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    _both(C, s, "ramp", 37, max_iter=FIXED_ITER, llr_scale=SCALE)  # the code object decodes as before


# ---- the sweep drivers ------------------------------------------------------------------------------------------------------------------
def test_simulation_bp_pn_message_counters(C):
    """One batch of 256 random codewords over the device channel, per-frame exit on the syndrome: the counters recomputed from
    LDPC_Decoder_BP_GPU + Syndrome on the same channel draws."""
    from cuda_ldpc_amd.simulation import Simulation_GPU
    J, L, Z = 4, 24, 96
    code = C.BinaryCode.from_blockh(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L, Z)
    F, maxIT, pn_seed, snr = 256, 20, 4242, 2.4
    sigma = C.sigma_of(snr, 1, code.K / code.N)
    SIM = C.SimCounters()
    Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, SIM, Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME,
                   max_batches=1, log=None, PN_Message=1, pn_seed=pn_seed, schedule="bp", device_channel=True, stop_rule=C.STOP_SYNDROME)
    got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
    cw = C.PN_CodeWords(code, pn_seed, F, first_frame=0)
    y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code.N, F, CodeWord=cw)
    r = C.LDPC_Decoder_BP_GPU(code, y, max_iter=maxIT, llr_scale=2.0 / (sigma * sigma), length=code.K, exit_mode=C.EXIT_PER_FRAME,
                              stop_rule=C.STOP_SYNDROME)
    flag = r["D"][code.N].clone()
    syn = C.Syndrome(code, r["D"].clone(), into_flag_row=False)
    torch.cuda.synchronize()
    assert torch.equal(flag, syn["flag"]), "the flag row is the syndrome check"
    D, cwn, it = r["D"].cpu().numpy(), cw.cpu().numpy(), r["iters"].cpu().numpy()
    errs = (D[:code.K] != cwn[:code.K]).sum(0)
    ok = syn["flag"].cpu().numpy() != 0
    want = [np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)]
    assert SIM.num_Frames == F and got == [int(x) for x in want]
    assert 0 < got[0] < F and got[2] < maxIT * F
    for bad in (dict(alpha=0.75), dict(exit_mode=C.EXIT_BATCH_GLOBAL)):
        kw = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=1, log=None, PN_Message=1, schedule="bp",
                  device_channel=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, C.SimCounters(), **kw)
    code.close()


def test_simulation_bp_over_qam_and_rate_matched(C):
    """llr_scale on the other two paths of Simulation_GPU(schedule="bp"): 1.0 after the 64-QAM demapper (scale 1 / (2 sigma^2)), and
    2 / sigma^2 on the rate-matched BPSK channel.  One batch of 256 frames each, against the primitives."""
    from cuda_ldpc_amd import nbldpc as nb
    from cuda_ldpc_amd.simulation import Simulation_GPU
    J, L, Z = 4, 24, 96
    code = C.BinaryCode.from_blockh(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L, Z)
    N, K, F, maxIT, pn_seed, q, m = code.N, code.K, 256, 25, 31337, 64, 6
    kw = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=1, log=None, PN_Message=1, pn_seed=pn_seed, schedule="bp",
              device_channel=True, leastTestFrames=10 ** 9)

    def counters(SIM):
        return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]

    def count(r, cw):
        D, cwn, it = r["D"].cpu().numpy(), cw.cpu().numpy(), r["iters"].cpu().numpy()
        errs = (D[:K] != cwn[:K]).sum(0)
        ok = D[N] != 0
        return [int(x) for x in (np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok))]

    con = C.Get_CONSTELLATION(os.path.join(DATA, "nb", "Constellation", "GRAY_64QAM.txt"), q)
    cond = torch.from_numpy(con).cuda()
    sigma = nb.sigma_of(10.0, K / N, 0, q)  # Eb/N0 10 dB: the middle of the waterfall of this code over 64-QAM (tests/test_modem_gpu.py)
    SIM = C.SimCounters()
    Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, SIM, n_QAM=q, CONSTELLATION=con, **kw)
    cw = C.PN_CodeWords(code, pn_seed, F, first_frame=0)
    rx = C.AWGNChannel_QAM_GPU(np.array([173, 173, 173], np.int32), sigma, C.Modulate_QAM(cw, N, m), cond)
    y = C.Demodulate_QAM(rx, cond, 1.0 / (2.0 * sigma * sigma), N)
    want = count(C.LDPC_Decoder_BP_GPU(code, y, max_iter=maxIT, llr_scale=1.0, length=K, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME), cw)
    print("sum-product over 64-QAM, sigma %.5f: counters %s" % (sigma, counters(SIM)))
    assert counters(SIM) == want and 0 < want[0] < F

    rm = C.RateMatch(N, range(0, 24), range(2188, 2260))
    sigma = C.sigma_of(2.7)
    SIM = C.SimCounters()
    Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, SIM, rate_match=rm, short_llr=1.0e4, **kw)
    cw = C.PN_CodeWords(code, pn_seed, F, first_frame=0, rate_match=rm)
    y = C.RM_Recover(rm, C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, rm.E, F, CodeWord=C.RM_Select(rm, cw)), 1.0e4)
    want = count(C.LDPC_Decoder_BP_GPU(code, y, max_iter=maxIT, llr_scale=2.0 / (sigma * sigma), length=K, exit_mode=C.EXIT_PER_FRAME,
                                       stop_rule=C.STOP_SYNDROME), cw)
    print("sum-product, rate-matched BPSK, sigma %.5f: counters %s" % (sigma, counters(SIM)))
    assert counters(SIM) == want and 0 < want[0] < F
    code.close()


def test_simulation_harq_bp_counters(C):
    """One batch of 256 random codewords, two transmissions: the counters of Simulation_HARQ_GPU(schedule="bp") against the loop
    written out from the primitives, the whole batch decoded again after the second transmission."""
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU
    J, L, Z = 4, 24, 96
    code = C.BinaryCode.from_blockh(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L, Z)
    N, K = code.N, code.K
    short_llr = 1.0e4
    rvs = [C.RateMatch.circular(N, range(0, 24), range(2188, 2260), k0, E) for k0, E in ((0, 2160), (2160, 48))]
    F, pn_seed, maxIT, sigma = 256, 31337, 25, C.sigma_of(2.7)
    SIM, seed, Ds = HarqCounters(), np.array([173, 173, 173], np.int32), []
    Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, Num_Frames_OneTime=F, max_batches=1, log=None, short_llr=short_llr, leastTestFrames=10 ** 9,
                        PN_Message=1, pn_seed=pn_seed, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, schedule="bp", stop_rule=C.STOP_SYNDROME, keep_D=Ds)
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
        r = C.LDPC_Decoder_BP_GPU(code, y, max_iter=maxIT, llr_scale=2.0 / (sigma * sigma), length=K, exit_mode=C.EXIT_PER_FRAME,
                                  stop_rule=C.STOP_SYNDROME)
        syn = C.Syndrome(code, r["D"].clone(), into_flag_row=False)
        torch.cuda.synchronize()
        assert torch.equal(r["D"][N], syn["flag"])
        Dh, it = r["D"].cpu().numpy(), r["iters"].cpu().numpy().astype(np.int64)
        now = (Dh[N] != 0) & ~ack
        wrong = (Dh[:K] != cwh[:K]).any(0)
        acked_t[t] += int(now.sum())
        und_t[t] += int((now & wrong).sum())
        bits += rm.E * int((~ack).sum())
        its += int(it[~ack].sum())
        ack |= now
    want = [acked_t, und_t, int((~ack).sum()), bits, its]
    print("sum-product HARQ sigma %.5f: acked %s undetected %s never %d bits %d iterations %d" % (sigma, *got))
    assert SIM.num_Frames == F and got == want and np.array_equal(seed, seed2)
    assert np.array_equal(Ds[0].cpu().numpy(), Dh), "D after the last decode"
    assert 0 < got[0][0] < F and got[0][1] > 0, "a sigma at which the first transmission fails for some frames and not for all"
    with pytest.raises(ValueError):
        Simulation_HARQ_GPU(code, seed, sigma, HarqCounters(), rvs, Num_Frames_OneTime=F, max_batches=1, log=None, PN_Message=1, schedule="bp",
                            exit_mode=C.EXIT_PER_FRAME, alpha=0.75)
    code.close()
