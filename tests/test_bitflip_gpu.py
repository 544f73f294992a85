"""GPU tests of hard-decision decoding (include/bldpc.h): the kernel k_bf against the host statement bldpc_decode_bitflip_host, exactly,
on iters, flag row, D and Dbits, on the matrices, batch sizes and inputs of tests/bitflip_cases.py (tests/test_bitflip_cpu.py holds the
host statement against the numpy restatement on the same cases and checks that the inputs meet their condition); garbage in the input
padding, a caller's D on a second stream, guard words around Dbits, one output only, scratch that shrinks and grows, the other decoders
of a code object around a bit-flip call, the refusals the device makes; the channel, pack and unpack kernels against their host
statements; shipped codes; and the two drivers against loops written out from the primitives."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bitflip_cases import (BATCHES, BF_GRADIENT, BF_THRESHOLD, EXIT_BATCH_GLOBAL, EXIT_FIXED, EXIT_PER_FRAME, F_MAX, MAX_ITER, RULES, accepted_dims,
                           bound_shapes, dims_id, garbage_padding, matrix, np_pack, np_unpack, ramp_input)
from conftest import DATA
from test_bitflip_cpu import special_values
from test_quant_gpu import _counts

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes, _host = {}, {}


def _code(C, dims, fresh=False):
    J, L, Z = dims
    if fresh:
        return C.BinaryCode.from_shifts(matrix(dims), J, L, Z)
    if dims not in _codes:
        _codes[dims] = C.BinaryCode.from_shifts(matrix(dims), J, L, Z)
    return _codes[dims]


def _bits(dims, F, dirty=False):
    b = np_pack(ramp_input(dims)[0][:, :F])
    return garbage_padding(b, F) if dirty else b


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32).copy()).cuda()


def _want(C, dims, F, rule, mode):
    """The host statement's result on the clean words: computed once per case, shared among the tests."""
    key = (dims, F, rule, mode)
    if key not in _host:
        J, L, Z = dims
        _host[key] = C.bitflip_host(matrix(dims), J, L, Z, _bits(dims, F), F, rule=rule, max_iter=MAX_ITER, exit_mode=mode)
    return _host[key]


def _same(r, want, what):
    assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    if r["D"] is not None:
        D = r["D"].cpu().numpy()
        assert np.array_equal(D[-1], want["D"][-1]), "flag row: " + what
        assert np.array_equal(D, want["D"]), "hard bits: " + what
    if r["Dbits"] is not None:
        assert np.array_equal(r["Dbits"].cpu().numpy().view(np.uint32), want["Dbits"]), "Dbits: " + what


def _both(C, dims, F, rule, mode, code=None, dirty=False, **kw):
    code = code or _code(C, dims)
    r = C.LDPC_Decoder_BitFlip_GPU(code, _dev(_bits(dims, F, dirty)), F, rule=rule, max_iter=MAX_ITER, exit_mode=mode, want_bits=True, **kw)
    torch.cuda.synchronize()
    assert code.last_kernel == "k_bf"
    want = _want(C, dims, F, rule, mode)
    _same(r, want, "%s F=%d rule %d mode %d" % (dims_id(dims), F, rule, mode))
    return r, want


@pytest.mark.parametrize("dims", accepted_dims(), ids=dims_id)
def test_every_shape_matches_the_host_statement(C, dims):
    for F in BATCHES:
        for rule in RULES:
            for mode in (EXIT_FIXED, EXIT_PER_FRAME):
                _both(C, dims, F, rule, mode)
    info = _code(C, dims).bitflip_info()
    assert info == C.bitflip_plan_host(matrix(dims), *dims) and info["fits"]


@pytest.mark.parametrize("dims", [(3, 5, 13), (3, 9, 96), (4, 27, 64)], ids=dims_id)
def test_garbage_in_the_input_padding(C, dims):
    for F in (1, 33, 37):
        for rule in RULES:
            _both(C, dims, F, rule, EXIT_PER_FRAME, dirty=True)


def test_caller_provided_D_on_another_stream(C):
    dims = (3, 9, 96)
    code = _code(C, dims)
    r0, want = _both(C, dims, 37, BF_GRADIENT, EXIT_PER_FRAME)
    bits = _dev(_bits(dims, 37))
    D = torch.full((code.N + 1, 37), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # D is filled and the words uploaded on the current stream
    r = C.LDPC_Decoder_BitFlip_GPU(code, bits, 37, rule=BF_GRADIENT, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME, D=D, stream=stream)
    stream.synchronize()
    assert r["D"] is D and r["Dbits"] is None
    _same(r, want, "D= and stream=")
    assert torch.equal(r["D"], r0["D"]) and torch.equal(r["iters"], r0["iters"])


def test_guard_words_around_Dbits_and_one_output_only(C):
    """The C entry point with Dbits inside a guarded buffer; Dbits only (no D is touched) and D only."""
    dims = (3, 7, 33)
    code = _code(C, dims)
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for F in (33, 37):
        W = (F + 31) // 32
        n = (code.N + 1) * W
        bits = _dev(_bits(dims, F, dirty=True))
        for rule in RULES:
            want = _want(C, dims, F, rule, EXIT_PER_FRAME)
            buf = torch.full((n + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            it = torch.full((F + 8,), -3, dtype=torch.int32, device="cuda")
            rc = lib.bldpc_decode_bitflip(code._h, ptr(bits), F, MAX_ITER, rule, EXIT_PER_FRAME, None, ptr(buf[32:]), ptr(it[4:]), st)
            torch.cuda.synchronize()
            assert rc == 0 and code.last_kernel == "k_bf"
            b = buf.cpu().numpy()
            assert (b[:32] == 0x5A5A5A5A).all() and (b[32 + n:] == 0x5A5A5A5A).all(), "a store outside Dbits"
            assert np.array_equal(b[32:32 + n].view(np.uint32).reshape(code.N + 1, W), want["Dbits"])
            i = it.cpu().numpy()
            assert (i[:4] == -3).all() and (i[4 + F:] == -3).all() and np.array_equal(i[4:4 + F], want["iters"])
            r = C.LDPC_Decoder_BitFlip_GPU(code, bits, F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME, want_bits=True, want_D=False)
            assert r["D"] is None
            _same(r, want, "Dbits only")
            r = C.LDPC_Decoder_BitFlip_GPU(code, bits, F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)
            assert r["Dbits"] is None
            _same(r, want, "D only")


def test_scratch_that_shrinks_and_grows(C):
    dims = (3, 9, 96)
    code = _code(C, dims, fresh=True)
    for F in (37, 1, 37):
        for rule in RULES:
            r = C.LDPC_Decoder_BitFlip_GPU(code, _dev(_bits(dims, F)), F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)  # D only: the plan's words
            torch.cuda.synchronize()
            _same(r, _want(C, dims, F, rule, EXIT_PER_FRAME), "F=%d" % F)
    assert code.last_kernel == "k_bf"
    code.close()


def _others(C, c, yy):
    a = C.LDPC_Decoder_GPU(c, yy, max_iter=8, exit_mode=C.EXIT_FIXED, want_app=True)
    out = [a["D"].clone(), a["app"].view(torch.int32).clone()]
    b = C.LDPC_Decoder_Layered_GPU(c, yy, max_iter=6, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
    out += [b["D"].clone(), b["app"].view(torch.int32).clone(), b["iters"].clone()]
    b = C.LDPC_Decoder_BP_GPU(c, yy, max_iter=6, llr_scale=2.0, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
    out += [b["D"].clone(), b["app"].view(torch.int32).clone(), b["iters"].clone()]
    b = C.LDPC_Decoder_Quant_GPU(c, yy, C.Quant(), max_iter=6, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME, want_app=True)
    out += [b["D"].clone(), b["app"].clone(), b["iters"].clone()]
    torch.cuda.synchronize()
    return out


def test_other_decoders_unchanged_around_a_bitflip_call(C):
    dims = (3, 9, 96)
    code = _code(C, dims, fresh=True)
    y = torch.from_numpy((1.0 - 2.0 * ramp_input(dims)[0][:, :37]).astype(np.float32)).cuda()
    before = _others(C, code, y)
    assert len(before) == 11
    _both(C, dims, 37, BF_GRADIENT, EXIT_PER_FRAME, code=code)
    _both(C, dims, 37, BF_THRESHOLD, EXIT_FIXED, code=code)
    after = _others(C, code, y)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    code.close()
    # and after a refused call
    beyond = bound_shapes()[1]
    big = _code(C, beyond, fresh=True)
    yb = torch.ones((big.N, 3), device="cuda")
    before = _others(C, big, yb)
    with pytest.raises(C._lib.LdpcError, match=r"\(-5\): .*LDS"):
        C.LDPC_Decoder_BitFlip_GPU(big, torch.zeros((big.N, 1), dtype=torch.int32, device="cuda"), 3)
    after = _others(C, big, yb)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    big.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_the_shape_beyond_the_bound_is_refused_and_nothing_is_launched(C):
    from cuda_ldpc_amd._lib import LdpcError
    beyond = bound_shapes()[1]
    code = _code(C, beyond, fresh=True)
    assert not code.bitflip_info()["fits"]
    F = 3
    bits = torch.zeros((code.N, 1), dtype=torch.int32, device="cuda")
    D = torch.full((code.N + 1, F), -7, dtype=torch.int32, device="cuda")
    before = code.last_kernel
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*LDS") as e:
            C.LDPC_Decoder_BitFlip_GPU(code, bits, F, D=D)
        said.append(str(e.value))
    torch.cuda.synchronize()
    assert said[0] == said[1] and code.last_kernel == before
    assert bool((D == -7).all()), "the outputs of a refused call are untouched"
    code.close()


def test_refusals_on_the_device(C):
    from cuda_ldpc_amd._lib import LdpcError
    dims = (3, 9, 96)
    code = _code(C, dims)
    F = 4
    bits = torch.zeros((code.N, 1), dtype=torch.int32, device="cuda")
    for kw in (dict(rule=2), dict(rule=-1), dict(max_iter=0), dict(exit_mode=EXIT_BATCH_GLOBAL), dict(exit_mode=9)):
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(-1\): .*\S") as e:
                C.LDPC_Decoder_BitFlip_GPU(code, bits, F, **kw)
            said.append(str(e.value))
        assert said[0] == said[1], kw
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")
    it = torch.empty(F, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(F=F, bits=bits, D=D, Db=None, it=it, mode=EXIT_FIXED):
        rc = lib.bldpc_decode_bitflip(code._h, ptr(bits), F, 5, BF_GRADIENT, mode, ptr(D), ptr(Db), ptr(it), st)
        return rc, lib.bldpc_last_error().decode()

    who = "bldpc_decode_bitflip"
    assert raw(F=0) == (-1, who + ": F=0 must be positive")
    assert raw(bits=None) == (-1, who + ": null bits_in")
    assert raw(D=None) == (-1, who + ": D and Dbits are both null")
    assert raw(it=None, mode=EXIT_PER_FRAME) == (-1, who + ": per-frame exit needs iters")
    assert raw(it=None)[0] == 0  # iters is optional in fixed mode
    assert lib.bldpc_decode_bitflip(None, ptr(bits), F, 5, 0, 0, ptr(D), None, ptr(it), st) == -1
    for bad in (dict(F=0), dict(F=40), dict(D=torch.empty((code.N, F), dtype=torch.int32, device="cuda")), dict(want_D=False)):
        with pytest.raises(ValueError):
            C.LDPC_Decoder_BitFlip_GPU(code, bits, **dict(dict(F=F), **bad))
    with pytest.raises(ValueError):
        C.LDPC_Decoder_BitFlip_GPU(code, bits.cpu(), F)
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    H, wc, wv = C.Get_H(os.path.join(BL, name), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*address table") as e:
            C.LDPC_Decoder_BitFlip_GPU(table, torch.zeros((table.N, 1), dtype=torch.int32, device="cuda"), F)
        said.append(str(e.value))
    assert said[0] == said[1]
    with pytest.raises(LdpcError, match=r"\(-5\): .*address table"):
        table.bitflip_info()
    for p in (-0.1, 0.6, float("nan")):
        with pytest.raises(ValueError):
            C.BSCChannel_GPU(np.array([1, 2, 3], np.int32), p, 8, 4)
    with pytest.raises(LdpcError, match=r"\(-1\): .*seed"):
        C.BSCChannel_GPU(np.array([1, 2, 63599], np.int32), 0.1, 8, 4)
    torch.cuda.synchronize()
    _both(C, dims, 37, BF_GRADIENT, EXIT_FIXED)  # the code object decodes as before


# ---- channel, pack, unpack --------------------------------------------------------------------------------------------------------------
def test_bsc_kernel_equals_the_host_channel(C):
    """N = 77 is no multiple of the run of rows a thread walks; F = 37 and 300 leave partly filled words, waves and workgroups; the
    second call starts from the advanced seed."""
    N = 77
    for F in (37, 300):
        cw = torch.from_numpy(np.random.default_rng(F).integers(0, 2, size=(N, F)).astype(np.int32)).cuda()
        for word in (None, cw):
            sd, sh = np.array([173, 173, 173], np.int32), np.array([173, 173, 173], np.int32)
            for call in range(2):
                got = C.BSCChannel_GPU(sd, 0.11, N, F, CodeWord=word)
                want = C.BSCChannel_CPU(sh, 0.11, N, F, CodeWord=None if word is None else word.cpu().numpy())
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), want), (F, call)
                assert np.array_equal(sd, sh)
            assert 0 < np_unpack(want, F).sum()


def test_pack_and_unpack_kernels(C):
    y, _ = special_values()
    y = np.ascontiguousarray(np.tile(y, (3, 7))[:, :77])  # [6, 77]: a partly filled third word
    got = C.Hard_Pack(torch.from_numpy(y).cuda())
    assert np.array_equal(got.cpu().numpy().view(np.uint32), C.Hard_Pack_host(y))
    rng = np.random.default_rng(12)
    for rows, F in ((1, 1), (5, 37), (3, 64), (9, 300)):
        b = rng.integers(0, 2, size=(rows, F)).astype(np.int32)
        bt = torch.from_numpy(b * 3).cuda()
        words = C.Hard_Pack_Int(bt)
        assert np.array_equal(words.cpu().numpy().view(np.uint32), C.Hard_Pack_Int_host(b)) and np.array_equal(C.Hard_Pack_Int_host(b), np_pack(b))
        back = C.Hard_Unpack(words, F)
        assert back.dtype == torch.int32 and np.array_equal(back.cpu().numpy(), b), "unpack of pack is the identity"
        yy = torch.from_numpy(np.where(b, -0.5, 0.5).astype(np.float32)).cuda()
        assert torch.equal(C.Hard_Pack(yy), words)
        dirty = torch.from_numpy(garbage_padding(np_pack(b), F).view(np.int32)).cuda()
        assert np.array_equal(C.Hard_Unpack(dirty, F).cpu().numpy(), b)


# ---- shipped codes ----------------------------------------------------------------------------------------------------------------------
def _shipped(C, name, J, L, Z, F, p, **kw):
    path = os.path.join(BL, name)
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    bits = C.BSCChannel_GPU(np.array([173, 173, 173], np.int32), p, L * Z, F)
    r = C.LDPC_Decoder_BitFlip_GPU(code, bits, F, want_bits=True, **kw)
    torch.cuda.synchronize()
    want = C.bitflip_host(H, J, L, Z, bits.cpu().numpy().view(np.uint32), F, **kw)
    _same(r, want, "%s %s" % (name, kw))
    assert code.last_kernel == "k_bf"
    return code, want


@pytest.mark.parametrize("name,J,L,Z,p", [("J4_L24_Z96_BlockH.txt", 4, 24, 96, 0.004), ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 0.02)])
def test_shipped_codes(C, name, J, L, Z, p):
    for rule in RULES:
        code, want = _shipped(C, name, J, L, Z, 64, p, rule=rule, max_iter=30, exit_mode=EXIT_PER_FRAME)
        print("%s p=%g rule %d: iters %s" % (name, p, rule, np.unique(want["iters"]).tolist()))
        assert np.unique(want["iters"]).size >= 3
        code.close()


def test_shipped_PON(C):
    for rule in RULES:
        code, _ = _shipped(C, "PON_LDPC.txt", 12, 69, 256, 3, 0.003, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)
        assert code.bitflip_info()["fits"]
        code.close()


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------
def test_simulation_bsc_equals_a_loop_over_the_host_statement(C):
    """Two batches of 64 random codewords: the counters of Simulation_BSC_GPU recomputed with bitflip_host on the same channel draws."""
    from cuda_ldpc_amd.simulation import Simulation_BSC_GPU
    J, L, Z = 4, 24, 96
    path = os.path.join(BL, "J4_L24_Z96_BlockH.txt")
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    F, maxIT, pn_seed, p = 64, 30, 4242, 0.006
    for rule in RULES:
        SIM, seed = C.SimCounters(), np.array([173, 173, 173], np.int32)
        Simulation_BSC_GPU(code, seed, p, SIM, rule=rule, Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=EXIT_PER_FRAME, PN_Message=1, pn_seed=pn_seed,
                           max_batches=2, leastTestFrames=10 ** 9, log=None)
        got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
        seed2, want = np.array([173, 173, 173], np.int32), np.zeros(5, np.int64)
        for b in range(2):
            cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
            bits = C.BSCChannel_GPU(seed2, p, N, F, CodeWord=cw)
            r = C.bitflip_host(H, J, L, Z, bits.cpu().numpy().view(np.uint32), F, rule=rule, max_iter=maxIT, exit_mode=EXIT_PER_FRAME)
            want += _counts(r["D"], cw.cpu().numpy(), r["iters"], N, K)
        print("bit flipping rule %d at p=%g: counters %s" % (rule, p, got))
        assert SIM.num_Frames == 2 * F and got == want.tolist() and np.array_equal(seed, seed2)
        assert 0 < got[0] < 2 * F and got[2] < maxIT * 2 * F
    for bad in (dict(rule=2), dict(exit_mode=EXIT_BATCH_GLOBAL), dict(PN_Message=2)):
        with pytest.raises(ValueError):
            Simulation_BSC_GPU(code, np.array([173, 173, 173], np.int32), p, C.SimCounters(), max_batches=1, log=None, **bad)
    with pytest.raises(ValueError):
        Simulation_BSC_GPU(code, np.array([173, 173, 173], np.int32), 0.7, C.SimCounters(), max_batches=1, log=None)
    code.close()


def test_simulation_hard_schedule_equals_a_loop_over_the_host_statement(C):
    """Simulation_GPU(schedule="hard") over the device AWGN channel against Hard_Pack_host on the channel output and bitflip_host."""
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_GPU, Simulation_HARQ_GPU
    J, L, Z = 4, 24, 96
    path = os.path.join(BL, "J4_L24_Z96_BlockH.txt")
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    F, maxIT, pn_seed, snr = 64, 30, 99, 5.2
    sigma = C.sigma_of(snr, 1, K / N)
    base = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=EXIT_PER_FRAME, max_batches=2, log=None, PN_Message=1, pn_seed=pn_seed, schedule="hard",
                device_channel=True, leastTestFrames=10 ** 9)
    for rule in RULES:
        SIM, seed = C.SimCounters(), np.array([173, 173, 173], np.int32)
        Simulation_GPU(code, seed, sigma, SIM, hard_rule=rule, **base)
        got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
        seed2, want = np.array([173, 173, 173], np.int32), np.zeros(5, np.int64)
        for b in range(2):
            cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
            y = C.AWGNChannel_GPU(seed2, sigma, N, F, CodeWord=cw)
            r = C.bitflip_host(H, J, L, Z, C.Hard_Pack_host(y.cpu().numpy()), F, rule=rule, max_iter=maxIT, exit_mode=EXIT_PER_FRAME)
            want += _counts(r["D"], cw.cpu().numpy(), r["iters"], N, K)
        print("hard schedule rule %d at %.1f dB: counters %s" % (rule, snr, got))
        assert SIM.num_Frames == 2 * F and got == want.tolist() and np.array_equal(seed, seed2)
        assert 0 < got[0] < 2 * F
    rm = C.RateMatch(N, [], range(N - 8, N))
    for bad in (dict(rate_match=rm), dict(alpha=0.75), dict(quant=C.Quant()), dict(stop_rule=C.STOP_SYNDROME), dict(hard_rule=5),
                dict(exit_mode=EXIT_BATCH_GLOBAL), dict(schedule="layered", hard_rule=BF_GRADIENT)):
        with pytest.raises(ValueError):
            Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, C.SimCounters(), **dict(base, **bad))
    with pytest.raises(ValueError, match="hard"):
        Simulation_HARQ_GPU(code, np.array([173, 173, 173], np.int32), sigma, HarqCounters(), [rm], Num_Frames_OneTime=F, max_batches=1, log=None,
                            schedule="hard")
    code.close()
