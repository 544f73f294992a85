"""GPU tests of erasure decoding by elimination (include/bldpc.h): the kernels k_er_ml and k_er_ml_ws against the host statement
bldpc_decode_erasure_ml_host, exactly, on Dbits, Ebits, D, status and rank, on the shapes, batch sizes, inputs and max_erased values of
tests/erasure_ml_cases.py (tests/test_erasure_ml_cpu.py holds the host statement against the restatement on the same cases and asserts
the case table), every tier the case admits; garbage in the padding and under the erasures, each output alone, guard words, a caller's
stream, scratch that grows and is reused, an empty and a full frame list, more listed frames than workspace slots, the other decoders
of a code object around an accepted and a refused call, the refusals the device makes; a shipped code around its cliff; and
Simulation_BEC_GPU with and without elimination against loops written out from the host statements, whole and in shards."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from erasure_ml_cases import (ALL_ERASED, BATCHES, DIMS, EXTREME, ML_NONE, ML_SKIPPED, ML_SOLVED, WORKSPACE_DIMS, dims_id, matrix, max_erased_values,
                              ml_dirty_input, ml_input, np_pack, np_unpack)

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
KERNEL = {"lds": "k_er_ml", "workspace": "k_er_ml_ws"}


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


def _words(dims, F, dirty=False):
    if dirty:
        return ml_dirty_input(dims, F)
    bits, er, _ = ml_input(dims)
    return np_pack(bits[:, :F]), np_pack(er[:, :F])


def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _want(C, dims, F, me):
    """The host statement's result on the clean words: computed once per case, shared among the tests."""
    key = (dims, F, me)
    if key not in _host:
        J, L, Z = dims
        _host[key] = C.erasure_ml_host(matrix(dims), J, L, Z, *_words(dims, F), F, max_erased=me)
    return _host[key]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(r, want, what):
    assert np.array_equal(r["status"].cpu().numpy(), want["status"]), "status: " + what
    assert np.array_equal(r["rank"].cpu().numpy(), want["rank"]), "rank: " + what
    if r["Dbits"] is not None:
        assert np.array_equal(_u32(r["Dbits"])[-1], want["Dbits"][-1]), "flag words: " + what
        assert np.array_equal(_u32(r["Dbits"]), want["Dbits"]), "Dbits: " + what
    if r["Ebits"] is not None:
        assert np.array_equal(_u32(r["Ebits"]), want["Ebits"]), "Ebits: " + what
    if r["D"] is not None:
        assert np.array_equal(r["D"].cpu().numpy(), want["D"]), "D: " + what


def _tiers(C, dims, me):
    """The tiers to force at this max_erased, and the one AUTO takes."""
    auto = C.erasure_ml_plan_host(matrix(dims), *dims, max_erased=me)["tier"]
    return (["lds"] if auto == "lds" else []) + ["workspace"], auto


def _both(C, dims, F, me, tier="auto", code=None, dirty=False, **kw):
    code = code or _code(C, dims)
    b, e = _words(dims, F, dirty)
    r = C.LDPC_Decoder_Erasure_ML_GPU(code, _dev(b), _dev(e), F, max_erased=me, tier=tier, **dict(dict(want_D=True), **kw))
    torch.cuda.synchronize()
    assert code.last_kernel == KERNEL[_tiers(C, dims, me)[1] if tier == "auto" else tier]
    want = _want(C, dims, F, me)
    _same(r, want, "%s F=%d max_erased=%d tier=%s" % (dims_id(dims), F, me, tier))
    return r, want


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_every_shape_matches_the_host_statement(C, dims):
    for me in max_erased_values(dims):
        forced, auto = _tiers(C, dims, me)
        for F in BATCHES:
            for tier in forced + ["auto"]:
                _both(C, dims, F, me, tier)
        info = _code(C, dims).erasure_ml_info(max_erased=me)
        assert info == C.erasure_ml_plan_host(matrix(dims), *dims, max_erased=me) and info["tier"] == auto
    assert _tiers(C, dims, 0)[1] == ("workspace" if dims == WORKSPACE_DIMS else "lds")


@pytest.mark.parametrize("dims", [(3, 5, 13), (3, 9, 96), EXTREME], ids=dims_id)
def test_garbage_in_the_padding_and_under_the_erasures(C, dims):
    for F in (1, 33, 37):
        for tier in ("lds", "workspace"):
            r, _ = _both(C, dims, F, dims[1] * dims[2], tier, dirty=True)
            for k in ("Dbits", "Ebits"):
                assert (_u32(r[k])[:, -1] >> np.uint32(F % 32)).max() == 0, "output padding: " + k


def test_caller_provided_D_on_another_stream(C):
    dims = (3, 9, 96)
    code = _code(C, dims)
    r0, want = _both(C, dims, 37, 0)
    b, e = (_dev(a) for a in _words(dims, 37))
    D = torch.full((code.N + 1, 37), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # D is filled and the words uploaded on the current stream
    r = C.LDPC_Decoder_Erasure_ML_GPU(code, b, e, 37, D=D, want_bits=False, want_erased=False, stream=stream)
    stream.synchronize()
    assert r["D"] is D and r["Dbits"] is None and r["Ebits"] is None
    _same(r, want, "D= and stream=")
    assert torch.equal(r["D"], r0["D"]) and torch.equal(r["status"], r0["status"])


def test_guard_words_and_each_output_alone(C):
    """The C entry point with Dbits, Ebits, status and rank inside guarded buffers; then each of the three outputs without the other two."""
    dims = (3, 7, 33)
    code = _code(C, dims)
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    G = 0x5A5A5A5A
    me = code.N
    for F in (33, 37):
        for tier in (1, 2):
            W = (F + 31) // 32
            nd, ne = (code.N + 1) * W, code.N * W
            b, e = (_dev(a) for a in _words(dims, F, dirty=True))
            want = _want(C, dims, F, me)
            dbuf = torch.full((nd + 64,), G, dtype=torch.int32, device="cuda")
            ebuf = torch.full((ne + 64,), G, dtype=torch.int32, device="cuda")
            sbuf = torch.full((F + 8,), -3, dtype=torch.int32, device="cuda")
            rbuf = torch.full((F + 8,), -3, dtype=torch.int32, device="cuda")
            rc = lib.bldpc_decode_erasure_ml(code._h, ptr(b), ptr(e), F, me, tier, None, ptr(dbuf[32:]), ptr(ebuf[32:]), ptr(sbuf[4:]), ptr(rbuf[4:]), st)
            torch.cuda.synchronize()
            assert rc == 0 and code.last_kernel == ("k_er_ml", "k_er_ml_ws")[tier - 1]
            d, ee, s, k = dbuf.cpu().numpy(), ebuf.cpu().numpy(), sbuf.cpu().numpy(), rbuf.cpu().numpy()
            assert (d[:32] == G).all() and (d[32 + nd:] == G).all(), "a store outside Dbits"
            assert (ee[:32] == G).all() and (ee[32 + ne:] == G).all(), "a store outside Ebits"
            assert np.array_equal(d[32:32 + nd].view(np.uint32).reshape(code.N + 1, W), want["Dbits"])
            assert np.array_equal(ee[32:32 + ne].view(np.uint32).reshape(code.N, W), want["Ebits"])
            assert (s[:4] == -3).all() and (s[4 + F:] == -3).all() and np.array_equal(s[4:4 + F], want["status"])
            assert (k[:4] == -3).all() and (k[4 + F:] == -3).all() and np.array_equal(k[4:4 + F], want["rank"])
        for kw in (dict(want_bits=True, want_erased=False), dict(want_bits=False, want_erased=True), dict(want_bits=False, want_erased=False, want_D=True)):
            r = C.LDPC_Decoder_Erasure_ML_GPU(code, b, e, F, max_erased=me, **kw)
            torch.cuda.synchronize()
            assert [k for k in ("D", "Dbits", "Ebits") if r[k] is not None] == [k for k, flag in (("D", "want_D"), ("Dbits", "want_bits"),
                                                                                                 ("Ebits", "want_erased")) if kw.get(flag)]
            _same(r, want, "one output: %s" % sorted(kw.items()))
        # without status and rank
        out = torch.full((ne,), G, dtype=torch.int32, device="cuda")
        assert lib.bldpc_decode_erasure_ml(code._h, ptr(b), ptr(e), F, me, 0, None, None, ptr(out), None, None, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_u32(out).reshape(code.N, W), want["Ebits"])


def test_scratch_that_grows_and_is_reused_by_a_smaller_call(C):
    dims = (3, 9, 96)
    code = _code(C, dims, fresh=True)
    for F, tier in ((37, "workspace"), (1, "lds"), (64, "workspace"), (33, "workspace"), (64, "lds"), (1, "workspace")):
        b, e = (_dev(a) for a in _words(dims, F))
        r = C.LDPC_Decoder_Erasure_ML_GPU(code, b, e, F, max_erased=code.N, tier=tier, want_D=True, want_bits=False, want_erased=False)  # the plan's words
        torch.cuda.synchronize()
        _same(r, _want(C, dims, F, code.N), "F=%d %s" % (F, tier))
        assert code.last_kernel == KERNEL[tier]
    code.close()


def test_an_empty_frame_list_and_a_full_one(C):
    dims = (3, 7, 33)
    J, L, Z = dims
    code = _code(C, dims)
    bits, er, cw = ml_input(dims)
    F = 40
    for tier in ("lds", "workspace"):
        # nothing erased in any frame, then every frame above the bound: no frame is listed
        clean = np_pack(cw[:, :F])
        r = C.LDPC_Decoder_Erasure_ML_GPU(code, _dev(clean), _dev(np.zeros_like(clean)), F, tier=tier, want_D=True)
        want = C.erasure_ml_host(matrix(dims), J, L, Z, clean, np.zeros_like(clean), F)
        _same(r, want, "nothing erased")
        codeword = np.flatnonzero((np.arange(F) < 3) | (np.arange(F) > 6))  # frames 3 .. 6 of the input are no codewords
        assert (want["status"] == ML_NONE).all() and want["D"][-1, codeword].all() and not want["D"][-1, 3:7].any()
        heavy = np_pack(np.repeat(er[:, ALL_ERASED:ALL_ERASED + 1], F, 1))
        r = C.LDPC_Decoder_Erasure_ML_GPU(code, _dev(clean), _dev(heavy), F, max_erased=5, tier=tier, want_D=True)
        want = C.erasure_ml_host(matrix(dims), J, L, Z, clean, heavy, F, max_erased=5)
        _same(r, want, "everything skipped")
        assert (want["status"] == ML_SKIPPED).all() and not want["Dbits"].any()
        # every frame is listed
        b, e = _words(dims, 64)
        full = [f for f in range(64) if _want(C, dims, 64, code.N)["status"][f] != ML_NONE][:F]
        bf, ef = np_pack(np_unpack(b, 64)[:, full]), np_pack(np_unpack(e, 64)[:, full])
        r = C.LDPC_Decoder_Erasure_ML_GPU(code, _dev(bf), _dev(ef), F, max_erased=code.N, tier=tier, want_D=True)
        want = C.erasure_ml_host(matrix(dims), J, L, Z, bf, ef, F, max_erased=code.N)
        _same(r, want, "every frame listed")
        assert len(full) == F and not np.isin(want["status"], (ML_NONE, ML_SKIPPED)).any()
    torch.cuda.synchronize()


def test_more_listed_frames_than_workspace_slots(C):
    """F = 64 on the workspace shape with the slot count pinned to 3 (BLDPC_ML_SLOTS, read when the plan is made): every workgroup
    takes frame after frame from the list, and its slot, bitmaps and list of positions are reused."""
    dims = WORKSPACE_DIMS
    os.environ["BLDPC_ML_SLOTS"] = "3"
    try:
        code = _code(C, dims, fresh=True)
        assert code.erasure_ml_info()["slots"] == 3
    finally:
        del os.environ["BLDPC_ML_SLOTS"]
    want = _want(C, dims, 64, 0)
    assert (~np.isin(want["status"], (ML_NONE, ML_SKIPPED))).sum() > 40
    _both(C, dims, 64, 0, code=code)
    _both(C, dims, 64, 33, "workspace", code=code)
    assert code.erasure_ml_info()["slots"] == 3 and _code(C, dims).erasure_ml_info()["slots"] > 3
    code.close()


def _others(C, c, yy, b, e):
    from test_erasure_gpu import _others as rest
    out = rest(C, c, yy)
    r = C.LDPC_Decoder_Erasure_GPU(c, b, e, int(yy.shape[1]), max_iter=100, want_D=True)
    out += [r["D"].clone(), r["Dbits"].clone(), r["Ebits"].clone(), r["iters"].clone()]
    torch.cuda.synchronize()
    return out


def test_other_decoders_unchanged_around_an_accepted_and_a_refused_call(C):
    from cuda_ldpc_amd._lib import LdpcError
    dims = WORKSPACE_DIMS
    code = _code(C, dims, fresh=True)
    bits, er, _ = ml_input(dims)
    y = torch.from_numpy(((1.0 - 2.0 * bits[:, :37]) * (1 - er[:, :37])).astype(np.float32)).cuda()
    b, e = (_dev(a) for a in _words(dims, 37))
    before = _others(C, code, y, b, e)
    assert len(before) == 18
    _both(C, dims, 37, 33, code=code)
    _both(C, dims, 37, 0, code=code, want_bits=False)
    D = torch.full((code.N + 1, 37), -7, dtype=torch.int32, device="cuda")
    kernel, said = code.last_kernel, []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS") as err:
            C.LDPC_Decoder_Erasure_ML_GPU(code, b, e, 37, tier="lds", D=D)
        said.append(str(err.value))
    torch.cuda.synchronize()
    assert said[0] == said[1] and code.last_kernel == kernel and bool((D == -7).all()), "a refused call launches nothing"
    after = _others(C, code, y, b, e)
    assert all(torch.equal(x, z) for x, z in zip(before, after))
    _both(C, dims, 37, 33, "lds", code=code)  # refused at M, taken at 33: decided per call
    code.close()


def test_refusals_on_the_device(C):
    from cuda_ldpc_amd._lib import LdpcError
    dims = (3, 9, 96)
    code = _code(C, dims)
    F, N = 4, code.N
    z = torch.zeros((N, 1), dtype=torch.int32, device="cuda")
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(F=F, bits=z, er=z, D=D, me=0, tier=0):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_erasure_ml(code._h, ptr(bits), ptr(er), F, me, tier, ptr(D), None, None, None, None, st)
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_erasure_ml"
    assert raw() == (0, "")
    assert raw(F=0) == (-1, who + ": F=0 must be positive")
    assert raw(bits=None) == (-1, who + ": null bits_in") and raw(er=None) == (-1, who + ": null erased_in")
    assert raw(D=None) == (-1, who + ": D, Dbits and Ebits are all null")
    assert raw(me=-1)[0] == -1 and raw(me=N + 1) == (-1, who + ": max_erased=%d outside [0,%d]" % (N + 1, N))
    assert raw(tier=3) == (-1, who + ": unknown tier 3")
    assert lib.bldpc_decode_erasure_ml(None, ptr(z), ptr(z), F, 0, 0, ptr(D), None, None, None, None, st) == -1
    for bad in (dict(F=0), dict(F=40), dict(D=torch.empty((N, F), dtype=torch.int32, device="cuda")), dict(want_bits=False, want_erased=False),
                dict(tier="fast")):
        with pytest.raises(ValueError):
            C.LDPC_Decoder_Erasure_ML_GPU(code, z, z, **dict(dict(F=F), **bad))
    with pytest.raises(ValueError):
        C.LDPC_Decoder_Erasure_ML_GPU(code, z.cpu(), z, F)
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    H, wc, wv = C.Get_H(os.path.join(BL, name), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    zt = torch.zeros((table.N, 1), dtype=torch.int32, device="cuda")
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*address table") as e:
            C.LDPC_Decoder_Erasure_ML_GPU(table, zt, zt, F)
        said.append(str(e.value))
    assert said[0] == said[1]
    with pytest.raises(LdpcError, match=r"\(-5\): .*address table"):
        table.erasure_ml_info()
    torch.cuda.synchronize()
    _both(C, dims, 37, 0)  # the code object decodes as before


# ---- a shipped code ---------------------------------------------------------------------------------------------------------------------
def test_a_shipped_code_on_a_ramp_around_its_cliff(C):
    """J4_L24_Z96, 64 frames of the all-zero word, frame f with 250 + 3 f erased positions (0.108 N to 0.19 N, the capacity at N / 6 = 384):
    peeling, then elimination on what it left, on both tiers."""
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    path = os.path.join(BL, name)
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, F = L * Z, 64
    rng = np.random.default_rng(5)
    er = np.zeros((N, F), np.int32)
    for f in range(F):
        er[rng.choice(N, size=250 + 3 * f, replace=False), f] = 1
    peel = C.LDPC_Decoder_Erasure_GPU(code, _dev(np.zeros((N, 2), np.uint32)), _dev(np_pack(er)), F, max_iter=100)
    want = C.erasure_ml_host(H, J, L, Z, _u32(peel["Dbits"])[:N], _u32(peel["Ebits"]), F)
    for tier in ("auto", "workspace"):
        r = C.LDPC_Decoder_Erasure_ML_GPU(code, peel["Dbits"][:N], peel["Ebits"], F, tier=tier, want_D=True)
        torch.cuda.synchronize()
        _same(r, want, name + " " + tier)
        assert code.last_kernel == ("k_er_ml_ws" if tier == "workspace" else "k_er_ml")
    left_peel, left = int((np_unpack(_u32(peel["Dbits"])[N:], F) == 0).sum()), int((want["D"][N] == 0).sum())
    print("%s: peeling leaves %d of %d frames, elimination %d; statuses %s" % (name, left_peel, F, left, np.bincount(want["status"], minlength=6).tolist()))
    assert 0 < left < left_peel < F and (want["status"] == ML_SOLVED).sum() > 0
    code.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def test_simulation_bec_with_and_without_elimination(C):
    """Two batches of 64 random codewords at p = 0.14 on J4_L24_Z96: the counters of Simulation_BEC_GPU(ml=True) recomputed with the
    host statements on the same draws, then as the sum over the ranks of a world of 2 and of 3; and ml=False gives the counters of the
    peeling loop, as before."""
    from test_erasure_gpu import _Rank, _sim
    J, L, Z = 4, 24, 96
    path = os.path.join(BL, "J4_L24_Z96_BlockH.txt")
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    F, maxIT, pn_seed, p = 64, 100, 4242, 0.14
    kw = dict(maxIT=maxIT, PN_Message=1, pn_seed=pn_seed)
    seed2, want_ml, want_peel = np.array([173, 173, 173], np.int32), np.zeros(5, np.int64), np.zeros(5, np.int64)
    for b in range(2):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F).cpu().numpy()
        cwb = C.Hard_Pack_Int_host(cw)
        bits, erased = C.BECChannel_CPU(seed2, p, N, F, CodeWord=cw)
        r = C.erasure_host(H, J, L, Z, bits, erased, F, max_iter=maxIT)
        C.Statistic_Bits_host(N, r["Dbits"], F, K, Ebits=r["Ebits"], CodeWordBits=cwb, iters=r["iters"], counters=want_peel)
        m = C.erasure_ml_host(H, J, L, Z, r["Dbits"][:N], r["Ebits"], F)
        C.Statistic_Bits_host(N, m["Dbits"], F, K, Ebits=m["Ebits"], CodeWordBits=cwb, iters=r["iters"], counters=want_ml)
    got, seed, SIM = _sim(C, code, p, F, ml=True, **kw)
    assert code.last_kernel == "k_er_ml"
    print("p=%g: peeling %s, peeling + elimination %s" % (p, want_peel.tolist(), got))
    assert SIM.num_Frames == 2 * F and got == want_ml.tolist() and np.array_equal(seed, seed2)
    assert got[0] < want_peel[0] and got[2] == want_peel[2] and got[3] == 0
    for world in (2, 3):
        total = np.zeros(5, np.int64)
        for rank in range(world):
            part, seed3, _ = _sim(C, code, p, F, dist=_Rank(rank, world), ml=True, **kw)
            total += np.array(part, np.int64)
            assert np.array_equal(seed3, seed2)
        assert total.tolist() == got, world
    for more in (dict(), dict(ml=False), dict(ml=False, ml_max_erased=5, ml_tier="workspace")):
        plain, seed4, _ = _sim(C, code, p, F, **dict(kw, **more))
        assert plain == want_peel.tolist() and np.array_equal(seed4, seed2)
    forced, _, _ = _sim(C, code, p, F, ml=True, ml_tier="workspace", **kw)
    assert forced == got and code.last_kernel == "k_er_ml_ws"
    none, _, _ = _sim(C, code, p, F, ml=True, ml_max_erased=1, **kw)  # nothing that peeling leaves has one erasure
    assert none == want_peel.tolist()
    code.close()
