"""GPU tests of erasure decoding (include/bldpc.h): the kernel k_er against the host statement bldpc_decode_erasure_host, exactly, on
Dbits, Ebits, D and iters, on the matrices, batch sizes and inputs of tests/erasure_cases.py (tests/test_erasure_cpu.py holds the host
statement against the numpy restatement on the same cases and checks that the inputs meet their conditions); garbage in the padding and
under the erasures, each output alone, guard words, a caller's stream, scratch that shrinks and grows, the other decoders of a code object
around a call, the refusals the device makes; the channel, the rate-matching and the statistics kernels against their host statements;
shipped codes; and Simulation_BEC_GPU against a loop written out from the host statements, whole and in shards."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from erasure_cases import (BATCHES, EXTREME, MAX_ITER, accepted_dims, bound_shapes, dims_id, dirty_input, erased_input, garbage_padding, matrix,
                           np_pack, np_unpack)

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


def _words(dims, F, dirty=False):
    if dirty:
        return dirty_input(dims, F)
    bits, er, _ = erased_input(dims)
    return np_pack(bits[:, :F]), np_pack(er[:, :F])


def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _want(C, dims, F, max_iter=MAX_ITER):
    """The host statement's result on the clean words: computed once per case, shared among the tests."""
    key = (dims, F, max_iter)
    if key not in _host:
        J, L, Z = dims
        _host[key] = C.erasure_host(matrix(dims), J, L, Z, *_words(dims, F), F, max_iter=max_iter)
    return _host[key]


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(r, want, what):
    assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    if r["Dbits"] is not None:
        assert np.array_equal(_u32(r["Dbits"])[-1], want["Dbits"][-1]), "flag words: " + what
        assert np.array_equal(_u32(r["Dbits"]), want["Dbits"]), "Dbits: " + what
    if r["Ebits"] is not None:
        assert np.array_equal(_u32(r["Ebits"]), want["Ebits"]), "Ebits: " + what
    if r["D"] is not None:
        assert np.array_equal(r["D"].cpu().numpy(), want["D"]), "D: " + what


def _both(C, dims, F, code=None, dirty=False, max_iter=MAX_ITER, **kw):
    code = code or _code(C, dims)
    b, e = _words(dims, F, dirty)
    r = C.LDPC_Decoder_Erasure_GPU(code, _dev(b), _dev(e), F, max_iter=max_iter, **dict(dict(want_D=True), **kw))
    torch.cuda.synchronize()
    assert code.last_kernel == "k_er"
    want = _want(C, dims, F, max_iter)
    _same(r, want, "%s F=%d max_iter=%d" % (dims_id(dims), F, max_iter))
    return r, want


@pytest.mark.parametrize("dims", accepted_dims(), ids=dims_id)
def test_every_shape_matches_the_host_statement(C, dims):
    for F in BATCHES:
        _both(C, dims, F)
    _both(C, dims, 37, max_iter=2)  # the cap cuts the history
    info = _code(C, dims).erasure_info()
    assert info == C.erasure_plan_host(matrix(dims), *dims) and info["fits"] and info["frames_per_wg"] == 32


@pytest.mark.parametrize("dims", [(3, 5, 13), (3, 9, 96), (4, 27, 64), EXTREME], ids=dims_id)
def test_garbage_in_the_padding_and_under_the_erasures(C, dims):
    for F in (1, 33, 37):
        r, _ = _both(C, dims, F, dirty=True)
        for k in ("Dbits", "Ebits"):
            assert (_u32(r[k])[:, -1] >> np.uint32(F % 32)).max() == 0, "output padding: " + k


def test_caller_provided_D_on_another_stream(C):
    dims = (3, 9, 96)
    code = _code(C, dims)
    r0, want = _both(C, dims, 37)
    b, e = (_dev(a) for a in _words(dims, 37))
    D = torch.full((code.N + 1, 37), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # D is filled and the words uploaded on the current stream
    r = C.LDPC_Decoder_Erasure_GPU(code, b, e, 37, max_iter=MAX_ITER, D=D, want_bits=False, want_erased=False, stream=stream)
    stream.synchronize()
    assert r["D"] is D and r["Dbits"] is None and r["Ebits"] is None
    _same(r, want, "D= and stream=")
    assert torch.equal(r["D"], r0["D"]) and torch.equal(r["iters"], r0["iters"])


def test_guard_words_and_each_output_alone(C):
    """The C entry point with Dbits, Ebits and iters inside guarded buffers; then each of the three outputs without the other two."""
    dims = (3, 7, 33)
    code = _code(C, dims)
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    G = 0x5A5A5A5A
    for F in (33, 37):
        W = (F + 31) // 32
        nd, ne = (code.N + 1) * W, code.N * W
        b, e = (_dev(a) for a in _words(dims, F, dirty=True))
        want = _want(C, dims, F)
        dbuf = torch.full((nd + 64,), G, dtype=torch.int32, device="cuda")
        ebuf = torch.full((ne + 64,), G, dtype=torch.int32, device="cuda")
        it = torch.full((F + 8,), -3, dtype=torch.int32, device="cuda")
        rc = lib.bldpc_decode_erasure(code._h, ptr(b), ptr(e), F, MAX_ITER, None, ptr(dbuf[32:]), ptr(ebuf[32:]), ptr(it[4:]), st)
        torch.cuda.synchronize()
        assert rc == 0 and code.last_kernel == "k_er"
        d, ee, i = dbuf.cpu().numpy(), ebuf.cpu().numpy(), it.cpu().numpy()
        assert (d[:32] == G).all() and (d[32 + nd:] == G).all(), "a store outside Dbits"
        assert (ee[:32] == G).all() and (ee[32 + ne:] == G).all(), "a store outside Ebits"
        assert np.array_equal(d[32:32 + nd].view(np.uint32).reshape(code.N + 1, W), want["Dbits"])
        assert np.array_equal(ee[32:32 + ne].view(np.uint32).reshape(code.N, W), want["Ebits"])
        assert (i[:4] == -3).all() and (i[4 + F:] == -3).all() and np.array_equal(i[4:4 + F], want["iters"])
        for kw in (dict(want_bits=True, want_erased=False), dict(want_bits=False, want_erased=True), dict(want_bits=False, want_erased=False, want_D=True)):
            r = C.LDPC_Decoder_Erasure_GPU(code, b, e, F, max_iter=MAX_ITER, **kw)
            torch.cuda.synchronize()
            assert [k for k in ("D", "Dbits", "Ebits") if r[k] is not None] == [k for k, flag in (("D", "want_D"), ("Dbits", "want_bits"),
                                                                                                 ("Ebits", "want_erased")) if kw.get(flag)]
            _same(r, want, "one output: %s" % sorted(kw.items()))
        # without iters
        out = torch.full((ne,), G, dtype=torch.int32, device="cuda")
        assert lib.bldpc_decode_erasure(code._h, ptr(b), ptr(e), F, MAX_ITER, None, None, ptr(out), None, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_u32(out).reshape(code.N, W), want["Ebits"])


def test_scratch_that_shrinks_and_grows(C):
    dims = (3, 9, 96)
    code = _code(C, dims, fresh=True)
    for F in (37, 1, 64, 33):
        b, e = (_dev(a) for a in _words(dims, F))
        r = C.LDPC_Decoder_Erasure_GPU(code, b, e, F, max_iter=MAX_ITER, want_D=True, want_bits=False, want_erased=False)  # D only: the plan's words
        torch.cuda.synchronize()
        _same(r, _want(C, dims, F), "F=%d" % F)
    assert code.last_kernel == "k_er"
    code.close()


def _others(C, c, yy):
    from test_bitflip_gpu import _others as soft
    out = soft(C, c, yy)
    if c.bitflip_info()["fits"]:
        b = C.LDPC_Decoder_BitFlip_GPU(c, C.Hard_Pack(yy), int(yy.shape[1]), max_iter=5, exit_mode=C.EXIT_PER_FRAME, want_bits=True)
        out += [b["D"].clone(), b["Dbits"].clone(), b["iters"].clone()]
    torch.cuda.synchronize()
    return out


def test_other_decoders_unchanged_around_an_erasure_call(C):
    dims = (3, 9, 96)
    code = _code(C, dims, fresh=True)
    bits, er, _ = erased_input(dims)
    y = torch.from_numpy(((1.0 - 2.0 * bits[:, :37]) * (1 - er[:, :37])).astype(np.float32)).cuda()
    before = _others(C, code, y)
    assert len(before) == 14
    _both(C, dims, 37, code=code)
    _both(C, dims, 64, code=code, want_bits=False)
    after = _others(C, code, y)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    code.close()
    # and after a refused call
    beyond = bound_shapes()[1]
    big = _code(C, beyond, fresh=True)
    yb = torch.ones((big.N, 3), device="cuda")
    before = _others(C, big, yb)
    z = torch.zeros((big.N, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(C._lib.LdpcError, match=r"\(-5\): .*LDS"):
        C.LDPC_Decoder_Erasure_GPU(big, z, z, 3)
    after = _others(C, big, yb)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
    big.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_the_shape_beyond_the_bound_is_refused_and_nothing_is_launched(C):
    from cuda_ldpc_amd._lib import LdpcError
    beyond = bound_shapes()[1]
    code = _code(C, beyond, fresh=True)
    assert not code.erasure_info()["fits"]
    F = 3
    z = torch.zeros((code.N, 1), dtype=torch.int32, device="cuda")
    D = torch.full((code.N + 1, F), -7, dtype=torch.int32, device="cuda")
    before = code.last_kernel
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*LDS") as e:
            C.LDPC_Decoder_Erasure_GPU(code, z, z, F, D=D)
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
    z = torch.zeros((code.N, 1), dtype=torch.int32, device="cuda")
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-1\): .*max_iter") as e:
            C.LDPC_Decoder_Erasure_GPU(code, z, z, F, max_iter=0)
        said.append(str(e.value))
    assert said[0] == said[1]
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")
    it = torch.empty(F, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(F=F, bits=z, er=z, D=D, it=it, max_iter=5):
        rc = lib.bldpc_decode_erasure(code._h, ptr(bits), ptr(er), F, max_iter, ptr(D), None, None, ptr(it), st)
        return rc, lib.bldpc_last_error().decode()

    who = "bldpc_decode_erasure"
    assert raw(F=0) == (-1, who + ": F=0 must be positive")
    assert raw(bits=None) == (-1, who + ": null bits_in") and raw(er=None) == (-1, who + ": null erased_in")
    assert raw(D=None) == (-1, who + ": D, Dbits and Ebits are all null")
    assert raw(max_iter=0) == (-1, who + ": max_iter=0 must be at least 1")
    assert raw(it=None)[0] == 0  # iters is optional
    assert lib.bldpc_decode_erasure(None, ptr(z), ptr(z), F, 5, ptr(D), None, None, ptr(it), st) == -1
    for bad in (dict(F=0), dict(F=40), dict(D=torch.empty((code.N, F), dtype=torch.int32, device="cuda")), dict(want_bits=False, want_erased=False)):
        with pytest.raises(ValueError):
            C.LDPC_Decoder_Erasure_GPU(code, z, z, **dict(dict(F=F), **bad))
    with pytest.raises(ValueError):
        C.LDPC_Decoder_Erasure_GPU(code, z.cpu(), z, F)
    with pytest.raises(ValueError):
        C.LDPC_Decoder_Erasure_GPU(code, z, z[:-1], F)
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    H, wc, wv = C.Get_H(os.path.join(BL, name), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    zt = torch.zeros((table.N, 1), dtype=torch.int32, device="cuda")
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*address table") as e:
            C.LDPC_Decoder_Erasure_GPU(table, zt, zt, F)
        said.append(str(e.value))
    assert said[0] == said[1]
    with pytest.raises(LdpcError, match=r"\(-5\): .*address table"):
        table.erasure_info()
    for p in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            C.BECChannel_GPU(np.array([1, 2, 3], np.int32), p, 8, 4)
    with pytest.raises(LdpcError, match=r"\(-1\): .*seed"):
        C.BECChannel_GPU(np.array([1, 2, 63599], np.int32), 0.1, 8, 4)
    cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
    Db = torch.zeros((code.N + 1, 1), dtype=torch.int32, device="cuda")
    assert lib.bldpc_statistic_bits(None, ptr(Db), None, None, F, 0, None, ptr(cnt), st) == -1
    assert lib.bldpc_statistic_bits(code._h, None, None, None, F, 0, None, ptr(cnt), st) == -1
    assert lib.bldpc_statistic_bits(code._h, ptr(Db), None, None, 0, 0, None, ptr(cnt), st) == -1
    assert lib.bldpc_statistic_bits(code._h, ptr(Db), None, None, F, code.N + 1, None, ptr(cnt), st) == -1
    assert lib.bldpc_statistic_bits(code._h, ptr(Db), None, None, F, -1, None, ptr(cnt), st) == -1
    assert lib.bldpc_statistic_bits(code._h, ptr(Db), None, None, F, 0, None, None, st) == -1
    for bad in (dict(Dbits=Db[:-1]), dict(Ebits=Db), dict(length=code.N + 1), dict(counters=cnt[:4]), dict(iters=it.long())):
        kw = dict(dict(Dbits=Db, counters=cnt), **bad)
        with pytest.raises(ValueError):
            C.Statistic_Bits(code, kw.pop("Dbits"), F, kw.pop("counters"), **kw)
    rm = C.RateMatch(code.N, [0], [5])
    tx = torch.zeros((rm.E, 1), dtype=torch.int32, device="cuda")
    assert lib.bldpc_rm_select_bits(rm._h, None, F, ptr(tx), st) == -1 and lib.bldpc_rm_select_bits(None, ptr(z), F, ptr(tx), st) == -1
    assert lib.bldpc_rm_recover_bits(rm._h, ptr(tx), None, F, None, ptr(z), st) == -1
    assert lib.bldpc_rm_recover_bits(rm._h, ptr(tx), None, 0, ptr(z), ptr(z), st) == -1
    with pytest.raises(ValueError):
        C.RM_Select_Bits(rm, tx, F)
    with pytest.raises(ValueError):
        C.RM_Recover_Bits(rm, z, F)
    torch.cuda.synchronize()
    assert not cnt.any()
    _both(C, dims, 37)  # the code object decodes as before


# ---- channel, rate matching, statistics -------------------------------------------------------------------------------------------------
def test_bec_kernel_equals_the_host_channel(C):
    """N = 77 is no multiple of the run of rows a thread walks; F = 37 and 300 leave partly filled words, waves and workgroups; the
    second call starts from the advanced seed; the mask is the BSC kernel's flip mask."""
    N = 77
    for F in (37, 300):
        cw = torch.from_numpy(np.random.default_rng(F).integers(0, 2, size=(N, F)).astype(np.int32)).cuda()
        for word in (None, cw):
            for p in (0.11, 0.0, 1.0):
                sd, sh = np.array([173, 173, 173], np.int32), np.array([173, 173, 173], np.int32)
                for call in range(2):
                    flips = C.BSCChannel_GPU(sd.copy(), min(p, 0.5), N, F)
                    got = C.BECChannel_GPU(sd, p, N, F, CodeWord=word)
                    want = C.BECChannel_CPU(sh, p, N, F, CodeWord=None if word is None else word.cpu().numpy())
                    for g, w in zip(got, want):
                        assert g.dtype == torch.int32 and np.array_equal(_u32(g), w), (F, p, call)
                    assert np.array_equal(sd, sh)
                    if p <= 0.5:
                        assert torch.equal(got[1], flips)
            assert 0 < np_unpack(want[1], F).sum()


def test_rate_matching_kernels_equal_their_host_statements(C):
    from test_erasure_cpu import rm_profiles
    N = 60
    rng = np.random.default_rng(22)
    for rm in rm_profiles(C, N):
        for F in (1, 37, 300):
            cw = rng.integers(0, 2, size=(N, F)).astype(np.int32)
            cw[rm.shorten] = 0
            bits = garbage_padding(np_pack(cw), F)
            tx = C.RM_Select_Bits(rm, _dev(bits), F)
            assert tx.dtype == torch.int32 and np.array_equal(_u32(tx), C.RM_Select_Bits_host(rm, bits, F))
            assert torch.equal(tx, C.Hard_Pack_Int(C.RM_Select(rm, torch.from_numpy(cw).cuda()))), "select is pack of the int32 select"
            rxe = garbage_padding(np_pack((rng.random((rm.E, F)) < 0.4).astype(np.int32)), F, seed=3)
            rx = garbage_padding(np_pack(rng.integers(0, 2, size=(rm.E, F)).astype(np.int32)), F, seed=4)  # value bits under the erasures too
            for mask in (rxe, None):
                got = C.RM_Recover_Bits(rm, _dev(rx), F, rx_erased=None if mask is None else _dev(mask))
                want = C.RM_Recover_Bits_host(rm, rx, F, rx_erased=mask)
                for g, w in zip(got, want):
                    assert np.array_equal(_u32(g), w), (rm.is_circular, rm.E, F, mask is None)


def test_statistic_bits_kernel_equals_its_host_statement(C):
    """F = 37 and 64 on a short code, F = 1100 (35 words: two workgroups, the second partly filled) on the same: accumulation over two
    calls, length < N and the default length, and each of the three optional arguments absent."""
    dims = (3, 9, 96)
    J, L, Z = dims
    N = L * Z
    code = _code(C, dims)
    bits, er, cw = erased_input(dims)
    for F in (37, 64, 1100):
        reps = (F + 63) // 64
        b, e, c = (np.tile(a, (1, reps))[:, :F] for a in (bits, er, cw))
        r = C.erasure_host(matrix(dims), J, L, Z, np_pack(b), np_pack(e), F, max_iter=3)
        Db, Eb, cwb, it = _dev(garbage_padding(r["Dbits"], F)), _dev(r["Ebits"]), _dev(garbage_padding(np_pack(c), F, seed=2)), torch.from_numpy(r["iters"]).cuda()
        for length in (N, 100, 0):
            for kw in (dict(Ebits=1, CodeWordBits=1, iters=1), dict(CodeWordBits=1, iters=1), dict(Ebits=1, iters=1), dict(Ebits=1, CodeWordBits=1)):
                dev = {k: dict(Ebits=Eb, CodeWordBits=cwb, iters=it)[k] for k in kw}
                host = {k: dict(Ebits=r["Ebits"], CodeWordBits=np_pack(c), iters=r["iters"])[k] for k in kw}
                cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
                C.Statistic_Bits(code, Db, F, cnt, length=length, **dev)
                want = C.Statistic_Bits_host(N, r["Dbits"], F, length or code.K, **host)
                assert cnt.cpu().tolist() == want.tolist(), (F, length, sorted(kw))
                C.Statistic_Bits(code, Db, F, cnt, length=length, **dev)  # accumulates
                assert cnt.cpu().tolist() == (2 * want).tolist(), (F, length, sorted(kw))
        assert want[0] > 0 and want[1] > 0


@pytest.mark.parametrize("F", [37, 512 * 32 + 37, 4096 * 32 + 37])
def test_statistic_bits_at_every_tile_width(C, F):
    """The kernel gives a workgroup 2, 8 or 32 words of a row by the width of the batch (below 512 words, below 4096, above): random
    words on the shortest code at a batch in each range, the last word partly filled."""
    dims = (3, 5, 13)
    code = _code(C, dims)
    N, W = code.N, (F + 31) // 32
    rng = np.random.default_rng(F)
    Db, Eb, cwb = (rng.integers(0, 1 << 32, size=(rows, W), dtype=np.uint64).astype(np.uint32) for rows in (N + 1, N, N))
    Eb &= rng.integers(0, 1 << 32, size=(N, W), dtype=np.uint64).astype(np.uint32)
    it = rng.integers(0, 50, size=F).astype(np.int32)
    for length in (N, 17):
        cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
        C.Statistic_Bits(code, _dev(Db), F, cnt, Ebits=_dev(Eb), CodeWordBits=_dev(cwb), iters=torch.from_numpy(it).cuda(), length=length)
        want = C.Statistic_Bits_host(N, Db, F, length, Ebits=Eb, CodeWordBits=cwb, iters=it)
        assert cnt.cpu().tolist() == want.tolist() and want[:4].min() > 0, (F, length)


# ---- shipped codes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,J,L,Z,step", [("J4_L24_Z96_BlockH.txt", 4, 24, 96, 6.0), ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 30.0),
                                             ("PON_LDPC.txt", 12, 69, 256, 45.0)])
def test_shipped_codes_on_an_erasure_ramp(C, name, J, L, Z, step):
    """64 frames of the all-zero word, frame f with int(f * step) erased positions: both sides of each code's waterfall."""
    path = os.path.join(BL, name)
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, F = L * Z, 64
    rng = np.random.default_rng(5)
    er = np.zeros((N, F), np.int32)
    for f in range(F):
        er[rng.choice(N, size=int(f * step), replace=False), f] = 1
    bits, erased = np.zeros((N, 2), np.uint32), np_pack(er)
    r = C.LDPC_Decoder_Erasure_GPU(code, _dev(bits), _dev(erased), F, max_iter=100, want_D=True)
    torch.cuda.synchronize()
    want = C.erasure_host(H, J, L, Z, bits, erased, F, max_iter=100)
    _same(r, want, name)
    u = np.unique(want["iters"])
    print("%s: iters %s, %d of %d frames recovered" % (name, u.tolist(), int(want["D"][N].sum()), F))
    assert code.last_kernel == "k_er" and code.erasure_info()["fits"] and u.size >= 3 and 0 < want["D"][N].sum() < F
    code.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
class _Rank:
    """One rank of a world of `world` without a process group (as in test_rate_match_gpu.py): the all-reduce is the sum the test makes."""

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


def _sim(C, code, p, F, dist=None, **kw):
    from cuda_ldpc_amd.simulation import Simulation_BEC_GPU
    SIM, seed = C.SimCounters(), np.array([173, 173, 173], np.int32)
    Simulation_BEC_GPU(code, seed, p, SIM, Num_Frames_OneTime=F, max_batches=2, leastTestFrames=10 ** 9, log=None, dist=dist, **kw)
    return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames], seed, SIM


@pytest.mark.parametrize("profile", ["none", "linear", "circular"])
def test_simulation_bec_equals_a_loop_over_the_host_statements(C, profile):
    """Two batches of 64 random codewords: the counters of Simulation_BEC_GPU recomputed with the host statements on the same draws, then
    the same counters as the sum over the ranks of a world of 2 and of 3."""
    from cuda_ldpc_amd.simulation import Simulation_BEC_GPU
    J, L, Z = 4, 24, 96
    path = os.path.join(BL, "J4_L24_Z96_BlockH.txt")
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, K = code.N, code.K
    F, maxIT, pn_seed = 64, 100, 4242
    sh, pu = list(range(0, 24)), list(range(2188, 2260))
    rm = dict(none=None, linear=C.RateMatch(N, sh, pu), circular=C.RateMatch.circular(N, sh, pu, 100, N + 300))[profile]
    p = dict(none=0.125, linear=0.10, circular=0.13)[profile]
    for PN in (1, 0):
        kw = dict(maxIT=maxIT, PN_Message=PN, pn_seed=pn_seed, rate_match=rm)
        got, seed, SIM = _sim(C, code, p, F, **kw)
        seed2, want = np.array([173, 173, 173], np.int32), np.zeros(5, np.int64)
        for b in range(2):
            cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F, rate_match=rm).cpu().numpy() if PN else np.zeros((N, F), np.int32)
            cwb = C.Hard_Pack_Int_host(cw)
            if rm is None:
                bits, erased = C.BECChannel_CPU(seed2, p, N, F, CodeWord=cw)
            else:
                rx, rxe = C.BECChannel_CPU(seed2, p, rm.E, F, CodeWord=C.RM_Select_host(rm, cw))
                assert np.array_equal(rx, C.RM_Select_Bits_host(rm, cwb, F) & ~rxe)
                bits, erased = C.RM_Recover_Bits_host(rm, rx, F, rx_erased=rxe)
            r = C.erasure_host(H, J, L, Z, bits, erased, F, max_iter=maxIT)
            C.Statistic_Bits_host(N, r["Dbits"], F, K, Ebits=r["Ebits"], CodeWordBits=cwb if PN else None, iters=r["iters"], counters=want)
        print("peeling at p=%g, profile %s, PN %d: counters %s" % (p, profile, PN, got))
        assert SIM.num_Frames == 2 * F and got == want.tolist() and np.array_equal(seed, seed2)
        assert 0 < got[0] < 2 * F and got[3] == 0
        for world in (2, 3):
            total = np.zeros(5, np.int64)
            for rank in range(world):
                part, seed3, _ = _sim(C, code, p, F, dist=_Rank(rank, world), **kw)
                total += np.array(part, np.int64)
                assert np.array_equal(seed3, seed2), "every rank advances the seed by the whole batch"
            assert total.tolist() == got, (world, PN)
    for bad in (dict(PN_Message=2), dict(maxIT=0), dict(rate_match=C.RateMatch(N - 1, [], [0]))):
        with pytest.raises(ValueError):
            Simulation_BEC_GPU(code, np.array([173, 173, 173], np.int32), p, C.SimCounters(), max_batches=1, log=None, **bad)
    with pytest.raises(ValueError):
        Simulation_BEC_GPU(code, np.array([173, 173, 173], np.int32), 1.2, C.SimCounters(), max_batches=1, log=None)
    code.close()
