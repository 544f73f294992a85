"""The device halves of both encoders and syndrome checks (k_enc_pack, k_enc_pack_short, k_enc_parity, k_syndrome_part,
k_syndrome_final; k_nbenc_pack, k_nbenc_parity, k_nb_syndrome) on the generated codes of tests/enc_shape_cases.py, against the numpy
reference of that module: K' < 64, N and K' that are no multiples of 64, one or two live words in the second register tile of P, odd
Z, a repeated block row, K' = 20 480 (all 160 KiB of LDS) and its refusal one block column later, scattered information positions
under shortening; GF(4) ... GF(256), a last LDS chunk of 4 symbols, sentinel padding across a chunk boundary, rank mod 8 = 1 and
rank-deficient codes.  Everything is compared exactly; tests/test_enc_shapes_cpu.py holds the cases and the host generators."""
import ctypes

import numpy as np
import pytest
import torch

import enc_shape_cases as E
import nb_shape_cases as S
from test_encoder_cpu import encode_np, syndrome_np
from test_nb_encoder_cpu import encode_np as nb_encode_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


@pytest.fixture(scope="module")
def nb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cuda_ldpc_amd import nbldpc
    return nbldpc


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ======================================================================================================================= binary codes
_bcodes = {}
ENCODABLE = [cid for cid in E.B_IDS if cid != "lds_over"]
SMALL = [cid for cid in ENCODABLE if cid != "lds_full"]
CASE_F = [(cid, F) for cid in ENCODABLE for F in (1, 65) if (cid, F) != ("lds_full", 1)]


def _bcode(C, cid):
    """(code object, flat shifts, reference generator) of a binary case; one code object per case for the whole module."""
    if cid not in _bcodes:
        c = E.B_BY_ID[cid]
        H = np.ascontiguousarray(E.bin_h(cid)).reshape(-1)
        _bcodes[cid] = (C.BinaryCode.from_shifts(H, c.J, c.L, c.Z), H, E.bin_ref(cid))
    return _bcodes[cid]


def _check_codewords(cid, cw, msg, H, ref):
    """cw int [N, F] is the encoding of msg [K', F] (bit 0): 0/1 only, systematic on the reference's info_pos, parity = the
    reference's P * msg, H * c = 0."""
    c = E.B_BY_ID[cid]
    assert set(np.unique(cw)) <= {0, 1}
    assert np.array_equal(cw[ref["info_pos"]], msg & 1), "not systematic on the reference's information positions"
    assert np.array_equal(cw, encode_np(ref, c.L * c.Z, msg)), "differs from the encoding through the reference's P"
    assert not syndrome_np(H, c.J, c.L, c.Z, cw.astype(np.uint8)).any(), "H * c != 0"


@pytest.mark.parametrize("cid", E.B_IDS)
def test_binary_encoder_info_is_the_reference(C, cid):
    code, H, ref = _bcode(C, cid)
    assert (code.K_info, code.rank) == (ref["K_info"], ref["rank"]) and np.array_equal(code.info_positions, ref["info_pos"])


@pytest.mark.parametrize("cid,F", CASE_F)
def test_binary_encode(C, cid, F):
    code, H, ref = _bcode(C, cid)
    rng = np.random.default_rng(F * 31 + len(cid))
    msg = rng.integers(0, 1 << 31, (ref["K_info"], F), dtype=np.int32)  # only bit 0 counts
    cw = C.Encode(code, torch.from_numpy(msg).cuda())
    torch.cuda.synchronize()
    _check_codewords(cid, cw.cpu().numpy(), msg, H, ref)
    ones = C.Encode(code, torch.ones((ref["K_info"], F), dtype=torch.int32, device="cuda")).cpu().numpy()
    _check_codewords(cid, ones, np.ones((ref["K_info"], F), np.int32), H, ref)


@pytest.mark.parametrize("cid,F", CASE_F)
def test_binary_pn_codewords(C, cid, F):
    from cuda_ldpc_amd.bldpc import pn_messages
    code, H, ref = _bcode(C, cid)
    seed = 0xDEADBEEF12345678 + F
    cw, msg = C.PN_CodeWords(code, seed, F + 3, want_msg=True)
    torch.cuda.synchronize()
    want = pn_messages(seed, ref["K_info"], F + 3)
    assert np.array_equal(msg.cpu().numpy(), want), "messages differ from the counter rule"
    _check_codewords(cid, cw.cpu().numpy(), want, H, ref)
    tail, tmsg = C.PN_CodeWords(code, seed, F, first_frame=3, want_msg=True)
    assert torch.equal(tail, cw[:, 3:].contiguous()) and torch.equal(tmsg, msg[:, 3:].contiguous()), "a batch at first_frame = 3"


def _syndrome_batch(C, code, ref, N, F, rng, order):
    """int32 [N + 1, F]: a third valid words, a third with one flipped bit, a third random, in the given order of the thirds."""
    n = F // 3
    valid = C.PN_CodeWords(code, 3 + F, n).cpu().numpy()
    flipped = valid.copy()
    flipped[rng.integers(0, N, n), np.arange(n)] ^= 1
    parts = dict(valid=valid, flipped=flipped, random=rng.integers(0, 2, (N, F - 2 * n), dtype=np.int32))
    D = np.concatenate([parts[k] for k in order], axis=1)
    return np.concatenate([D, rng.integers(0, 2, (1, F), dtype=np.int32)])


@pytest.mark.parametrize("cid", SMALL)
def test_binary_syndrome_smaller_then_larger_batch(C, cid):
    """One fresh code object, F = 300, 40, 700 in that order: the scratch counters are grown and zeroed by the first and the third
    call and must have been left zeroed for the second, whose valid words sit where the first call counted the most."""
    c = E.B_BY_ID[cid]
    enc, H, ref = _bcode(C, cid)
    code = C.BinaryCode.from_shifts(H, c.J, c.L, c.Z)
    rng = np.random.default_rng(11)
    N = code.N
    for F, order in ((300, ("random", "flipped", "valid")), (40, ("valid", "flipped", "random")), (700, ("flipped", "random", "valid"))):
        D = _syndrome_batch(C, enc, ref, N, F, rng, order)
        want = syndrome_np(H, c.J, c.L, c.Z, D[:N].astype(np.uint8)).sum(0).astype(np.int32)
        Dt = torch.from_numpy(D).cuda()
        r = C.Syndrome(code, Dt, into_flag_row=True)
        torch.cuda.synchronize()
        assert np.array_equal(r["unsat"].cpu().numpy(), want), "unsatisfied checks, F = %d" % F
        assert np.array_equal(Dt[N].cpu().numpy(), (want == 0).astype(np.int32)), "flags, F = %d" % F
        assert np.array_equal(Dt[:N].cpu().numpy(), D[:N]), "rows 0 .. N-1 of D changed"
        size = dict(valid=F // 3, flipped=F // 3, random=F - 2 * (F // 3))
        cut = np.cumsum([0] + [size[k] for k in order])
        by = {k: want[cut[i]:cut[i + 1]] for i, k in enumerate(order)}
        assert (by["valid"] == 0).all() and (by["flipped"] > 0).all() and (by["random"] > 0).any()
    code.close()


@pytest.mark.parametrize("cid", ["k_lt_64", "n_500"])
def test_binary_guard_elements(C, cid):
    """Through the C ABI with CodeWord (and msg) inside larger tensors filled with a marker: nothing outside [N][F] ([K'][F]) changes."""
    from cuda_ldpc_amd._lib import check, lib
    from cuda_ldpc_amd.bldpc import pn_messages
    code, H, ref = _bcode(C, cid)
    N, K, F, G = code.N, ref["K_info"], 65, 128
    msg = np.random.default_rng(3).integers(0, 2, (K, F), dtype=np.int32)
    buf = torch.full((N * F + 2 * G,), -7, dtype=torch.int32, device="cuda")
    check(lib.bldpc_encode(code._h, _ptr(torch.from_numpy(msg).cuda()), F, _ptr(buf[G:]), _stream()), "encode")
    torch.cuda.synchronize()
    assert bool((buf[:G] == -7).all()) and bool((buf[G + N * F:] == -7).all()), "bldpc_encode wrote outside CodeWord"
    _check_codewords(cid, buf[G:G + N * F].reshape(N, F).cpu().numpy(), msg, H, ref)
    buf.fill_(-7)
    mbuf = torch.full((K * F + 2 * G,), -7, dtype=torch.int32, device="cuda")
    check(lib.bldpc_encode_random(code._h, ctypes.c_ulonglong(99), 0, F, _ptr(mbuf[G:]), _ptr(buf[G:]), _stream()), "encode_random")
    torch.cuda.synchronize()
    assert bool((buf[:G] == -7).all()) and bool((buf[G + N * F:] == -7).all()), "bldpc_encode_random wrote outside CodeWord"
    assert bool((mbuf[:G] == -7).all()) and bool((mbuf[G + K * F:] == -7).all()), "bldpc_encode_random wrote outside msg"
    want = pn_messages(99, K, F)
    assert np.array_equal(mbuf[G:G + K * F].reshape(K, F).cpu().numpy(), want)
    _check_codewords(cid, buf[G:G + N * F].reshape(N, F).cpu().numpy(), want, H, ref)


def test_lds_full_syndrome(C):
    """K' = 20 480 encodes (test_binary_encode, test_binary_pn_codewords); its words pass the device syndrome, flipped ones do not."""
    code, H, ref = _bcode(C, "lds_full")
    c = E.B_BY_ID["lds_full"]
    F = 65
    cw = C.PN_CodeWords(code, 5, F)
    D = torch.cat([cw, torch.zeros((1, F), dtype=torch.int32, device="cuda")]).contiguous()
    D[torch.arange(0, code.N, 331, device="cuda")[:32], torch.arange(32, device="cuda")] ^= 1
    want = syndrome_np(H, c.J, c.L, c.Z, D[:code.N].cpu().numpy().astype(np.uint8)).sum(0).astype(np.int32)
    r = C.Syndrome(code, D)
    assert np.array_equal(r["unsat"].cpu().numpy(), want) and (want[:32] > 0).all() and (want[32:] == 0).all()
    assert np.array_equal(D[code.N].cpu().numpy(), (want == 0).astype(np.int32))


def test_lds_over_is_refused(C):
    """One block column past K' = 20 480 the slices of a frame group no longer fit LDS: Encode and PN_CodeWords refuse with
    BLDPC_EUNSUPPORTED, the generator's K' is still reported and the syndrome check still works."""
    from cuda_ldpc_amd._lib import LdpcError
    code, H, ref = _bcode(C, "lds_over")
    c = E.B_BY_ID["lds_over"]
    K, F = ref["K_info"], 65
    assert K > E.LDS_MAX_INFO_BITS and code.K_info == K
    with pytest.raises(LdpcError, match=r"\(-5\).*fit LDS"):
        C.Encode(code, torch.zeros((K, F), dtype=torch.int32, device="cuda"))
    with pytest.raises(LdpcError, match=r"\(-5\).*fit LDS"):
        C.PN_CodeWords(code, 1, F)
    assert code.K_info == K and code.rank == ref["rank"] and np.array_equal(code.info_positions, ref["info_pos"])
    rng = np.random.default_rng(9)
    cw = encode_np(ref, code.N, rng.integers(0, 2, (K, F), dtype=np.int32)).astype(np.int32)
    cw[rng.integers(0, code.N, 32), np.arange(32)] ^= 1
    want = syndrome_np(H, c.J, c.L, c.Z, cw.astype(np.uint8)).sum(0).astype(np.int32)
    r = C.Syndrome(code, torch.from_numpy(cw).cuda(), into_flag_row=False)
    assert np.array_equal(r["unsat"].cpu().numpy(), want) and np.array_equal(r["flag"].cpu().numpy(), (want == 0).astype(np.int32))
    assert (want[:32] > 0).all() and (want[32:] == 0).all()


@pytest.mark.parametrize("cid", ["n_500", "kw_34_odd"])
def test_binary_shortened_packing_through_scattered_positions(C, cid):
    from cuda_ldpc_amd._lib import LdpcError
    from cuda_ldpc_amd.bldpc import pn_messages
    code, H, ref = _bcode(C, cid)
    pos, K, N = ref["info_pos"], ref["K_info"], code.N
    assert not np.array_equal(pos, np.arange(K)), "information positions are not 0 .. K'-1"
    ks = np.unique(np.r_[0, K - 1, 62, 63, 64, 65, np.arange(7, K, 37), np.flatnonzero(pos != np.arange(K))[:8]])
    parity = np.setdiff1d(np.arange(N), pos)
    rm = C.RateMatch(N, pos[ks], parity[[0, 5, len(parity) // 2, len(parity) - 1]])
    F, seed = 65, 777
    cw, msg = C.PN_CodeWords(code, seed, F, want_msg=True, rate_match=rm)
    torch.cuda.synchronize()
    want = pn_messages(seed, K, F)
    assert want[ks].any(axis=1).all(), "the rule itself sets every one of these bits in some frame"
    want[ks] = 0
    assert np.array_equal(msg.cpu().numpy(), want), "the rule's messages with the shortened bits forced to 0"
    _check_codewords(cid, cw.cpu().numpy(), want, H, ref)
    assert not cw.cpu().numpy()[pos[ks]].any()
    alone = C.PN_CodeWords(code, seed, F - 3, first_frame=3, rate_match=rm)
    assert torch.equal(alone, cw[:, 3:].contiguous())
    with pytest.raises(LdpcError, match="parity position"):
        C.PN_CodeWords(code, seed, F, rate_match=C.RateMatch(N, [int(pos[0]), int(parity[1])]))


def test_n_500_chain_over_64qam_without_noise(C):
    """N = 500 is no multiple of 6: encode, map, channel at sigma 0, demap, hard decision, syndrome."""
    import os
    from conftest import DATA
    code, H, ref = _bcode(C, "n_500")
    F, m = 65, 6
    con = torch.from_numpy(C.Get_CONSTELLATION(os.path.join(DATA, "nb", "Constellation", "GRAY_64QAM.txt"), 64)).cuda()
    cw = C.PN_CodeWords(code, 99, F)
    sym = C.Modulate_QAM(cw, code.N, m)
    assert sym.shape == (F, 84)
    rx = C.AWGNChannel_QAM_GPU(np.array([173, 173, 173], np.int32), 0.0, sym, con)
    assert torch.equal(rx, con[sym.long()])
    y = C.Demodulate_QAM(rx, con, 1.0, code.N)
    hard = (y < 0).int()
    assert torch.equal(hard, cw) and bool((y != 0).all())
    D = torch.cat([hard, torch.zeros((1, F), dtype=torch.int32, device="cuda")]).contiguous()
    r = C.Syndrome(code, D)
    assert bool((D[code.N] == 1).all()) and not bool(r["unsat"].any())


# ======================================================================================================================== GF(q) codes
_nbcodes = {}


def _nbcode(nb, cid):
    """(NBCode, multiply table int64, reference generator) of a GF(q) case."""
    if cid not in _nbcodes:
        mpath, gpath = E.nb_files(cid)
        q = E.nb_code(cid).q
        mul, _, _ = nb.GFInitial(q, gpath)
        assert np.array_equal(mul, S.gf_tables(q)[0])
        _nbcodes[cid] = (nb.NBCode(mpath, mul), S.gf_tables(q)[0], E.nb_ref(cid))
    return _nbcodes[cid]


def _nb_syndrome_np(cid, mul, words):
    """[B, M] check sums over GF(q) of words [B, N] (low log2 q bits), from the case's edge list."""
    c = E.nb_code(cid)
    w = np.asarray(words, np.int64) & (c.q - 1)
    s = np.zeros((w.shape[0], c.M), np.int64)
    for r, v, h in c.edges:
        s[:, r] ^= mul[h, w[:, v]]
    return s


def _check_nb_codewords(cid, cw, msg, mul, ref):
    c = E.nb_code(cid)
    assert cw.min() >= 0 and cw.max() < c.q
    assert np.array_equal(cw[:, ref["info_pos"]], msg & (c.q - 1)), "not systematic on the reference's information positions"
    assert np.array_equal(cw, nb_encode_np(ref, c.N, mul, msg)), "parity symbols differ from the reference's P * msg"
    assert not _nb_syndrome_np(cid, mul, cw).any(), "H * c != 0 over GF(%d)" % c.q


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("cid", E.NB_IDS)
def test_nb_encode(nb, cid, B):
    code, mul, ref = _nbcode(nb, cid)
    q, K = code.q, ref["K_info"]
    assert (code.K_info, code.rank) == (K, ref["rank"]) and np.array_equal(code.info_positions, ref["info_pos"])
    rng = np.random.default_rng(B * 7 + len(cid))
    msg = rng.integers(0, 1 << 30, (B, K), dtype=np.int32)  # only the low log2 q bits count
    cw = nb.Encode(code, torch.from_numpy(msg).cuda())
    flag = nb.Syndrome(code, cw)["flag"]
    torch.cuda.synchronize()
    _check_nb_codewords(cid, cw.cpu().numpy(), msg, mul, ref)
    assert bool((flag == 1).all()), "the device syndrome rejects an encoded word"
    edge = np.stack([np.zeros(K, np.int32), np.full(K, q - 1, np.int32)])  # all-zero and all q-1 messages
    ecw = nb.Encode(code, torch.from_numpy(edge).cuda()).cpu().numpy()
    _check_nb_codewords(cid, ecw, edge, mul, ref)
    assert not ecw[0].any()


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("cid", E.NB_IDS)
def test_nb_encode_random(nb, cid, B):
    code, mul, ref = _nbcode(nb, cid)
    seed = 0xDEADBEEF12345678 + B
    cw, msg = nb.PN_CodeWords(code, seed, B + 3, want_msg=True)
    torch.cuda.synchronize()
    want = nb.pn_messages(seed, ref["K_info"], code.q, B + 3)
    assert np.array_equal(msg.cpu().numpy(), want), "messages differ from the counter rule"
    _check_nb_codewords(cid, cw.cpu().numpy(), want, mul, ref)
    tail, tmsg = nb.PN_CodeWords(code, seed, B, first_frame=3, want_msg=True)
    assert torch.equal(tail, cw[3:].contiguous()) and torch.equal(tmsg, msg[3:].contiguous()), "a batch at first_frame = 3"


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("cid", E.NB_IDS)
def test_nb_syndrome(nb, cid, B):
    code, mul, ref = _nbcode(nb, cid)
    c = E.nb_code(cid)
    rng = np.random.default_rng(11 + B)
    valid = nb_encode_np(ref, c.N, mul, rng.integers(0, c.q, (B, ref["K_info"])))
    seen = np.unique([v for _, v, _ in c.edges])  # a twin may have a column that no check sees
    bad = valid.copy()
    bad[np.arange(B), rng.choice(seen, B)] ^= rng.integers(1, c.q, B)  # one symbol changed
    rnd = rng.integers(0, c.q, (B, c.N))
    words = np.concatenate([valid, bad, rnd, valid])
    words = (words + (rng.integers(0, 1 << 20, words.shape) << 8)).astype(np.int32)  # bits above the low m are not read
    words[:B] = valid
    r = nb.Syndrome(code, torch.from_numpy(words).cuda())
    torch.cuda.synchronize()
    unsat = (_nb_syndrome_np(cid, mul, words) != 0).sum(1)
    assert np.array_equal(r["unsat"].cpu().numpy(), unsat)
    assert np.array_equal(r["flag"].cpu().numpy(), (unsat == 0).astype(np.int32))
    assert (unsat[:B] == 0).all() and (unsat[B:2 * B] > 0).all() and (unsat[3 * B:] == 0).all()


@pytest.mark.parametrize("cid", ["q4_pad", "q128_rank1"])
def test_nb_guard_elements(nb, cid):
    from cuda_ldpc_amd.nbldpc import _check, lib
    code, mul, ref = _nbcode(nb, cid)
    N, K, B, G = code.N, ref["K_info"], 65, 128
    msg = np.random.default_rng(3).integers(0, code.q, (B, K), dtype=np.int32)
    buf = torch.full((B * N + 2 * G,), -7, dtype=torch.int32, device="cuda")
    _check(lib.nbldpc_encode(code._h, _ptr(torch.from_numpy(msg).cuda()), B, _ptr(buf[G:]), _stream()), "encode")
    torch.cuda.synchronize()
    assert bool((buf[:G] == -7).all()) and bool((buf[G + B * N:] == -7).all()), "nbldpc_encode wrote outside CodeWord_sym"
    _check_nb_codewords(cid, buf[G:G + B * N].reshape(B, N).cpu().numpy(), msg, mul, ref)
    buf.fill_(-7)
    mbuf = torch.full((B * K + 2 * G,), -7, dtype=torch.int32, device="cuda")
    _check(lib.nbldpc_encode_random(code._h, ctypes.c_ulonglong(99), 0, B, _ptr(mbuf[G:]), _ptr(buf[G:]), _stream()), "encode_random")
    torch.cuda.synchronize()
    assert bool((buf[:G] == -7).all()) and bool((buf[G + B * N:] == -7).all()), "nbldpc_encode_random wrote outside CodeWord_sym"
    assert bool((mbuf[:G] == -7).all()) and bool((mbuf[G + B * K:] == -7).all()), "nbldpc_encode_random wrote outside msg"
    want = nb.pn_messages(99, K, code.q, B)
    assert np.array_equal(mbuf[G:G + B * K].reshape(B, K).cpu().numpy(), want)
    _check_nb_codewords(cid, buf[G:G + B * N].reshape(B, N).cpu().numpy(), want, mul, ref)
