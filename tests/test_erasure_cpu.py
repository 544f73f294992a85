"""CPU tests of erasure decoding (include/bldpc.h): the host statement bldpc_decode_erasure_host against the integer-only numpy
restatement of tests/erasure_cases.py, exactly, on every shape and batch size of that file and all four outputs; the conditions on the
inputs that tests/test_erasure_gpu.py relies on; the binary erasure channel against a literal loop over the RandomModule draws and against
the BSC's flip mask; rate matching and statistics on packed words against numpy; padding; every refusal; the plan on the shipped matrices;
the two sides of the waterfall on a shipped code; and the host statements as a stand-alone program (tests/cpp/erasure_host_test.hip)
under the address + undefined and the thread sanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from erasure_cases import (ALL_ERASED, BATCHES, EXTREME, F_MAX, LDS_BOUND, MAX_ITER, RANDOM_KNOWN, X_COL0, X_COL0_VAR, X_COL16, X_COL16_VAR, X_ROW1,
                           X_ROW1_VAR, accepted_dims, bound_shapes, dims_id, dirty_input, erased_input, garbage_padding, matrix, np_outputs, np_pack,
                           np_peel, np_syndrome, np_unpack, ramp_frames)
from test_bitflip_cpu import random_module
from test_bp_cpu import fnv64
from test_layered_cpu import read_H


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_np = {}


def np_case(dims):
    """The restatement's history on the shape's input at F_MAX: computed once, the frames of a smaller batch are its first columns."""
    dims = tuple(dims)
    if dims not in _np:
        bits, er, _ = erased_input(dims)
        _np[dims] = np_peel(matrix(dims), dims[2], bits, er, MAX_ITER)
    return _np[dims]


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", accepted_dims(), ids=dims_id)
def test_inputs_meet_their_conditions(dims):
    """Judged by the restatement alone.  The ramp: at least three distinct iteration counts, 0 among them, none at the cap, and a frame
    that ends with erasures left after one or more productive iterations.  The fixed frames: what erasure_cases.py says of each.  The
    frame with every position erased has iters 0 wherever every block row has weight two or more; on EXTREME it does not."""
    J, L, Z = dims
    H = matrix(dims)
    bits, er, cw = erased_input(dims)
    D, E, it = np_outputs(H, Z, np_case(dims))
    rf = ramp_frames()
    u = np.unique(it[rf])
    print("%s: iters %s, %d of %d ramp frames flagged" % (dims_id(dims), u.tolist(), int(D[-1, rf].sum()), len(rf)))
    assert u.size >= 3 and u[0] == 0 and u[-1] < MAX_ITER
    assert ((it[rf] > 0) & E[:, rf].any(0)).any(), "no frame is stuck after progress"
    assert not er[:, 0].any() and it[0] == 0 and D[-1, 0] == 1 and not np_syndrome(H, Z, cw[:, rf].astype(np.int64)).any()
    assert er[:, ALL_ERASED].all() and D[-1, ALL_ERASED] == 0
    if (H != -1).sum(1).min() > 1:  # every check sees two erasures or more: nothing starts
        assert it[ALL_ERASED] == 0 and E[:, ALL_ERASED].all()
    else:  # EXTREME: the checks of its weight-1 block row resolve their variable from nothing, and peeling goes on from there
        assert dims == EXTREME and it[ALL_ERASED] > 0 and E[:, ALL_ERASED].any() and not D[:-1, ALL_ERASED].any()
    rk = list(RANDOM_KNOWN)
    split = np_case(dims)["split"][rk]
    print("%s: variables resolved by disagreeing checks in the random-known frames: %s" % (dims_id(dims), split.tolist()))
    assert split.max() > 0, "no frame tests the OR rule"
    assert np_syndrome(H, Z, cw[:, rk].astype(np.int64)).any(0).all() and (it[rk] > 0).all()
    assert not D[-1, rk][~E[:, rk].any(0)].any(), "a word that is no codeword ends with flag 0 even when every erasure is resolved"
    if dims == EXTREME:
        w = (H != -1).sum(0)
        assert w[0] == 16 and w[2] == 0 and (H[16] != -1).sum() == 1 and H[16, 3] != -1
        assert er[:, X_ROW1].sum() == 1 and er[X_ROW1_VAR, X_ROW1] and it[X_ROW1] == 1 and D[-1, X_ROW1] == 1 and D[X_ROW1_VAR, X_ROW1] == 0
        assert er[X_COL0_VAR, X_COL0] and it[X_COL0] == 0 and D[-1, X_COL0] == 0 and E[:, X_COL0].sum() == 1
        assert er[:, X_COL16].sum() == 1 and er[X_COL16_VAR, X_COL16] and it[X_COL16] == 1 and D[-1, X_COL16] == 1
        assert np.array_equal(D[:-1, X_COL16], cw[:, X_COL16])


@pytest.mark.parametrize("dims", accepted_dims(), ids=dims_id)
def test_host_equals_numpy(C, dims):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    bits, er, _ = erased_input(dims)
    D, E, it = np_outputs(H, Z, np_case(dims))
    for F in BATCHES:
        what = "%s F %d" % (dims_id(dims), F)
        r = C.erasure_host(H, J, L, Z, np_pack(bits[:, :F]), np_pack(er[:, :F]), F, max_iter=MAX_ITER)
        assert np.array_equal(r["D"], D[:, :F]), "D: " + what
        assert np.array_equal(r["Dbits"], np_pack(D[:, :F])), "Dbits: " + what
        assert np.array_equal(r["Ebits"], np_pack(E[:, :F])), "Ebits: " + what
        assert np.array_equal(r["iters"], it[:F]), "iters: " + what
        assert r["D"].shape == (N + 1, F) and set(np.unique(r["D"]).tolist()) <= {0, 1}
        assert np.array_equal(np_unpack(r["Dbits"], F), r["D"]), "D is the unpacked Dbits: " + what
        assert not (r["Dbits"][:-1] & r["Ebits"]).any(), "a position still erased holds 0"


def test_fewer_iterations_are_a_prefix_of_the_history(C):
    dims = (6, 12, 500)
    J, L, Z = dims
    H = matrix(dims)
    bits, er, _ = erased_input(dims)
    full = np_outputs(H, Z, np_case(dims))[2]
    assert full.max() > 20
    for k in (1, 2, 5, 20):
        D, E, it = np_outputs(H, Z, np_case(dims), k)
        got = C.erasure_host(H, J, L, Z, np_pack(bits), np_pack(er), F_MAX, max_iter=k)
        assert np.array_equal(got["D"], D) and np.array_equal(got["Ebits"], np_pack(E))
        assert np.array_equal(got["iters"], it) and np.array_equal(it, np.minimum(full, k))


def test_padding_of_the_inputs_changes_nothing_and_output_padding_is_zero(C):
    dims = (3, 7, 33)
    J, L, Z = dims
    bits, er, _ = erased_input(dims)
    for F in (1, 33, 37):
        clean = (np_pack(bits[:, :F]), np_pack(er[:, :F]))
        dirty = dirty_input(dims, F)
        assert not np.array_equal(clean[0], dirty[0]) and not np.array_equal(clean[1], dirty[1])
        a = C.erasure_host(matrix(dims), J, L, Z, clean[0], clean[1], F, max_iter=MAX_ITER)
        b = C.erasure_host(matrix(dims), J, L, Z, dirty[0], dirty[1], F, max_iter=MAX_ITER)
        for k in ("D", "Dbits", "Ebits", "iters"):
            assert np.array_equal(a[k], b[k]), (F, k)
        for k in ("Dbits", "Ebits"):
            assert (b[k][:, -1] >> np.uint32(F % 32)).max() == 0, k


# ---- the channel ------------------------------------------------------------------------------------------------------------------------
def test_bec_against_a_literal_loop_over_the_draws_and_the_bsc(C):
    N, F, p = 45, 37, 0.2
    cw = np.random.default_rng(8).integers(0, 2, size=(N, F)).astype(np.int32)
    for word in (None, cw):
        seed = np.array([173, 4711, 99], np.int32)
        s = [int(x) for x in seed]
        er = np.zeros((N, F), np.int32)
        for f in range(F):
            for n in range(N):
                er[n, f] = int(random_module(s) < np.float32(p))
        bits, erased = C.BECChannel_CPU(seed, p, N, F, CodeWord=word)
        assert bits.dtype == np.uint32 and erased.dtype == np.uint32
        assert np.array_equal(erased, np_pack(er)) and np.array_equal(bits, np_pack((0 if word is None else word) * (1 - er)))
        assert seed.tolist() == s, "the seed advances by N * F draws"
        assert 0 < er.sum() < N * F // 2
        # with the same seed and p the mask is the BSC's flip mask on the all-zero word
        assert np.array_equal(erased, C.BSCChannel_CPU(np.array([173, 4711, 99], np.int32), p, N, F))


def test_bec_edges_sharding_and_seed_advance(C):
    from cuda_ldpc_amd import sharding
    N, F = 70, 37
    cw = np.random.default_rng(9).integers(0, 2, size=(N, F)).astype(np.int32)
    seed = np.array([173, 173, 173], np.int32)
    bits, erased = C.BECChannel_CPU(seed, 0.0, N, F, CodeWord=cw)
    assert not erased.any() and np.array_equal(bits, np_pack(cw))
    assert seed.tolist() == sharding.lcg_jump([173, 173, 173], N * F).tolist() and sharding.bec_draws_per_frame(N) == N
    bits, erased = C.BECChannel_CPU(np.array([173, 173, 173], np.int32), 1.0, N, F, CodeWord=cw)
    assert not bits.any() and np.array_equal(erased, np_pack(np.ones((N, F), np.int32)))
    full = [np_unpack(a, F) for a in C.BECChannel_CPU(np.array([5, 6, 7], np.int32), 0.3, N, F, CodeWord=cw)]
    for world in (1, 2, 3, 5):
        for rank in range(world):
            first, count = sharding.shard_frames(F, world, rank)
            mine = sharding.lcg_jump([5, 6, 7], first * sharding.bec_draws_per_frame(N))
            got = C.BECChannel_CPU(mine, 0.3, N, count, CodeWord=cw[:, first:first + count])
            for a, b in zip(got, full):
                assert np.array_equal(np_unpack(a, count), b[:, first:first + count]), (world, rank)
    seed = np.array([5, 6, 7], np.int32)  # two calls in a row are one longer call
    a = C.BECChannel_CPU(seed, 0.3, N, 20, CodeWord=cw[:, :20])
    b = C.BECChannel_CPU(seed, 0.3, N, 17, CodeWord=cw[:, 20:])
    for k in range(2):
        assert np.array_equal(np.concatenate([np_unpack(a[k], 20), np_unpack(b[k], 17)], 1), full[k])


# ---- rate matching on packed words ------------------------------------------------------------------------------------------------------
def np_recover(rm, rx, rxe, N, F):
    """(bits, erased) [N, F]: every transmitted copy in order, the first unerased one gives the value."""
    known, bits = np.zeros((N, F), bool), np.zeros((N, F), np.int32)
    for e, n in enumerate(rm.tx_pos):
        take = ~known[n] & (rxe[e] == 0)
        bits[n][take] = rx[e][take]
        known[n] |= take
    known[rm.shorten] = True
    return bits, (~known).astype(np.int32)


def rm_profiles(C, N):
    """A linear profile with shortening and puncturing; a circular one with k0 > 0, a wrap and more than one lap (2.5 laps of Ncb)."""
    sh, pu = [0, 3, 17], list(range(N - 9, N - 2))
    ncb = N - len(sh) - len(pu)
    return [C.RateMatch(N, sh, pu), C.RateMatch.circular(N, sh, pu, 7, ncb * 5 // 2), C.RateMatch.circular(N, [], pu, ncb // 2, ncb // 3)]


def test_rate_matching_on_packed_words_against_numpy(C):
    N = 60
    rng = np.random.default_rng(21)
    for rm in rm_profiles(C, N):
        assert rm.E == len(rm.tx_pos)
        for F in (1, 37, 64):
            cw = rng.integers(0, 2, size=(N, F)).astype(np.int32)
            cw[rm.shorten] = 0
            tx = C.RM_Select_Bits_host(rm, garbage_padding(np_pack(cw), F), F)
            assert tx.dtype == np.uint32 and np.array_equal(tx, np_pack(cw[rm.tx_pos]))
            assert np.array_equal(tx, C.Hard_Pack_Int_host(C.RM_Select_host(rm, cw))), "select is pack of the int32 select"
            rxe = (rng.random((rm.E, F)) < 0.4).astype(np.int32)
            rx = cw[rm.tx_pos] * (1 - rxe)
            junk = rng.integers(0, 2, size=rx.shape).astype(np.int32) & rxe  # value bits at erased positions carry no meaning
            for mask in (rxe, None):
                want_b, want_e = np_recover(rm, rx, rxe if mask is not None else np.zeros_like(rxe), N, F)
                got_b, got_e = C.RM_Recover_Bits_host(rm, garbage_padding(np_pack(rx | junk), F), F,
                                                      rx_erased=None if mask is None else garbage_padding(np_pack(mask), F, seed=4))
                if mask is None:  # nothing erased: the junk bits count as received values
                    want_b, want_e = np_recover(rm, rx | junk, np.zeros_like(rxe), N, F)
                assert np.array_equal(got_b, np_pack(want_b)) and np.array_equal(got_e, np_pack(want_e)), (rm.is_circular, F, mask is None)
                assert not want_e[rm.shorten].any() and not want_b[rm.shorten].any() and want_e[rm.puncture].all()
                if mask is not None:
                    assert np.array_equal(want_b, cw * (1 - want_e)), "what is known is the sent bit"
    rm2 = rm_profiles(C, N)[1]
    assert rm2.laps == 3 and rm2.k0 == 7
    # a position sent three times takes its first unerased copy: erase the first copy and corrupt the third
    F = 5
    n = int(rm2.tx_pos[0])
    copies = np.flatnonzero(rm2.tx_pos == n)
    assert copies.size == 3
    rx, rxe = np.zeros((rm2.E, F), np.int32), np.zeros((rm2.E, F), np.int32)
    rxe[copies[0]] = 1
    rx[copies[1]] = [1, 0, 1, 0, 1]
    rx[copies[2]] = 1
    b, e = C.RM_Recover_Bits_host(rm2, np_pack(rx), F, rx_erased=np_pack(rxe))
    assert np_unpack(b, F)[n].tolist() == [1, 0, 1, 0, 1] and not np_unpack(e, F)[n].any()


# ---- statistics on packed words ---------------------------------------------------------------------------------------------------------
def np_counters(D, E, cw, iters, length):
    """The five counters of bldpc_statistic_per_frame on D with every position still erased replaced by the complement of the sent bit."""
    N = D.shape[0] - 1
    cw = np.zeros((N, D.shape[1]), np.int32) if cw is None else cw
    d = D[:N].copy()
    if E is not None:
        d = np.where(E == 1, 1 - cw[:N], d)
    err = (d[:length] != cw[:length]).sum(0)
    flag = D[N]
    it = 0 if iters is None else int(np.asarray(iters).sum())
    return np.array([((err != 0) | (flag == 0)).sum(), err.sum(), it, ((err != 0) & (flag == 1)).sum(), ((err == 0) & (flag == 0)).sum()], np.int64)


def test_statistic_bits_host_against_a_numpy_count(C):
    dims = (3, 9, 96)
    J, L, Z = dims
    N = L * Z
    bits, er, cw = erased_input(dims)
    for F in (1, 37, 64):
        r = C.erasure_host(matrix(dims), J, L, Z, np_pack(bits[:, :F]), np_pack(er[:, :F]), F, max_iter=3)
        E = np_unpack(r["Ebits"], F)
        cwb = np_pack(cw[:, :F])
        for length in (N, N - J * Z, 5):
            for kw in (dict(Ebits=r["Ebits"], CodeWordBits=cwb, iters=r["iters"]), dict(CodeWordBits=cwb, iters=r["iters"]),
                       dict(Ebits=r["Ebits"], iters=r["iters"]), dict(Ebits=r["Ebits"], CodeWordBits=cwb)):
                want = np_counters(r["D"], E if "Ebits" in kw else None, cw[:, :F] if "CodeWordBits" in kw else None, kw.get("iters"), length)
                got = C.Statistic_Bits_host(N, garbage_padding(r["Dbits"], F), F, length, **kw)
                assert got.tolist() == want.tolist(), (F, length, sorted(kw))
        # accumulation, and the frames add up
        acc = C.Statistic_Bits_host(N, r["Dbits"], F, N, Ebits=r["Ebits"], CodeWordBits=cwb, iters=r["iters"])
        twice = C.Statistic_Bits_host(N, r["Dbits"], F, N, Ebits=r["Ebits"], CodeWordBits=cwb, iters=r["iters"], counters=acc.copy())
        assert twice.tolist() == (2 * acc).tolist() and acc[0] + (r["D"][N] == 1).sum() - acc[3] == F
    assert acc[0] > 0 and acc[1] > 0 and acc[2] > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    lib = C._lib.lib
    J, L, Z, F = 4, 24, 96, 2
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    N = L * Z
    bits, er = np.zeros((N, 1), np.uint32), np.zeros((N, 1), np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D, Db, Eb, it = np.zeros((N + 1, F), np.int32), np.zeros((N + 1, 1), np.uint32), np.zeros((N, 1), np.uint32), np.zeros(F, np.int32)

    def raw(F=F, max_iter=5, bits=bits, er=er, D=D, Db=Db, Eb=Eb, it=it, H=H):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_erasure_host(J, L, Z, ptr(H), ptr(bits), ptr(er), F, max_iter, ptr(D), ptr(Db), ptr(Eb), ptr(it))
            out.append((rc, lib.bldpc_last_error().decode()))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_erasure_host"
    assert raw()[0] == 0
    assert raw(max_iter=0) == (-1, who + ": max_iter=0 must be at least 1")
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(F=-3)[0] == -1
    assert raw(bits=None) == (-1, who + ": null bits_in") and raw(er=None) == (-1, who + ": null erased_in")
    assert raw(D=None, Db=None, Eb=None) == (-1, who + ": D, Dbits and Ebits are all null")
    assert raw(H=None)[0] == -1
    for only in ("D", "Db", "Eb"):  # one output is enough; iters is optional
        assert raw(**{k: None for k in ("D", "Db", "Eb", "it") if k != only})[0] == 0, only
    Hbad = H.copy()
    Hbad[0, 0] = Z
    assert raw(H=Hbad)[0] == -1
    # a block row of weight 1 and an all-zero block column are taken
    H1 = H.copy().reshape(J, L)
    H1[2, 1:] = -1
    H1[2, 0] = 0
    H1[:, 5] = -1
    one = np.zeros((N, 1), np.uint32)
    one[5 * Z + 1, 0] = 1  # a position of the all-zero block column
    r = C.erasure_host(H1.reshape(-1), J, L, Z, bits, one, 1, max_iter=3)
    assert r["iters"].tolist() == [0] and r["D"][N].tolist() == [0] and np.array_equal(r["Ebits"], one)
    # the Python wrappers
    with pytest.raises(LdpcError, match=r"\(-1\): .*max_iter"):
        C.erasure_host(H, J, L, Z, bits, er, F, max_iter=0)
    for bad in (dict(F=0), dict(F=33), dict(H=H[:-1]), dict(bits=bits.astype(np.float32)), dict(er=np.zeros((N - 1, 1), np.uint32))):
        kw = dict(dict(H=H, bits=bits, er=er, F=F), **bad)
        with pytest.raises(ValueError):
            C.erasure_host(kw["H"], J, L, Z, kw["bits"], kw["er"], kw["F"])
    # the channel: p in [0, 1], the seed checks of the BSC
    for p in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            C.BECChannel_CPU(np.array([1, 2, 3], np.int32), p, 8, 4)
        seed = np.array([1, 2, 3], np.int32)
        a, b = np.zeros((8, 1), np.uint32), np.zeros((8, 1), np.uint32)
        assert lib.bldpc_bec_channel_host(ptr(seed), ctypes.c_float(p), None, 8, 4, ptr(a), ptr(b)) == -1 and seed.tolist() == [1, 2, 3]
    C.BECChannel_CPU(np.array([1, 2, 3], np.int32), 0.75, 8, 4)  # above the BSC's 0.5
    for bad_seed in ([61967, 1, 1], [1, -1, 1], [1, 1, 63599]):
        with pytest.raises(LdpcError, match=r"\(-1\): .*seed"):
            C.BECChannel_CPU(np.array(bad_seed, np.int32), 0.1, 8, 4)
    with pytest.raises(ValueError):
        C.BECChannel_CPU([1, 2, 3], 0.1, 8, 4)
    with pytest.raises(ValueError):
        C.BECChannel_CPU(np.array([1, 2, 3], np.int32), 0.1, 8, 4, CodeWord=np.zeros((8, 5), np.int32))
    a = np.zeros((8, 1), np.uint32)
    seed = np.array([1, 2, 3], np.int32)
    assert lib.bldpc_bec_channel_host(ptr(seed), ctypes.c_float(0.1), None, 8, 4, ptr(a), None) == -1
    assert lib.bldpc_bec_channel_host(ptr(seed), ctypes.c_float(0.1), None, 8, 4, None, ptr(a)) == -1
    assert lib.bldpc_erasure_plan_host(J, L, Z, ptr(H), None) == -1
    # rate matching and statistics
    rm = C.RateMatch(8, [0], [7])
    tx, w8 = np.zeros((rm.E, 1), np.uint32), np.zeros((8, 1), np.uint32)
    assert lib.bldpc_rm_select_bits_host(None, ptr(w8), 4, ptr(tx)) == -1 and lib.bldpc_rm_select_bits_host(rm._h, None, 4, ptr(tx)) == -1
    assert lib.bldpc_rm_select_bits_host(rm._h, ptr(w8), 0, ptr(tx)) == -1 and lib.bldpc_rm_select_bits_host(rm._h, ptr(w8), 4, None) == -1
    assert lib.bldpc_rm_recover_bits_host(rm._h, None, None, 4, ptr(w8), ptr(w8)) == -1
    assert lib.bldpc_rm_recover_bits_host(rm._h, ptr(tx), None, 4, None, ptr(w8)) == -1
    assert lib.bldpc_rm_recover_bits_host(rm._h, ptr(tx), None, 4, ptr(w8), None) == -1
    assert lib.bldpc_rm_recover_bits_host(rm._h, ptr(tx), None, 4, ptr(w8), ptr(w8.copy())) == 0
    with pytest.raises(ValueError):
        C.RM_Select_Bits_host(rm, np.zeros((7, 1), np.uint32), 4)
    with pytest.raises(ValueError):
        C.RM_Recover_Bits_host(rm, tx, 4, rx_erased=np.zeros((rm.E, 2), np.uint32))
    cnt = np.zeros(5, np.int64)
    d9 = np.zeros((9, 1), np.uint32)
    for bad in (dict(N=0), dict(F=0), dict(length=0), dict(length=9), dict(D=None), dict(cnt=None)):
        kw = dict(dict(N=8, F=4, length=8, D=d9, cnt=cnt), **bad)
        assert lib.bldpc_statistic_bits_host(kw["N"], ptr(kw["D"]), None, None, kw["F"], kw["length"], None, ptr(kw["cnt"])) == -1, bad
    assert not cnt.any()
    with pytest.raises(ValueError):
        C.Statistic_Bits_host(8, np.zeros((8, 1), np.uint32), 4, 8)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_on_the_shipped_matrices_and_at_the_bound(C):
    pon = C.erasure_plan_host(read_H("PON_LDPC.txt", 12, 69), 12, 69, 256)
    assert pon["fits"] and pon["frames_per_wg"] == 32 and pon["threads"] % 64 == 0 and 64 <= pon["threads"] <= 1024
    assert pon["lds_bytes"] == 153600 == 4 * (2 * 69 + 12) * 256
    big = C.erasure_plan_host(read_H("J15_L30_Z1280_BlockH.txt", 15, 30), 15, 30, 1280)
    assert not big["fits"] and big["lds_bytes"] == 4 * 75 * 1280
    small = C.erasure_plan_host(read_H("J4_L24_Z96_BlockH.txt", 4, 24), 4, 24, 96)
    assert small["fits"] and small["lds_bytes"] == 4 * 52 * 96
    fit, beyond = bound_shapes()
    assert C.erasure_plan_host(matrix(fit), *fit)["lds_bytes"] <= LDS_BOUND < C.erasure_plan_host(matrix(beyond), *beyond)["lds_bytes"]
    assert C.erasure_plan_host(matrix(fit), *fit)["fits"] and not C.erasure_plan_host(matrix(beyond), *beyond)["fits"]
    # the host statement has no such bound
    J, L, Z = beyond
    z = np.zeros((L * Z, 1), np.uint32)
    assert C.erasure_host(matrix(beyond), J, L, Z, z, z, 1, max_iter=2)["D"][L * Z].tolist() == [1]


# ---- direction --------------------------------------------------------------------------------------------------------------------------
WATERFALL = {0.10: 0, 0.14: 151}  # frames left unrecovered of 256, by the restatement on the project's stream (seed 173, 173, 173)


def test_both_sides_of_the_waterfall_on_a_shipped_code(C):
    """J4_L24_Z96, 256 all-zero frames through BECChannel_CPU from seed (173, 173, 173), 100 iterations: the host statement is held to
    the counts the restatement gives, and the restatement is run again here."""
    J, L, Z, F = 4, 24, 96, 256
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    left = {}
    for p, want in WATERFALL.items():
        bits, erased = C.BECChannel_CPU(np.array([173, 173, 173], np.int32), p, L * Z, F)
        r = C.erasure_host(H, J, L, Z, bits, erased, F, max_iter=100)
        h = np_peel(np.asarray(H).reshape(J, L), Z, np_unpack(bits, F), np_unpack(erased, F), 100)
        D, E, it = np_outputs(np.asarray(H).reshape(J, L), Z, h)
        left[p] = int((r["D"][L * Z] == 0).sum())
        print("J4_L24_Z96 p=%g: %d of %d frames unrecovered, iterations up to %d" % (p, left[p], F, int(r["iters"].max())))
        assert int((D[-1] == 0).sum()) == want, "the restatement's count"
        assert left[p] == want and np.array_equal(r["D"], D) and np.array_equal(r["iters"], it)
        assert np.array_equal(r["D"][L * Z] == 0, np_unpack(r["Ebits"], F).any(0)), "on the all-zero word a frame fails by erasures alone"
    assert left[0.10] < F // 8 and left[0.14] > F // 2


# ---- the host statements under the host sanitizers, stand-alone -----------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def erasure_exe(request, tmp_path_factory):
    """tests/cpp/erasure_host_test.hip, built as test_bitflip_cpu.py builds bitflip_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("erasure_host_" + request.param)
    exe = str(tmp / "erasure_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "erasure_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("dims,p", [((3, 5, 13), 0.3), (EXTREME, 0.05)], ids=lambda v: dims_id(v) if isinstance(v, tuple) else str(v))
def test_host_statements_stand_alone(C, erasure_exe, tmp_path, dims, p):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F = 37
    rx, rxe = C.BECChannel_CPU(np.array([173, 173, 173], np.int32), p, N, F)
    want = C.erasure_host(H, J, L, Z, rx, rxe, F, max_iter=MAX_ITER)
    assert np.unique(want["iters"]).size >= 2, "the input must hold frames that stop at different times"
    cnt = C.Statistic_Bits_host(N, want["Dbits"], F, N, Ebits=want["Ebits"], iters=want["iters"])
    r = subprocess.run([erasure_exe, path] + [str(a) for a in (J, L, Z, F, MAX_ITER, p)], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
    assert "Sanitizer" not in out and "runtime error" not in out, out
    tok = out.strip().split("\n")[-1].split()
    assert int(tok[0], 16) == fnv64(rx, rxe, want["D"], want["Dbits"], want["Ebits"], want["iters"], cnt), \
        "outputs differ from what the host statements returned in Python"
    if len(os.sched_getaffinity(0)) > 1:
        assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
