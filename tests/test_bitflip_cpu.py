"""CPU tests of hard-decision decoding (include/bldpc.h): the host statement bldpc_decode_bitflip_host against the integer-only numpy
restatement of tests/bitflip_cases.py, exactly, on every shape, batch size, rule and exit mode of that file; the condition on the inputs
that tests/test_bitflip_gpu.py relies on; pack, unpack and the binary symmetric channel against numpy and against a literal loop over the
RandomModule draws; padding; every refusal; the plan on the shipped matrices; the direction of the two rules on a shipped code; and the
host statements as a stand-alone program (tests/cpp/bitflip_host_test.hip) under the address + undefined and the thread sanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from bitflip_cases import (BATCHES, BF_GRADIENT, BF_THRESHOLD, EXIT_BATCH_GLOBAL, EXIT_FIXED, EXIT_PER_FRAME, EXTREME, F_MAX, LDS_BOUND, MAX_ITER,
                           RULES, accepted_dims, bound_shapes, dims_id, garbage_padding, matrix, np_bitflip, np_outputs, np_pack, np_syndrome,
                           np_unpack, ramp_input)
from test_bp_cpu import fnv64
from test_layered_cpu import read_H

LCG_A, LCG_M = (249, 251, 252), (61967, 63443, 63599)


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def _dims():
    return accepted_dims()


_np = {}


def np_case(dims, rule):
    """(D, per-frame iters, x history) of the restatement on the shape's ramp at F_MAX: computed once, the frames of a smaller batch
    are its first columns (frames are independent)."""
    key = (tuple(dims), rule)
    if key not in _np:
        xs, flags = np_bitflip(matrix(dims), dims[2], ramp_input(dims)[0], MAX_ITER, rule)
        _np[key] = np_outputs(xs, flags) + (xs,)
    return _np[key]


def random_module(seed):
    """One draw of the reference's generator, as its source writes it: three LCGs, float32 quotients summed in float32, fraction kept."""
    for i in range(3):
        seed[i] = (seed[i] * LCG_A[i]) % LCG_M[i]
    t = np.float32(seed[0]) / np.float32(LCG_M[0])
    t = np.float32(t + np.float32(seed[1]) / np.float32(LCG_M[1]))
    t = np.float32(t + np.float32(seed[2]) / np.float32(LCG_M[2]))
    return np.float32(t - np.float32(int(t)))


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", _dims(), ids=dims_id)
def test_inputs_meet_their_condition(C, dims):
    """Judged by the host statement alone: under per-frame exit the ramp gives at least three distinct iteration counts, 1 and MAX_ITER
    among them, under both rules; frame 0 is a codeword."""
    J, L, Z = dims
    r, cw = ramp_input(dims)
    assert np.array_equal(r[:, 0], cw[:, 0]) and not np_syndrome(matrix(dims), Z, cw.astype(np.int64)).any()
    for rule in RULES:
        it = C.bitflip_host(matrix(dims), J, L, Z, np_pack(r), F_MAX, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)["iters"]
        u = np.unique(it)
        print("%s rule %d: iters %s" % (dims_id(dims), rule, u.tolist()))
        assert u.size >= 3 and u[0] == 1 and u[-1] == MAX_ITER, (dims, rule, u)


def test_the_extreme_matrix_reaches_the_fifth_plane():
    """Frame 1 of its ramp has one error in the block column of weight 16: all 16 checks of that variable fail, u = 16."""
    J, L, Z = EXTREME
    H = matrix(EXTREME)
    r, cw = ramp_input(EXTREME)
    s = np_syndrome(H, Z, r[:, 1:2].astype(np.int64))
    assert int(s.sum()) == 16 and (r[:, 1] != cw[:, 1]).sum() == 1
    w = (H != -1).sum(0)
    assert w.max() == 16 and 1 in w and 0 in w and 1 in (H != -1).sum(1)


@pytest.mark.parametrize("dims", _dims(), ids=dims_id)
def test_host_equals_numpy(C, dims):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    r = ramp_input(dims)[0]
    for rule in RULES:
        D, want_it, _ = np_case(dims, rule)
        for F in BATCHES:
            bits = np_pack(r[:, :F])
            what = "%s rule %d F %d" % (dims_id(dims), rule, F)
            fx = C.bitflip_host(H, J, L, Z, bits, F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_FIXED)
            pf = C.bitflip_host(H, J, L, Z, bits, F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)
            assert np.array_equal(fx["D"], D[:, :F]), "D: " + what
            assert (fx["iters"] == MAX_ITER).all(), what
            assert np.array_equal(pf["iters"], want_it[:F]), "per-frame iters: " + what
            assert np.array_equal(fx["Dbits"], np_pack(D[:, :F])), "Dbits: " + what
            # both modes return the same D, Dbits and flags
            assert np.array_equal(pf["D"], fx["D"]) and np.array_equal(pf["Dbits"], fx["Dbits"]), what
            assert fx["D"].shape == (N + 1, F) and set(np.unique(fx["D"]).tolist()) <= {0, 1}


def test_fewer_iterations_are_a_prefix_of_the_history(C):
    dims = (3, 9, 96)
    J, L, Z = dims
    for rule in RULES:
        xs = np_case(dims, rule)[2]
        for k in (1, 2, 5):
            got = C.bitflip_host(matrix(dims), J, L, Z, np_pack(ramp_input(dims)[0]), F_MAX, rule=rule, max_iter=k)
            assert np.array_equal(got["D"][:-1], xs[k - 1])


def test_padding_of_the_input_changes_nothing_and_output_padding_is_zero(C):
    dims = (3, 7, 33)
    J, L, Z = dims
    r = ramp_input(dims)[0]
    for F in (1, 33, 37):
        bits = np_pack(r[:, :F])
        dirty = garbage_padding(bits, F)
        assert not np.array_equal(bits, dirty)
        for rule in RULES:
            a = C.bitflip_host(matrix(dims), J, L, Z, bits, F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)
            b = C.bitflip_host(matrix(dims), J, L, Z, dirty, F, rule=rule, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME)
            for k in ("D", "Dbits", "iters"):
                assert np.array_equal(a[k], b[k]), (F, rule, k)
            assert (b["Dbits"][:, -1] >> np.uint32(F % 32)).max() == 0
    assert np.array_equal(C.Hard_Unpack_host(garbage_padding(np_pack(r[:, :37]), 37), 37), r[:, :37])


# ---- pack, unpack, channel --------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_against_numpy(C):
    rng = np.random.default_rng(3)
    for rows, F in ((1, 1), (5, 31), (7, 32), (3, 33), (9, 37), (2, 64), (4, 100)):
        b = rng.integers(0, 2, size=(rows, F)).astype(np.int32)
        want = np_pack(b)
        assert np.array_equal(C.Hard_Pack_Int_host(b * 7), want)
        assert np.array_equal(C.Hard_Pack_host(np.where(b, -1.5, 2.0).astype(np.float32)), want)
        assert np.array_equal(C.Hard_Unpack_host(want, F), b) and np.array_equal(np_unpack(want, F), b)
        assert C.Hard_Unpack_host(want, F).dtype == np.int32


def special_values():
    """float32 [2, 12] and the bits they pack to: the layered decoders' hard-bit rule is y < 0."""
    v = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0], np.float32)
    want = np.array([0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1], np.int32)
    return np.stack([v, v[::-1]]), np.stack([want, want[::-1]])


def test_pack_special_values(C):
    y, want = special_values()
    assert np.array_equal(C.Hard_Pack_host(y), np_pack(want))


def test_bsc_against_a_literal_loop_over_the_draws(C):
    N, F, p = 45, 37, 0.2
    cw = np.random.default_rng(8).integers(0, 2, size=(N, F)).astype(np.int32)
    for word in (None, cw):
        seed = np.array([173, 4711, 99], np.int32)
        s = [int(x) for x in seed]
        want = np.zeros((N, F), np.int32)
        for f in range(F):
            for n in range(N):
                u = random_module(s)
                want[n, f] = (0 if word is None else word[n, f]) ^ int(u < np.float32(p))
        got = C.BSCChannel_CPU(seed, p, N, F, CodeWord=word)
        assert got.dtype == np.uint32 and np.array_equal(got, np_pack(want))
        assert seed.tolist() == s, "the seed advances by N * F draws"
        assert 0 < (want != (0 if word is None else word)).sum() < N * F // 2


def test_bsc_edges_sharding_and_seed_advance(C):
    from cuda_ldpc_amd import sharding
    N, F = 70, 37
    seed = np.array([173, 173, 173], np.int32)
    assert not C.BSCChannel_CPU(seed, 0.0, N, F).any()
    assert seed.tolist() == sharding.lcg_jump([173, 173, 173], N * F).tolist() and sharding.bsc_draws_per_frame(N) == N
    half = np_unpack(C.BSCChannel_CPU(np.array([173, 173, 173], np.int32), 0.5, N, F), F)
    assert 0.4 < half.mean() < 0.6
    full = np_unpack(C.BSCChannel_CPU(np.array([5, 6, 7], np.int32), 0.3, N, F), F)
    for world in (1, 2, 3, 5):
        for rank in range(world):
            first, count = sharding.shard_frames(F, world, rank)
            mine = sharding.lcg_jump([5, 6, 7], first * sharding.bsc_draws_per_frame(N))
            got = np_unpack(C.BSCChannel_CPU(mine, 0.3, N, count), count)
            assert np.array_equal(got, full[:, first:first + count]), (world, rank)
    # two calls in a row are one longer call
    seed = np.array([5, 6, 7], np.int32)
    a = np_unpack(C.BSCChannel_CPU(seed, 0.3, N, 20), 20)
    b = np_unpack(C.BSCChannel_CPU(seed, 0.3, N, 17), 17)
    assert np.array_equal(np.concatenate([a, b], 1), full)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    lib = C._lib.lib
    J, L, Z, F = 4, 24, 96, 2
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    N = L * Z
    bits = np.zeros((N, 1), np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D, Db, it = np.zeros((N + 1, F), np.int32), np.zeros((N + 1, 1), np.uint32), np.zeros(F, np.int32)

    def raw(F=F, max_iter=5, rule=BF_GRADIENT, mode=EXIT_FIXED, bits=bits, D=D, Db=Db, it=it, H=H):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_bitflip_host(J, L, Z, ptr(H), ptr(bits), F, max_iter, rule, mode, ptr(D), ptr(Db), ptr(it))
            out.append((rc, lib.bldpc_last_error().decode()))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_bitflip_host"
    assert raw() == (0, raw()[1])
    assert raw(rule=2) == (-1, who + ": unknown rule 2") and raw(rule=-1)[0] == -1
    assert raw(mode=7) == (-1, who + ": unknown exit_mode 7")
    assert raw(mode=EXIT_BATCH_GLOBAL)[0] == -1 and "BLDPC_EXIT_BATCH_GLOBAL" in raw(mode=EXIT_BATCH_GLOBAL)[1]
    assert raw(max_iter=0) == (-1, who + ": max_iter=0 must be at least 1")
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(F=-3)[0] == -1
    assert raw(bits=None) == (-1, who + ": null bits_in")
    assert raw(D=None, Db=None) == (-1, who + ": D and Dbits are both null")
    assert raw(mode=EXIT_PER_FRAME, it=None) == (-1, who + ": per-frame exit needs iters")
    assert raw(H=None)[0] == -1
    assert raw(D=None)[0] == 0 and raw(Db=None)[0] == 0 and raw(it=None)[0] == 0  # one output is enough; iters is optional in fixed mode
    Hbad = H.copy()
    Hbad[0, 0] = Z
    assert raw(H=Hbad)[0] == -1
    # a block row of weight 1 and an all-zero block column are taken
    H1 = H.copy().reshape(J, L)
    H1[2, 1:] = -1
    H1[2, 0] = 0
    H1[:, 5] = -1
    r = C.bitflip_host(H1.reshape(-1), J, L, Z, bits[:, :1], 1, max_iter=3, exit_mode=EXIT_PER_FRAME)
    assert r["iters"].tolist() == [1] and r["D"][N].tolist() == [1]
    # the Python wrappers
    for bad in (dict(rule=2), dict(max_iter=0), dict(exit_mode=EXIT_BATCH_GLOBAL), dict(exit_mode=9)):
        with pytest.raises(LdpcError, match=r"\(-1\): .*\S"):
            C.bitflip_host(H, J, L, Z, bits, F, **bad)
    with pytest.raises(ValueError):
        C.bitflip_host(H, J, L, Z, bits, 0)
    with pytest.raises(ValueError):
        C.bitflip_host(H, J, L, Z, bits, 33)  # one word per row is not enough for 33 frames
    with pytest.raises(ValueError):
        C.bitflip_host(H[:-1], J, L, Z, bits, F)
    with pytest.raises(ValueError):
        C.bitflip_host(H, J, L, Z, bits.astype(np.float32), F)
    # the channel
    for p in (-0.01, 0.51, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            C.BSCChannel_CPU(np.array([1, 2, 3], np.int32), p, 8, 4)
        seed = np.array([1, 2, 3], np.int32)
        out = np.zeros((8, 1), np.uint32)
        assert lib.bldpc_bsc_channel_host(ptr(seed), ctypes.c_float(p), None, 8, 4, ptr(out)) == -1 and seed.tolist() == [1, 2, 3]
    for bad_seed in ([61967, 1, 1], [1, -1, 1], [1, 1, 63599]):
        with pytest.raises(LdpcError, match=r"\(-1\): .*seed"):
            C.BSCChannel_CPU(np.array(bad_seed, np.int32), 0.1, 8, 4)
    with pytest.raises(ValueError):
        C.BSCChannel_CPU([1, 2, 3], 0.1, 8, 4)
    with pytest.raises(ValueError):
        C.BSCChannel_CPU(np.array([1, 2, 3], np.int32), 0.1, 8, 4, CodeWord=np.zeros((8, 5), np.int32))
    one = np.zeros((1, 1), np.uint32)
    assert lib.bldpc_hard_pack_host(None, 1, 1, ptr(one)) == -1 and lib.bldpc_hard_pack_int_host(ptr(one), 0, 1, ptr(one)) == -1
    assert lib.bldpc_hard_unpack_host(ptr(one), 1, 0, ptr(one)) == -1 and lib.bldpc_bitflip_plan_host(J, L, Z, ptr(H), None) == -1
    with pytest.raises(ValueError):
        C.Hard_Unpack_host(np.zeros((2, 1), np.uint32), 40)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_on_the_shipped_matrices_and_at_the_bound(C):
    pon = C.bitflip_plan_host(read_H("PON_LDPC.txt", 12, 69), 12, 69, 256)
    assert pon["fits"] and pon["frames_per_wg"] == 32 and pon["threads"] % 64 == 0 and 64 <= pon["threads"] <= 1024
    assert pon["lds_bytes"] == 4 * (69 + 12) * 256  # about 82 KB
    big = C.bitflip_plan_host(read_H("J15_L30_Z1280_BlockH.txt", 15, 30), 15, 30, 1280)
    assert not big["fits"] and big["lds_bytes"] == 4 * 45 * 1280  # about 230 KB
    small = C.bitflip_plan_host(read_H("J4_L24_Z96_BlockH.txt", 4, 24), 4, 24, 96)
    assert small["fits"] and small["lds_bytes"] >= 4 * 28 * 96
    fit, beyond = bound_shapes()
    assert C.bitflip_plan_host(matrix(fit), *fit)["lds_bytes"] <= LDS_BOUND < C.bitflip_plan_host(matrix(beyond), *beyond)["lds_bytes"]
    assert C.bitflip_plan_host(matrix(fit), *fit)["fits"] and not C.bitflip_plan_host(matrix(beyond), *beyond)["fits"]
    # the host statement has no such bound
    J, L, Z = beyond
    assert C.bitflip_host(matrix(beyond), J, L, Z, np.zeros((L * Z, 1), np.uint32), 1, max_iter=2)["D"][L * Z].tolist() == [1]


# ---- direction --------------------------------------------------------------------------------------------------------------------------
def test_gradient_descent_beats_the_threshold_rule_on_a_shipped_code(C):
    """J4_L24_Z96, 256 frames of the all-zero word through the BSC at p = 0.004 from seed (173, 173, 173), 30 iterations."""
    J, L, Z, F, p = 4, 24, 96, 256, 0.004
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    bits = C.BSCChannel_CPU(np.array([173, 173, 173], np.int32), p, L * Z, F)
    left = {}
    for rule in RULES:
        r = C.bitflip_host(H, J, L, Z, bits, F, rule=rule, max_iter=30, exit_mode=EXIT_PER_FRAME)
        left[rule] = int((r["D"][L * Z] == 0).sum())
    print("J4_L24_Z96 p=%g, %d frames, 30 iterations: unflagged frames threshold %d, gradient %d" % (p, F, left[BF_THRESHOLD], left[BF_GRADIENT]))
    assert 0 < left[BF_GRADIENT] < left[BF_THRESHOLD] < F


# ---- the host statements under the host sanitizers, stand-alone -----------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def bitflip_exe(request, tmp_path_factory):
    """tests/cpp/bitflip_host_test.hip, built as test_quant_cpu.py builds quant_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("bitflip_host_" + request.param)
    exe = str(tmp / "bitflip_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "bitflip_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("dims", [(3, 5, 13), EXTREME], ids=dims_id)
def test_host_statements_stand_alone(C, bitflip_exe, tmp_path, dims):
    J, L, Z = dims
    H = matrix(dims)
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F, p = 37, 0.03
    rx = C.BSCChannel_CPU(np.array([173, 173, 173], np.int32), p, L * Z, F)
    for mode, rule in ((EXIT_FIXED, BF_THRESHOLD), (EXIT_PER_FRAME, BF_GRADIENT)):
        want = C.bitflip_host(H, J, L, Z, rx, F, rule=rule, max_iter=MAX_ITER, exit_mode=mode)
        if mode == EXIT_PER_FRAME:
            assert np.unique(want["iters"]).size >= 2, "the input must hold frames that stop at different times"
        r = subprocess.run([bitflip_exe, path] + [str(a) for a in (J, L, Z, F, MAX_ITER, mode, rule, p)], timeout=300, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        out = r.stdout.decode()
        assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
        assert "Sanitizer" not in out and "runtime error" not in out, out
        tok = out.strip().split("\n")[-1].split()
        assert int(tok[0], 16) == fnv64(rx, want["D"], want["Dbits"], want["iters"]), "outputs differ from what bitflip_host returned in Python"
        if len(os.sched_getaffinity(0)) > 1:
            assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
