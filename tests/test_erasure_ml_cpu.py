"""CPU tests of erasure decoding by elimination (include/bldpc.h): the host statement bldpc_decode_erasure_ml_host against the restatement
of tests/erasure_ml_cases.py (Python integers as rows, determined unknowns through a null-space basis), exactly, on every shape, batch
size and max_erased of that file and all five outputs; the case table of the inputs that tests/test_erasure_ml_gpu.py relies on; that
the call contains peeling; padding and garbage; every refusal; the plan on the shipped matrices; what elimination adds to peeling on a
shipped code; and the host statement as a stand-alone program (tests/cpp/erasure_ml_host_test.hip) under the address + undefined and
the thread sanitizer."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from erasure_ml_cases import (ALL_ERASED, BATCHES, COUNTED, DIMS, EXTREME, F_MAX, HEAVY, ML_INCONSISTENT, ML_NONE, ML_PARTIAL, ML_SKIPPED, ML_SOLVED,
                              ML_STUCK, PARTIAL_XOR, RANDOM_KNOWN, WORKSPACE_DIMS, X_COL0, X_COL0_VAR, dims_id, matrix, max_erased_values,
                              ml_dirty_input, ml_input, np_ml_all, np_outputs, np_pack, np_syndrome, np_unpack, partial_outside, row_variables,
                              solve_frame, xor_support)
from test_bp_cpu import fnv64
from test_layered_cpu import read_H

LDS_BOUND = 160 * 1024 - 1024


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def rank_gf2(H, Z):
    """The rank of the expanded matrix, on Python integers."""
    basis = {}
    for vs in row_variables(H, Z):
        row = sum(1 << int(v) for v in vs)
        while row:
            low = (row & -row).bit_length() - 1
            if low not in basis:
                basis[low] = row
                break
            row ^= basis[low]
    return len(basis)


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_inputs_meet_their_conditions(dims):
    """The case table, judged by the restatement alone."""
    J, L, Z = dims
    N, M = L * Z, J * Z
    H = matrix(dims)
    bits, er, cw = ml_input(dims)
    a = np_ml_all(dims)
    e = a["e"]
    seen = set()
    for me in max_erased_values(dims):
        D, E, st, rk = np_outputs(dims, F_MAX, me)
        seen |= set(st.tolist())
        bound = me if me else M
        assert ((e > bound) == (st == ML_SKIPPED)).all() and ((rk == -1) == (st == ML_SKIPPED)).all()
        assert ((e == 0) == (st == ML_NONE)).all()
        if me in (31, 32, 33):  # a frame at the bound is taken, one above is not: the right-hand-side bit moves into a new word here
            at, over = [f for f, k in COUNTED.items() if k == me], [f for f, k in COUNTED.items() if k == me + 1]
            assert len(at) == 1 and len(over) == 1 and e[at[0]] == me and e[over[0]] == me + 1
            assert st[at[0]] not in (ML_SKIPPED, ML_NONE) and st[over[0]] == ML_SKIPPED
        assert not (D[:-1] & E).any() and not D[-1][E.any(0)].any()
    print("%s: statuses at max_erased = N %s" % (dims_id(dims), np.bincount(a["status"], minlength=6).tolist()))
    assert seen == {0, 1, 2, 3, 4, 5}, "every status value"
    known = [f for f in range(F_MAX) if f not in RANDOM_KNOWN]
    assert not np_syndrome(H, Z, cw[:, known].astype(np.int64)).any(), "the known bits of these frames come from a codeword"
    assert (a["status"][known] != ML_INCONSISTENT).all()
    assert (a["status"][list(RANDOM_KNOWN)] == ML_INCONSISTENT).all()
    # the frame with everything erased: skipped by default; with no bound nothing is determined unless a row has weight 1 (EXTREME)
    assert e[ALL_ERASED] == N and np_outputs(dims, F_MAX, 0)[2][ALL_ERASED] == ML_SKIPPED
    assert a["rank"][ALL_ERASED] == rank_gf2(H, Z)
    assert a["status"][ALL_ERASED] == (ML_PARTIAL if dims == EXTREME else ML_STUCK)
    # the support of the XOR of two codewords stays erased, what was erased outside it resolves
    sup, out = xor_support(dims)[0], partial_outside(dims)
    assert sup.size and out.size and not np.isin(out, sup).any() and e[PARTIAL_XOR] == sup.size + out.size
    assert a["status"][PARTIAL_XOR] == ML_PARTIAL and a["er"][sup, PARTIAL_XOR].all() and a["er"][:, PARTIAL_XOR].sum() == sup.size
    assert np.array_equal(a["x"][out, PARTIAL_XOR], cw[out, PARTIAL_XOR])
    if dims == EXTREME:  # a position of the weight-0 block column is in no equation
        assert e[X_COL0] == 1 and a["status"][X_COL0] == ML_STUCK and a["rank"][X_COL0] == 0 and a["er"][X_COL0_VAR, X_COL0] == 1
        assert a["er"][2 * Z:3 * Z, ALL_ERASED].all(), "never determined"
    if dims == WORKSPACE_DIMS:
        assert [int(e[f]) for f in HEAVY] == list(HEAVY.values()) and {ML_SOLVED, ML_PARTIAL} <= set(a["status"][list(HEAVY)].tolist())
    # what is determined agrees with the word sent
    ok = a["er"][:, known] == 0
    assert np.array_equal(a["x"][:, known][ok], cw[:, known][ok])


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_host_equals_restatement(C, dims):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    bits, er, _ = ml_input(dims)
    for me in max_erased_values(dims):
        for F in BATCHES:
            what = "%s F %d max_erased %d" % (dims_id(dims), F, me)
            D, E, st, rk = np_outputs(dims, F, me)
            r = C.erasure_ml_host(H, J, L, Z, np_pack(bits[:, :F]), np_pack(er[:, :F]), F, max_erased=me)
            assert np.array_equal(r["status"], st), "status: " + what
            assert np.array_equal(r["rank"], rk), "rank: " + what
            assert np.array_equal(r["D"], D), "D: " + what
            assert np.array_equal(r["Dbits"], np_pack(D)), "Dbits: " + what
            assert np.array_equal(r["Ebits"], np_pack(E)), "Ebits: " + what
            assert r["D"].shape == (N + 1, F) and np.array_equal(np_unpack(r["Dbits"], F), r["D"])


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_the_call_contains_peeling(C, dims):
    """On consistent inputs ml(input) == ml(peel(input)), and every position peeling resolves, ml resolves with the same value."""
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    bits, er, _ = ml_input(dims)
    keep = [f for f in range(F_MAX) if f not in RANDOM_KNOWN]
    F = len(keep)
    b, e = np_pack(bits[:, keep]), np_pack(er[:, keep])
    peel = C.erasure_host(H, J, L, Z, b, e, F, max_iter=200)
    assert (peel["iters"] < 200).all()
    direct = C.erasure_ml_host(H, J, L, Z, b, e, F, max_erased=N)
    after = C.erasure_ml_host(H, J, L, Z, peel["Dbits"][:N], peel["Ebits"], F, max_erased=N)
    for k in ("D", "Dbits", "Ebits"):
        assert np.array_equal(direct[k], after[k]), k
    assert not (direct["Ebits"] & ~peel["Ebits"]).any(), "never less than peeling"
    assert np.array_equal(direct["Dbits"][:N] & ~peel["Ebits"], peel["Dbits"][:N]), "with the same values"
    if dims != EXTREME:  # whose ramp is light: peeling resolves all that can be resolved there
        assert (peel["Ebits"] & ~direct["Ebits"]).any(), "and more, on some frame"


def test_padding_and_garbage_change_nothing_and_output_padding_is_zero(C):
    dims = (3, 7, 33)
    J, L, Z = dims
    bits, er, _ = ml_input(dims)
    for F in (1, 33, 37):
        clean = (np_pack(bits[:, :F]), np_pack(er[:, :F]))
        dirty = ml_dirty_input(dims, F)
        assert not np.array_equal(clean[0], dirty[0]) and not np.array_equal(clean[1], dirty[1])
        a = C.erasure_ml_host(matrix(dims), J, L, Z, clean[0], clean[1], F, max_erased=L * Z)
        b = C.erasure_ml_host(matrix(dims), J, L, Z, dirty[0], dirty[1], F, max_erased=L * Z)
        for k in ("D", "Dbits", "Ebits", "status", "rank"):
            assert np.array_equal(a[k], b[k]), (F, k)
        for k in ("Dbits", "Ebits"):
            assert (b[k][:, -1] >> np.uint32(F % 32)).max() == 0, k


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    lib = C._lib.lib
    J, L, Z, F = 4, 24, 96, 2
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    N = L * Z
    bits, er = np.zeros((N, 1), np.uint32), np.zeros((N, 1), np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D, Db, Eb = np.zeros((N + 1, F), np.int32), np.zeros((N + 1, 1), np.uint32), np.zeros((N, 1), np.uint32)
    st, rk = np.zeros(F, np.int32), np.zeros(F, np.int32)

    def raw(F=F, me=0, bits=bits, er=er, D=D, Db=Db, Eb=Eb, st=st, rk=rk, H=H):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_erasure_ml_host(J, L, Z, ptr(H), ptr(bits), ptr(er), F, me, ptr(D), ptr(Db), ptr(Eb), ptr(st), ptr(rk))
            out.append((rc, lib.bldpc_last_error().decode()))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_erasure_ml_host"
    assert raw()[0] == 0 and raw(me=1)[0] == 0 and raw(me=N)[0] == 0
    assert raw(me=-1) == (-1, who + ": max_erased=-1 outside [0,%d]" % N) and raw(me=N + 1) == (-1, who + ": max_erased=%d outside [0,%d]" % (N + 1, N))
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(F=-3)[0] == -1
    assert raw(bits=None) == (-1, who + ": null bits_in") and raw(er=None) == (-1, who + ": null erased_in")
    assert raw(D=None, Db=None, Eb=None) == (-1, who + ": D, Dbits and Ebits are all null")
    assert raw(H=None)[0] == -1
    for only in ("D", "Db", "Eb"):  # one output is enough; status and rank are optional
        assert raw(**{k: None for k in ("D", "Db", "Eb", "st", "rk") if k != only})[0] == 0, only
    Hbad = H.copy()
    Hbad[0, 0] = Z
    assert raw(H=Hbad)[0] == -1
    with pytest.raises(LdpcError, match=r"\(-1\): .*max_erased"):
        C.erasure_ml_host(H, J, L, Z, bits, er, F, max_erased=N + 1)
    for bad in (dict(F=0), dict(F=33), dict(H=H[:-1]), dict(bits=bits.astype(np.float32)), dict(er=np.zeros((N - 1, 1), np.uint32))):
        kw = dict(dict(H=H, bits=bits, er=er, F=F), **bad)
        with pytest.raises(ValueError):
            C.erasure_ml_host(kw["H"], J, L, Z, kw["bits"], kw["er"], kw["F"])
    # the plan
    info = np.zeros(4, np.int32)
    H32 = read_H("J32_L64_Z64_BlockH.txt", 32, 64)

    def plan(me=0, tier=0, info=info, H=H32):
        out = []
        for _ in range(2):
            rc = lib.bldpc_erasure_ml_plan_host(32, 64, 64, ptr(H), me, tier, ptr(info))
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_erasure_ml_plan_host"
    assert plan() == (0, "") and plan(info=None)[0] == -1 and plan(H=None)[0] == -1
    assert plan(tier=3) == (-1, who + ": unknown tier 3") and plan(tier=-1)[0] == -1
    assert plan(me=-1)[0] == -1 and plan(me=4097) == (-1, who + ": max_erased=4097 outside [0,4096]")
    rc, text = plan(tier=1)  # decided per call: it depends on max_erased
    assert rc == -5 and "BLDPC_ML_LDS" in text and "532480" in text and info[2] == -1
    assert plan(me=31, tier=1) == (0, "") and info[2] == 1
    with pytest.raises(ValueError):
        C.erasure_ml_plan_host(H, J, L, Z, tier="fast")
    with pytest.raises(LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS"):
        C.erasure_ml_plan_host(H32, 32, 64, 64, tier="lds")


def test_sweep_refuses_ml_without_erasure():
    """Before any device is opened."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra, word in ((["--ml"], "--erasure"), (["--ml-max-erased", "5"], "--erasure"), (["--erasure", "--bec", "0.1", "--ml-max-erased", "5"], "--ml")):
        r = subprocess.run([sys.executable, os.path.join(root, "sweep.py"), "binary"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, extra


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_on_the_shipped_matrices(C):
    from cuda_ldpc_amd._lib import LdpcError
    small = C.erasure_ml_plan_host(read_H("J4_L24_Z96_BlockH.txt", 4, 24), 4, 24, 96)
    assert small == dict(matrix_bytes=19968, threads=384, tier="lds", slots=0)
    assert C.erasure_ml_plan_host(read_H("J4_L24_Z96_BlockH.txt", 4, 24), 4, 24, 96, tier="workspace") == dict(matrix_bytes=19968, threads=384,
                                                                                                                 tier="workspace", slots=256)
    H32 = read_H("J32_L64_Z64_BlockH.txt", 32, 64)
    assert C.erasure_ml_plan_host(H32, 32, 64, 64) == dict(matrix_bytes=532480, threads=1024, tier="workspace", slots=256)
    assert C.erasure_ml_plan_host(H32, 32, 64, 64, max_erased=31)["tier"] == "lds"
    pon = C.erasure_ml_plan_host(read_H("PON_LDPC.txt", 12, 69), 12, 69, 256)
    assert pon == dict(matrix_bytes=1191936, threads=1024, tier="workspace", slots=256)
    for H, dims in ((H32, (32, 64, 64)), (read_H("PON_LDPC.txt", 12, 69), (12, 69, 256))):
        with pytest.raises(LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS"):
            C.erasure_ml_plan_host(H, *dims, tier="lds")
    # the largest max_erased whose matrix, bitmaps and list fit, on the shape of the workspace tests; J4_L24_Z96 fits at every max_erased
    assert C.erasure_ml_plan_host(read_H("J4_L24_Z96_BlockH.txt", 4, 24), 4, 24, 96, max_erased=4 * 24 * 96 // 4, tier="lds")["tier"] == "lds"
    J, L, Z = WORKSPACE_DIMS
    H = matrix(WORKSPACE_DIMS)
    fits = lambda me: 4 * J * Z * (me // 32 + 1) + 8 * ((L * Z + 31) // 32) + 4 * me <= LDS_BOUND  # noqa: E731
    me = max(m for m in range(1, L * Z + 1) if fits(m))
    assert me == 415 and C.erasure_ml_plan_host(H, J, L, Z, max_erased=me, tier="lds")["tier"] == "lds"
    assert C.erasure_ml_plan_host(H, J, L, Z, max_erased=me)["tier"] == "lds"
    assert C.erasure_ml_plan_host(H, J, L, Z, max_erased=me + 1)["tier"] == "workspace"
    with pytest.raises(LdpcError):
        C.erasure_ml_plan_host(H, J, L, Z, max_erased=me + 1, tier="lds")
    assert C.erasure_ml_plan_host(H, J, L, Z) == dict(matrix_bytes=1128000, threads=1024, tier="workspace", slots=256)
    # slots: what fits in 1 GiB
    big = C.erasure_ml_plan_host(read_H("J15_L30_Z1280_BlockH.txt", 15, 30), 15, 30, 1280)
    assert big["matrix_bytes"] == 4 * 19200 * 601 and big["slots"] == (1 << 30) // big["matrix_bytes"] == 23


# ---- direction --------------------------------------------------------------------------------------------------------------------------
PEELING = {0.14: 151, 0.16: 256}  # frames peeling leaves of 256 (test_erasure_cpu.py WATERFALL at 0.14)
LEFT_ML = {0.14: 4, 0.16: 117}    # frames left after elimination, by the restatement on the project's stream (seed 173, 173, 173)


def test_elimination_moves_the_cliff_of_a_shipped_code(C):
    """J4_L24_Z96, 256 all-zero frames through BECChannel_CPU from seed (173, 173, 173), peeling with 100 iterations, then elimination:
    the host statement is held to the counts the restatement gives, and the restatement is run again here.  At p = 0.14 peeling leaves
    151 frames and elimination 4; at 0.16, just under the capacity of 1/6, peeling leaves all 256 and elimination 117."""
    J, L, Z, F = 4, 24, 96, 256
    N = L * Z
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    rows_v = row_variables(np.asarray(H).reshape(J, L), Z)
    left = {}
    for p, want in LEFT_ML.items():
        bits, erased = C.BECChannel_CPU(np.array([173, 173, 173], np.int32), p, N, F)
        peel = C.erasure_host(H, J, L, Z, bits, erased, F, max_iter=100)
        assert int((peel["D"][N] == 0).sum()) == PEELING[p]
        r = C.erasure_ml_host(H, J, L, Z, peel["Dbits"][:N], peel["Ebits"], F)
        x, er = np_unpack(peel["Dbits"][:N], F).astype(np.int64), np_unpack(peel["Ebits"], F).astype(np.int64)
        status = np.zeros(F, np.int32)
        for f in range(F):
            status[f], _, pos, vals = solve_frame(rows_v, x[:, f], er[:, f])
            er[pos, f] = 0
            assert not any(vals)
        left[p] = int((r["D"][N] == 0).sum())
        print("J4_L24_Z96 p=%g: peeling leaves %d of %d frames, elimination %d; statuses %s" % (p, PEELING[p], F, left[p],
                                                                                             np.bincount(r["status"], minlength=6).tolist()))
        assert int(er.any(0).sum()) == want, "the restatement's count"
        assert left[p] == want and np.array_equal(r["status"], status) and np.array_equal(np_unpack(r["Ebits"], F), er)
        assert not r["Dbits"][:N].any() and (r["status"] != ML_SKIPPED).all()
    assert 4 * left[0.14] < PEELING[0.14]


# ---- the host statement under the host sanitizers, stand-alone -------------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def erasure_ml_exe(request, tmp_path_factory):
    """tests/cpp/erasure_ml_host_test.hip, built as test_erasure_cpu.py builds erasure_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("erasure_ml_host_" + request.param)
    exe = str(tmp / "erasure_ml_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "erasure_ml_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("dims,p,me", [((3, 5, 13), 0.45, 0), ((3, 7, 33), 0.4, 90), (EXTREME, 0.05, 0)],
                         ids=lambda v: dims_id(v) if isinstance(v, tuple) else str(v))
def test_host_statement_stand_alone(C, erasure_ml_exe, tmp_path, dims, p, me):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F = 37
    rx, rxe = C.BECChannel_CPU(np.array([173, 173, 173], np.int32), p, N, F)
    want = C.erasure_ml_host(H, J, L, Z, rx, rxe, F, max_erased=me)
    assert np.unique(want["status"]).size >= 2, "the input must hold frames that end differently"
    r = subprocess.run([erasure_ml_exe, path] + [str(a) for a in (J, L, Z, F, me, p)], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
    assert "Sanitizer" not in out and "runtime error" not in out, out
    tok = out.strip().split("\n")[-1].split()
    assert int(tok[0], 16) == fnv64(rx, rxe, want["D"], want["Dbits"], want["Ebits"], want["status"], want["rank"]), \
        "outputs differ from what the host statement returned in Python"
    if len(os.sched_getaffinity(0)) > 1:
        assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
