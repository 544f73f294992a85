"""CPU tests of ordered-statistics reprocessing (include/bldpc.h): the host statement bldpc_decode_osd_host against the restatement of
tests/osd_cases.py (the columns of H as Python integers, a greedy walk that reduces each column against the basis so far, then a solve),
exactly, on every shape and batch size of that file, with D_in NULL and with about half the frames kept; that every processed frame is
a codeword and keeps the hard decisions outside the basis; that the fixed frames of the inputs do what they are for; every refusal; the
plan of every case and on the shipped matrices; what reprocessing does after ten iterations of layered min-sum on a shipped code; and
the host statement as a stand-alone program (tests/cpp/osd_host_test.hip) under the address + undefined and the thread sanitizer."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from osd_cases import (ALL_PLUS_ZERO, BATCHES, CODEWORD, DEFICIENT, DIMS, EXTREME, F_MAX, FIXED, INF_AND_BIG, MIXED_ZEROS, RELIABLE_WRONG, SMALL_INTS,
                       WORKSPACE_DIMS, WORKSPACE_PROCESSED, dims_id, kept_input, matrix, np_osd_all, np_outputs, np_syndrome, osd_input,
                       processed_on_workspace, reliable_wrong_position)
from test_bp_cpu import fnv64
from test_erasure_ml_cpu import rank_gf2
from test_layered_cpu import read_H

LDS_BOUND = 160 * 1024 - 1024


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def _frames(dims):
    return processed_on_workspace() if dims == WORKSPACE_DIMS else list(range(F_MAX))


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_inputs_meet_their_conditions(dims):
    """What the fixed frames are for, judged by the restatement alone; and what the definition promises of every processed frame."""
    J, L, Z = dims
    N, M = L * Z, J * Z
    H = matrix(dims)
    app, cw = osd_input(dims)
    a = np_osd_all(dims)
    rank = rank_gf2(H, Z)
    assert (rank < M) == (dims == DEFICIENT), "one shape is rank deficient"
    frames = _frames(dims)
    assert not np_syndrome(H, Z, cw.astype(np.int64)).any(), "the words sent are codewords"
    y = (app < 0).astype(np.int64)
    c = a["c"][:, frames].astype(np.int64)
    assert not np_syndrome(H, Z, c).any(), "every processed frame is a codeword"
    for k, f in enumerate(frames):
        B = a["B"][f]
        assert len(B) == len(set(B)) == rank and rank <= a["scanned"][f] <= N, "|B| = rank(H), scanned >= rank"
        out = np.setdiff1d(np.arange(N), B)
        assert np.array_equal(c[out, k], y[out, f]), "outside B the hard decisions stay"
        assert a["flips"][f] == (c[:, k] != y[:, f]).sum()
    keys = np.ascontiguousarray(app).view(np.uint32) & np.uint32(0x7FFFFFFF)
    assert a["flips"][CODEWORD] == 0 and np.array_equal(y[:, CODEWORD], cw[:, CODEWORD])
    for f in (ALL_PLUS_ZERO, MIXED_ZEROS):  # every key 0: the order is the positions, y = 0, and -0.0 decides 0
        assert not keys[:, f].any() and not y[:, f].any() and a["flips"][f] == 0 and not a["c"][:, f].any()
    assert not np.signbit(app[:, ALL_PLUS_ZERO]).any() and 0 < np.signbit(app[:, MIXED_ZEROS]).sum() < N
    assert a["scanned"][ALL_PLUS_ZERO] == a["scanned"][MIXED_ZEROS] and a["B"][ALL_PLUS_ZERO] == a["B"][MIXED_ZEROS]
    assert a["B"][ALL_PLUS_ZERO] == sorted(a["B"][ALL_PLUS_ZERO]), "ties go to the lower position"
    assert np.unique(keys[:, SMALL_INTS]).size <= 4 and y[:, SMALL_INTS].any(), "nearly every key ties"
    assert np.isinf(app[:, INF_AND_BIG]).any() and (np.abs(app[:, INF_AND_BIG]) == 1.0e4).any() and a["flips"][INF_AND_BIG] > 0
    v = reliable_wrong_position(dims)
    assert v not in a["B"][RELIABLE_WRONG] and y[v, RELIABLE_WRONG] != cw[v, RELIABLE_WRONG]
    assert not np.array_equal(a["c"][:, RELIABLE_WRONG], cw[:, RELIABLE_WRONG]), "a codeword other than the one sent"
    ramp = [f for f in frames if f not in FIXED]
    assert any(np.array_equal(a["c"][:, f], cw[:, f]) for f in ramp) and any(a["flips"][f] > 0 for f in ramp)
    if dims == EXTREME:  # a position of the weight-0 block column never joins
        assert not any(2 * Z <= p < 3 * Z for f in frames for p in a["B"][f])
    if dims == WORKSPACE_DIMS:
        assert len(frames) == WORKSPACE_PROCESSED
    for F in BATCHES:
        kept = kept_input(dims, F)[N] != 0
        assert (~kept).sum() >= 1 and (F == 1 or kept.sum() >= 1)
        if dims == WORKSPACE_DIMS:
            assert (~kept).sum() <= WORKSPACE_PROCESSED
        else:
            assert F < 33 or abs(int(kept.sum()) - F // 2) <= F // 4, "about half the frames kept"
    print("%s: rank %d of %d rows, scanned %d .. %d, flips up to %d" % (dims_id(dims), rank, M, min(a["scanned"][frames]), max(a["scanned"][frames]),
                                                                      max(a["flips"][frames])))


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_host_equals_restatement(C, dims):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    app, _ = osd_input(dims)
    for F in BATCHES:
        for kept in ((True,) if dims == WORKSPACE_DIMS else (False, True)):
            what = "%s F %d kept %s" % (dims_id(dims), F, kept)
            Din = kept_input(dims, F) if kept else None
            D, flips, scanned = np_outputs(dims, F, Din)
            before = None if Din is None else Din.copy()
            r = C.osd_host(H, J, L, Z, np.ascontiguousarray(app[:, :F]), Din)
            assert np.array_equal(r[1], flips), "flips: " + what
            assert np.array_equal(r[2], scanned), "scanned: " + what
            assert np.array_equal(r[0], D) and r[0].shape == (N + 1, F), "D: " + what
            assert Din is None or np.array_equal(Din, before), "D_in is read only"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    lib = C._lib.lib
    J, L, Z, F = 4, 24, 96, 2
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    N = L * Z
    app = np.ones((N, F), np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D, fl, sc = np.zeros((N + 1, F), np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32)

    def raw(F=F, app=app, Din=None, D=D, fl=fl, sc=sc, H=H):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_osd_host(J, L, Z, ptr(H), ptr(app), ptr(Din), F, ptr(D), ptr(fl), ptr(sc))
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_osd_host"
    assert raw() == (0, "") and raw(fl=None) == (0, "") and raw(sc=None) == (0, "") and raw(fl=None, sc=None) == (0, "")
    assert raw(Din=D) == (0, ""), "in place"
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(F=-3)[0] == -1
    assert raw(app=None) == (-1, who + ": null app") and raw(D=None) == (-1, who + ": null D")
    assert raw(H=None)[0] == -1
    Hbad = H.copy()
    Hbad[0, 0] = Z
    assert raw(H=Hbad)[0] == -1
    for bad in (dict(H=H[:-1]), dict(app=app.astype(np.float64)), dict(app=app[:-1]), dict(D=np.zeros((N, F), np.int32)),
                dict(D=np.zeros((N + 1, F), np.int64))):
        kw = dict(dict(H=H, app=app, D=None), **bad)
        with pytest.raises(ValueError):
            C.osd_host(kw["H"], J, L, Z, kw["app"], kw["D"])
    # the plan
    info = np.zeros(4, np.int32)

    def plan(tier=0, info=info, H=H, dims=(J, L, Z)):
        out = []
        for _ in range(2):
            rc = lib.bldpc_osd_plan_host(*dims, ptr(H), tier, ptr(info))
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_osd_plan_host"
    assert plan() == (0, "") and plan(info=None)[0] == -1 and plan(H=None)[0] == -1
    assert plan(tier=3) == (-1, who + ": unknown tier 3") and plan(tier=-1)[0] == -1
    H32 = read_H("J32_L64_Z64_BlockH.txt", 32, 64)
    rc, text = plan(tier=1, H=H32, dims=(32, 64, 64))
    assert rc == -5 and "BLDPC_ML_LDS" in text and "532480" in text and info[2] == -1
    rc, text = plan(H=read_H("PON_LDPC.txt", 12, 69), dims=(12, 69, 256))
    assert rc == -5 and "sort keys" in text and info[2] == -1
    big = np.zeros((2, 3), np.int32)  # M = 65538 check rows
    rc, text = plan(H=big, dims=(2, 3, 32769))
    assert rc == -5 and "65538 check rows" in text
    with pytest.raises(ValueError):
        C.osd_plan_host(H, J, L, Z, tier="fast")
    with pytest.raises(LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS"):
        C.osd_plan_host(H32, 32, 64, 64, tier="lds")


def test_sweep_refuses_osd_where_the_simulation_does():
    """Before any device is opened."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra, word in ((["--osd"], "--layered"), (["--osd", "--fixed"], "--layered"), (["--osd", "--layered", "--fixed"], "--stop-rule syndrome"),
                        (["--osd", "--bp", "--per-frame", "--stop-rule", "prefix"], "--stop-rule syndrome"),
                        (["--osd", "--hard", "gradient", "--per-frame", "--device-channel"], "--layered")):
        r = subprocess.run([sys.executable, os.path.join(root, "sweep.py"), "binary"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([sys.executable, os.path.join(root, "sweep.py"), "nb", "--osd"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--osd" in r.stderr


def test_simulations_refuse_osd_before_the_device():
    """The refusals of _check_osd, which both drivers make before anything touches the device."""
    from cuda_ldpc_amd import STOP_PREFIX, STOP_SYNDROME
    from cuda_ldpc_amd.simulation import _check_osd
    for schedule in ("layered", "bp", "quant"):
        _check_osd(True, schedule, STOP_SYNDROME)
        with pytest.raises(ValueError, match="STOP_SYNDROME"):
            _check_osd(True, schedule, STOP_PREFIX)
    for schedule in ("flooding", "hard"):
        with pytest.raises(ValueError, match="osd belongs to"):
            _check_osd(True, schedule, None)
        _check_osd(False, schedule, None)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def _plan_by_hand(J, L, Z):
    N, M = L * Z, J * Z
    P = 2
    while P < N:
        P *= 2
    record, side = 4 * M * (M // 32 + 1), 8 * P + 8 * ((N + 31) // 32) + 4 * M
    return record, side, min(1024, max(64, (M + 63) // 64 * 64))


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_plan_of_every_case(C, dims):
    record, side, threads = _plan_by_hand(*dims)
    lds = record + side <= LDS_BOUND
    assert lds == (dims != WORKSPACE_DIMS)
    assert C.osd_plan_host(matrix(dims), *dims) == dict(lds_bytes=record + side if lds else side, threads=threads, tier="lds" if lds else "workspace",
                                                       slots=0 if lds else 256)
    assert C.osd_plan_host(matrix(dims), *dims, tier="workspace") == dict(lds_bytes=side, threads=threads, tier="workspace", slots=256)
    if lds:
        assert C.osd_plan_host(matrix(dims), *dims, tier="lds")["tier"] == "lds"
    else:
        with pytest.raises(C._lib.LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS"):
            C.osd_plan_host(matrix(dims), *dims, tier="lds")


def test_plan_on_the_shipped_matrices(C):
    from cuda_ldpc_amd._lib import LdpcError
    assert C.osd_plan_host(read_H("J4_L24_Z96_BlockH.txt", 4, 24), 4, 24, 96) == dict(lds_bytes=54848, threads=384, tier="lds", slots=0)
    H32 = read_H("J32_L64_Z64_BlockH.txt", 32, 64)
    assert _plan_by_hand(32, 64, 64) == (532480, 41984, 1024)
    assert C.osd_plan_host(H32, 32, 64, 64) == dict(lds_bytes=41984, threads=1024, tier="workspace", slots=256)
    for name, dims in (("PON_LDPC.txt", (12, 69, 256)), ("J15_L30_Z1280_BlockH.txt", (15, 30, 1280))):  # the keys fit neither tier
        assert _plan_by_hand(*dims)[1] > LDS_BOUND
        for tier in ("auto", "lds", "workspace"):
            with pytest.raises(LdpcError, match=r"\(-5\): .*sort keys"):
                C.osd_plan_host(read_H(name, dims[0], dims[1]), *dims, tier=tier)
    # slots: what fits in 1 GiB.  7 680 check rows: a record of 7 403 520 bytes
    J, L, Z = 30, 32, 256
    record, side, _ = _plan_by_hand(J, L, Z)
    assert side <= LDS_BOUND and (1 << 30) // record == 145
    assert C.osd_plan_host(np.zeros((J, L), np.int32), J, L, Z) == dict(lds_bytes=side, threads=1024, tier="workspace", slots=145)


# ---- direction --------------------------------------------------------------------------------------------------------------------------
def test_reprocessing_after_layered_min_sum_on_a_shipped_code(C):
    """J4_L24_Z96 at sigma 0.52, 400 frames of the all-zero word from seed (173, 173, 173), ten iterations of layered min-sum with alpha
    0.75 and the syndrome rule, then reprocessing on its D and app.  Kept frames are untouched, so the frames in error cannot grow;
    every frame ends detected, undetected or correct; every reprocessed frame is a codeword.  No gain is asserted: the counts are
    printed, and the README records them."""
    J, L, Z, F = 4, 24, 96, 400
    N = L * Z
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = C.AWGNChannel_CPU(np.array([173, 173, 173], np.int32), 0.52, N, F)
    r = C.layered_host(H, J, L, Z, y, max_iter=10, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    D0 = r["D"]
    failed = D0[N] == 0
    wrong0 = D0[:N].any(0)
    before = int((failed | wrong0).sum())
    D, flips, scanned = C.osd_host(H, J, L, Z, r["app"], D0)
    assert np.array_equal(D[:, ~failed], D0[:, ~failed]) and (flips[~failed] == -1).all() and (scanned[~failed] == 0).all()
    assert (D[N] == 1).all() and not np_syndrome(np.asarray(H).reshape(J, L), Z, D[:N].astype(np.int64)).any(), "every frame is a codeword now"
    assert (flips[failed] >= 0).all() and (scanned[failed] >= J * Z - 3).all()
    wrong = D[:N].any(0)
    detected, undetected, correct = int(((D[N] == 0) & wrong).sum()), int(((D[N] != 0) & wrong).sum()), int((~wrong).sum())
    after = detected + undetected
    print("J4_L24_Z96 sigma 0.52, %d frames: %d in error after ten layered iterations (%d of them detected), %d after reprocessing "
          "(%d reprocessed, %d of them correct, all the rest undetected)" % (F, before, int(failed.sum()), after, int(failed.sum()),
                                                                            int((failed & ~wrong).sum())))
    assert detected + undetected + correct == F and detected == 0
    assert after <= before
    assert failed.sum() > 0, "the point must leave frames to reprocess"


# ---- the host statement under the host sanitizers, stand-alone -------------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def osd_exe(request, tmp_path_factory):
    """tests/cpp/osd_host_test.hip, built as test_erasure_ml_cpu.py builds erasure_ml_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("osd_host_" + request.param)
    exe = str(tmp / "osd_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "osd_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


def standalone_input(N, F):
    """The input of tests/cpp/osd_host_test.hip: (app float32 [N, F], D_in int32 [N+1, F])."""
    i = np.arange(N * F, dtype=np.uint64)
    x = (i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    app = (((x % np.uint64(4001)).astype(np.int64) - 1200).astype(np.float32) / np.float32(64.0)).reshape(N, F)
    n, f = np.arange(N + 1)[:, None], np.arange(F)[None, :]
    Din = ((7 * n + f) % 5 - 2).astype(np.int32)
    Din[N] = np.where(np.arange(F) % 3 == 1, np.arange(F) + 1, 0)
    return app, Din


@pytest.mark.parametrize("dims", [(3, 5, 13), (3, 7, 33), EXTREME, DEFICIENT], ids=dims_id)
def test_host_statement_stand_alone(C, osd_exe, tmp_path, dims):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F = 37
    app, Din = standalone_input(N, F)
    want = C.osd_host(H, J, L, Z, app, Din)
    assert (want[1] > 0).any() and (want[1] == -1).any() and (app < 0).any() and np.unique(app).size < app.size
    r = subprocess.run([osd_exe, path] + [str(a) for a in (J, L, Z, F)], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
    assert "Sanitizer" not in out and "runtime error" not in out, out
    tok = out.strip().split("\n")[-1].split()
    assert int(tok[0], 16) == fnv64(app, want[0], want[1], want[2]), "outputs differ from what the host statement returned in Python"
    if len(os.sched_getaffinity(0)) > 1:
        assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
