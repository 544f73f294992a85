"""CPU tests of reprocessing of order 1 and 2 (include/bldpc.h): that the inputs of tests/osd_w_cases.py exercise every outcome, judged
by the restatement alone; the host statement bldpc_decode_osd_w_host against the restatement, exactly (D, flips, scanned, picked, metric
bits), on every shape, batch size and parameter set, with D_in NULL and with about half the frames kept; order 0 against
bldpc_decode_osd_host; what the definition promises of every processed frame; every refusal and the plan of every case; the counts on
a shipped code after ten layered iterations; and the host statement as a stand-alone program (tests/cpp/osd_w_host_test.hip) under the
address + undefined and the thread sanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from osd_cases import ALL_PLUS_ZERO, MIXED_ZEROS
from osd_w_cases import (DEFICIENT, DIMS, EXTREME, PAIR_DIMS, WORKSPACE_DIMS, WORKSPACE_W_PROCESSED, batches, dims_id, frames_of, kept_w_input,
                         matrix, metric_bits, n_frames, np_frames, np_syndrome, np_w_all, np_w_outputs, osd_w_input, pair_frame_positions, params,
                         processed_w)
from test_bp_cpu import fnv64
from test_layered_cpu import read_H
from test_osd_cpu import LDS_BOUND, SANITIZERS, _plan_by_hand, standalone_input


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_inputs_meet_their_conditions(dims):
    """By the restatement alone: at (2, 12) every LDS-tier shape has a processed frame that keeps order 0, one that picks a single, one
    that picks a pair and one with an exact metric tie at the minimum; the extra frames come out as the word sent with their pair."""
    J, L, Z = dims
    app, cw = osd_w_input(dims)
    assert app.shape == (L * Z, n_frames(dims)) and (n_frames(dims) > 64) == (dims in PAIR_DIMS)
    if dims == WORKSPACE_DIMS:
        assert len(processed_w()) == WORKSPACE_W_PROCESSED == len(frames_of(dims))
        return
    a = np_w_all(dims, 2, 12)
    singles = int(((a["picked"][0] >= 0) & (a["picked"][1] < 0)).sum())
    pairs = int((a["picked"][1] >= 0).sum())
    none = int((a["picked"][0] < 0).sum())
    ties = int((a["ties"] > 1).sum())
    print("%s at (2, 12): %d frames keep order 0, %d pick a single, %d a pair, %d have a tie at the minimum" % (dims_id(dims), none, singles, pairs, ties))
    assert none >= 1 and singles >= 1 and pairs >= 1 and ties >= 1
    for k in range(n_frames(dims) - 64):
        f = 64 + k
        assert a["picked"][:, f].tolist() == pair_frame_positions(dims, k) and np.array_equal(a["c"][:, f], cw[:, f])
        assert not np.array_equal(np_w_all(dims, 1, 0)["c"][:, f], cw[:, f]), "order 1 does not reach it"


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    D, flips, scanned, picked, mbits, done = want
    assert np.array_equal(got[1], flips), "flips: " + what
    assert np.array_equal(got[2], scanned), "scanned: " + what
    assert np.array_equal(got[3], picked), "picked: " + what
    assert np.array_equal(metric_bits(got[4])[done], mbits[done]), "metric bits: " + what
    assert np.array_equal(got[0], D), "D: " + what


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_host_equals_restatement(C, dims):
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    app, _ = osd_w_input(dims)
    for F in batches(dims):
        for kept in ((True,) if dims == WORKSPACE_DIMS else (False, True)):
            Din = kept_w_input(dims, F) if kept else None
            before = None if Din is None else Din.copy()
            for order, lam in params(dims):
                what = "%s F %d kept %s order %d lambda %d" % (dims_id(dims), F, kept, order, lam)
                r = C.osd_host(H, J, L, Z, np.ascontiguousarray(app[:, :F]), Din, order=order, lam=lam, want_metric=True)
                _same(r, np_w_outputs(dims, F, order, lam, Din), what)
                assert r[0].shape == (N + 1, F) and r[3].shape == (2, F) and r[4].dtype == np.float32
                assert (r[4][~np_w_outputs(dims, F, order, lam, Din)[5]] == 0).all(), "metric of a kept frame is not written"
                if order == 0:
                    old = C.osd_host(H, J, L, Z, np.ascontiguousarray(app[:, :F]), Din)
                    assert len(old) == 3 and all(np.array_equal(x, z) for x, z in zip(old, r[:3])), "order 0: " + what
                    assert (r[3] == -1).all()
            assert Din is None or np.array_equal(Din, before), "D_in is read only"


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_what_the_definition_promises(C, dims):
    """Of the host statement's outputs, per processed frame, with the basis taken from the restatement."""
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    app, _ = osd_w_input(dims)
    frames = frames_of(dims)
    F = n_frames(dims)
    Din = kept_w_input(dims, F) if dims == WORKSPACE_DIMS else None
    y = (app < 0).astype(np.int64)
    fr = np_frames(dims)
    last = {}
    for order, lam in params(dims):
        D, flips, scanned, picked, metric = C.osd_host(H, J, L, Z, app, Din, order=order, lam=lam, want_metric=True)
        assert not np_syndrome(H, Z, D[:N, frames].astype(np.int64)).any(), "zero syndrome"
        for f in frames:
            B, place = fr[f].B, {v: p for p, v in enumerate(fr[f].order)}
            S = [int(v) for v in picked[:, f] if v >= 0]
            assert len(S) <= order and (picked[0, f] >= 0 or picked[1, f] < 0) and not set(S) & set(B), "picked outside B"
            assert [place[v] for v in S] == sorted(place[v] for v in S) and len(set(S)) == len(S), "in ascending place"
            if order == 2 and len(S) == 2:
                assert all(fr[f].outside.index(place[v]) < lam for v in S), "a pair lies among the first lambda positions outside B"
            diff = np.flatnonzero(D[:N, f] != y[:, f])
            assert sorted(set(diff.tolist()) - set(B)) == sorted(S), "outside B the word differs from y exactly on picked"
            assert flips[f] == diff.size
            m = np.float32(0.0)
            with np.errstate(all="ignore"):
                for v in B:
                    if D[v, f] != y[v, f]:
                        m = np.float32(m + fr[f].w[v])
                for v in S:
                    m = np.float32(m + fr[f].w[v])
            assert metric_bits(m) == metric_bits(metric[f]), "the metric recomputed from the word"
            if f in (ALL_PLUS_ZERO, MIXED_ZEROS) and f in frames:
                assert not S and flips[f] == 0 and metric_bits(metric[f]) == 0, "nothing is picked where every value is zero"
        bits = metric_bits(metric)[frames].astype(np.int64)
        for o2, l2 in last:  # non-increasing from order 0 to 1 to (2, lambda), and in lambda
            if o2 < order or l2 <= lam:  # the candidates of (o2, l2) are among those of (order, lam)
                assert (bits <= last[(o2, l2)]).all(), "metric bits grow from (%d, %d) to (%d, %d)" % (o2, l2, order, lam)
        last[(order, lam)] = bits


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
    pk, me = np.zeros((2, F), np.int32), np.zeros(F, np.float32)

    def raw(F=F, app=app, Din=None, D=D, fl=fl, sc=sc, pk=pk, me=me, H=H, order=1, lam=0):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_osd_w_host(J, L, Z, ptr(H), ptr(app), ptr(Din), F, order, lam, ptr(D), ptr(fl), ptr(sc), ptr(pk), ptr(me))
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_osd_w_host"
    assert raw() == (0, "") and raw(fl=None, sc=None, pk=None, me=None) == (0, "") and raw(pk=None) == (0, "") and raw(me=None) == (0, "")
    assert raw(Din=D) == (0, ""), "in place"
    assert raw(order=0) == (0, "") and raw(order=2, lam=5) == (0, "") and raw(order=2, lam=10 ** 9) == (0, "")
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(F=-3)[0] == -1
    assert raw(app=None) == (-1, who + ": null app") and raw(D=None) == (-1, who + ": null D")
    assert raw(order=3) == (-1, who + ": order 3 outside 0 .. 2") and raw(order=-1)[0] == -1
    assert raw(order=2, lam=-1) == (-1, who + ": lambda=-1 must not be negative") and raw(order=0, lam=-1)[0] == -1
    assert raw(H=None)[0] == -1
    Hbad = H.copy()
    Hbad[0, 0] = Z
    assert raw(H=Hbad)[0] == -1
    for bad in (dict(H=H[:-1]), dict(app=app.astype(np.float64)), dict(app=app[:-1]), dict(D=np.zeros((N, F), np.int32))):
        kw = dict(dict(H=H, app=app, D=None), **bad)
        with pytest.raises(ValueError):
            C.osd_host(kw["H"], J, L, Z, kw["app"], kw["D"], order=1)
    with pytest.raises(LdpcError, match=r"\(-1\): .*order 3"):
        C.osd_host(H, J, L, Z, app, order=3)
    # the plan
    info = np.zeros(4, np.int32)

    def plan(tier=0, order=1, info=info, H=H, dims=(J, L, Z)):
        out = []
        for _ in range(2):
            rc = lib.bldpc_osd_w_plan_host(*dims, ptr(H), tier, order, ptr(info))
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_osd_w_plan_host"
    assert plan() == (0, "") and plan(order=0) == (0, "") and plan(order=2) == (0, "")
    assert plan(info=None)[0] == -1 and plan(H=None)[0] == -1
    assert plan(tier=3) == (-1, who + ": unknown tier 3") and plan(tier=-1)[0] == -1
    assert plan(order=3) == (-1, who + ": order 3 outside 0 .. 2") and plan(order=-1)[0] == -1 and info[2] == -1
    H32 = read_H("J32_L64_Z64_BlockH.txt", 32, 64)
    rc, text = plan(tier=1, H=H32, dims=(32, 64, 64))
    assert rc == -5 and "BLDPC_ML_LDS" in text and "532480" in text and info[2] == -1
    rc, text = plan(H=read_H("PON_LDPC.txt", 12, 69), dims=(12, 69, 256), order=2)
    assert rc == -5 and "sort keys" in text and info[2] == -1
    rc, text = plan(H=np.zeros((2, 3), np.int32), dims=(2, 3, 32769))
    assert rc == -5 and "65538 check rows" in text
    with pytest.raises(LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS"):
        C.osd_plan_host(H32, 32, 64, 64, tier="lds", order=2)


def test_simulations_refuse_an_order_without_osd():
    from cuda_ldpc_amd import STOP_SYNDROME
    from cuda_ldpc_amd.simulation import _check_osd
    _check_osd(True, "layered", STOP_SYNDROME, 2, 12)
    _check_osd(False, "layered", STOP_SYNDROME, 0, 0)
    for order, lam in ((1, 0), (2, 12), (0, 5)):
        with pytest.raises(ValueError, match="osd_order"):
            _check_osd(False, "layered", STOP_SYNDROME, order, lam)
    for order, lam in ((3, 0), (-1, 0), (2, -1)):
        with pytest.raises(ValueError, match="osd_order"):
            _check_osd(True, "layered", STOP_SYNDROME, order, lam)
    with pytest.raises(ValueError, match="osd belongs to"):
        _check_osd(True, "flooding", None, 1, 0)


def test_sweep_refuses_an_order_without_osd():
    """Before any device is opened."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra, word in ((["--osd-order", "1"], "belong to --osd"), (["--osd-lambda", "4"], "belong to --osd"), (["--osd", "--osd-order", "3"], "--osd-order"),
                        (["--osd", "--osd-order", "2"], "--layered"),
                        (["--osd", "--layered", "--per-frame", "--stop-rule", "syndrome", "--osd-order", "2", "--osd-lambda", "-1"], "--osd-lambda")):
        r = subprocess.run([sys.executable, os.path.join(root, "sweep.py"), "binary"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_plan_of_every_case(C, dims):
    """The search keeps its pivot list in the sort keys and takes no LDS of its own: the plan of every order is the one of k_osd."""
    record, side, threads = _plan_by_hand(*dims)
    lds = record + side <= LDS_BOUND
    assert lds == (dims != WORKSPACE_DIMS)
    for order in (0, 1, 2):
        assert C.osd_plan_host(matrix(dims), *dims, order=order) == dict(lds_bytes=record + side if lds else side, threads=threads,
                                                                        tier="lds" if lds else "workspace", slots=0 if lds else 256)
        assert C.osd_plan_host(matrix(dims), *dims, tier="workspace", order=order) == dict(lds_bytes=side, threads=threads, tier="workspace", slots=256)
        if lds:
            assert C.osd_plan_host(matrix(dims), *dims, tier="lds", order=order)["tier"] == "lds"
        else:
            with pytest.raises(C._lib.LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS"):
                C.osd_plan_host(matrix(dims), *dims, tier="lds", order=order)


# ---- direction --------------------------------------------------------------------------------------------------------------------------
def test_orders_after_layered_min_sum_on_a_shipped_code(C):
    """J4_L24_Z96 at sigma 0.52, 400 frames of the all-zero word from seed (173, 173, 173), ten iterations of layered min-sum with alpha
    0.75 and the syndrome rule (the setting of test_reprocessing_after_layered_min_sum_on_a_shipped_code), then the host statement at
    order 0, order 1 and (2, 60).  The frames in error after each are counted, printed and pinned; the definition guarantees no
    improvement (it minimises the metric, not the distance to the word sent), and none is asserted."""
    J, L, Z, F = 4, 24, 96, 400
    N = L * Z
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = C.AWGNChannel_CPU(np.array([173, 173, 173], np.int32), 0.52, N, F)
    r = C.layered_host(H, J, L, Z, y, max_iter=10, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    D0 = r["D"]
    failed = D0[N] == 0
    before = int((failed | D0[:N].any(0)).sum())
    counts, bits = [], []
    for order, lam in ((0, 0), (1, 0), (2, 60)):
        D, flips, scanned, picked, metric = C.osd_host(H, J, L, Z, r["app"], D0, order=order, lam=lam, want_metric=True)
        assert np.array_equal(D[:, ~failed], D0[:, ~failed]) and (flips[~failed] == -1).all() and (picked[:, ~failed] == -1).all()
        assert (D[N] == 1).all() and not np_syndrome(np.asarray(H).reshape(J, L), Z, D[:N].astype(np.int64)).any()
        counts.append(int(D[:N].any(0).sum()))
        bits.append(metric_bits(metric)[failed].astype(np.int64))
    print("J4_L24_Z96 sigma 0.52, %d frames: %d in error after ten layered iterations, %d reprocessed; in error after order 0: %d, after "
          "order 1: %d, after order 2 with lambda 60: %d" % (F, before, int(failed.sum()), *counts))
    assert (bits[1] <= bits[0]).all() and (bits[2] <= bits[1]).all()
    assert (before, counts[0]) == (11, 7)
    assert counts == PINNED_COUNTS


PINNED_COUNTS = [7, 6, 5]  # what the test found at that seed: frames in error after order 0, order 1 and (2, 60); the README quotes them


# ---- the host statement under the host sanitizers, stand-alone -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(SANITIZERS))
def osd_w_exe(request, tmp_path_factory):
    """tests/cpp/osd_w_host_test.hip, built as test_osd_cpu.py builds osd_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("osd_w_host_" + request.param)
    exe = str(tmp / "osd_w_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "osd_w_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("dims", [(3, 5, 13), (3, 7, 33), EXTREME, DEFICIENT], ids=dims_id)
def test_host_statement_stand_alone(C, osd_w_exe, tmp_path, dims):
    """The program runs (order, lambda) = (1, 0) and (2, 12) on the input of test_osd_cpu.py's stand-alone test; its digest is the one
    of what the host statement returned in Python."""
    J, L, Z = dims
    H, N = matrix(dims), L * Z
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F = 37
    app, Din = standalone_input(N, F)
    want = [C.osd_host(H, J, L, Z, app, Din, order=o, lam=lam) for o, lam in ((1, 0), (2, 12))]
    assert (dims == EXTREME or (want[1][3][0] >= 0).any()) and (want[1][1] == -1).any()  # EXTREME: this input keeps order 0 on every frame
    r = subprocess.run([osd_w_exe, path] + [str(a) for a in (J, L, Z, F)], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
    assert "Sanitizer" not in out and "runtime error" not in out, out
    tok = out.strip().split("\n")[-1].split()
    kept = Din[N] != 0
    parts = [app]
    for w in want:
        m = w[4].copy()
        m[kept] = 0
        parts += [w[0], w[1], w[2], w[3], metric_bits(m).astype(np.uint32)]
    assert int(tok[0], 16) == fnv64(*parts), "outputs differ from what the host statement returned in Python"
    if len(os.sched_getaffinity(0)) > 1:
        assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
