"""The quantised layered min-sum decoder without a GPU: bldpc_decode_layered_quant_host (plain C++, the statement of the semantics
inside the product) against the numpy restatement of tests/quant_cases.py, exactly, on three shipped matrices and on the random block
matrices of tests/test_layered_shapes_cpu.py under five parameter sets; per-frame exit as fixed runs; the conditions that the inputs
of tests/test_quant_gpu.py must meet, judged by the restatement alone; the error rate against fp32 layered min-sum on the same noise;
every refusal; and the host statement as a stand-alone program (tests/cpp/quant_host_test.hip) under the address + undefined and the
thread sanitizer.  tests/test_quant_gpu.py holds the device kernels against the host statement on the same matrices and inputs."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from quant_cases import (ACCEPTED, BY_DIMS, CLAMPS, F_PAIR, FIXED_ITER, INPUT, MAX_ITER, PARAMS, TIER, app_clamp_possible, input_for, np_quant_history,
                         np_quantise, pair_history, pair_input, special_input, tier_by_rule)
from test_bp_cpu import fnv64, generated_input
from test_layered_cpu import EXIT_BATCH_GLOBAL, EXIT_FIXED, EXIT_PER_FRAME, STOP_PREFIX, STOP_SYNDROME, raw_host_call, read_H
from test_layered_shapes_cpu import SHAPES, matrix_of, np_outputs, shape_id

GPU_PARAMS = ("P0", "P3")  # what test_quant_gpu.py runs on the random shapes


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def gpu_rules(s):
    """The stop rules test_quant_gpu.py runs on a shape: (rule, length)."""
    return [(STOP_SYNDROME, 0), (STOP_PREFIX, 0), (STOP_PREFIX, s[1] * s[2])]


def check_against_history(C, H, J, L, Z, y, hist, P, what, rules):
    """Fixed runs of 5 iterations and per-frame runs of at most 10 under every rule: iters, flag row, hard bits and app, exactly."""
    q = C.Quant(*P)
    for rule, length in rules:
        w = "%s %s rule %d length %d" % (what, P, rule, length)
        (D, S, _), _ = np_outputs(H, Z, hist[:FIXED_ITER], length, rule)
        got = C.quant_host(H, J, L, Z, y, q, max_iter=FIXED_ITER, length=length, stop_rule=rule)
        assert got["app"].dtype == np.int32 and (got["iters"] == FIXED_ITER).all(), w
        assert np.array_equal(got["D"], D), "hard bits / flag row: " + w
        assert np.array_equal(got["app"], S), "a-posteriori words: " + w
        _, (Dp, Sp, want_it) = np_outputs(H, Z, hist, length, rule)
        got = C.quant_host(H, J, L, Z, y, q, max_iter=MAX_ITER, length=length, exit_mode=EXIT_PER_FRAME, stop_rule=rule)
        assert np.array_equal(got["iters"], want_it), "per-frame exit, iters: " + w
        assert np.array_equal(got["D"], Dp), "per-frame exit, hard bits / flag row: " + w
        assert np.array_equal(got["app"], Sp), "per-frame exit, a-posteriori words: " + w


def all_rules(J, L, Z):
    N, K = L * Z, (L - J) * Z
    return [(STOP_SYNDROME, 0)] + [(STOP_PREFIX, n) for n in (0, 1, K - 1, N)]


# ---- the pieces -------------------------------------------------------------------------------------------------------------------------
def test_quantiser_rounds_ties_to_even_and_saturates(C):
    """The host statement has no quantiser of its own to call, so it is read from one iteration on a matrix whose rows each pair a
    hand-made value with a variable that quantises to 0: the smallest magnitude is 0, g(0) = 0, and the value comes back as it went in."""
    P = (6, 8, 6, 8, 0, 1.0)
    vals = np.array([0.5, 1.5, -0.5, -2.5, 2.5, 3.5, 0.49999997, 30.5, 31.0, 31.5, -31.5, 1e30, -1e30, 0.0, -0.0, 1e-45], np.float32)
    want = [0, 2, 0, -2, 2, 4, 0, 30, 31, 31, -31, 31, -31, 0, 0, 0]
    assert np_quantise(vals, P).tolist() == want
    J, L, Z = 1, 2, vals.size
    H = np.array([[0, 0]], np.int32)
    y = np.concatenate([np.zeros(Z, np.float32), vals])[:, None]  # block column 0 is all zero: both minima of every row are 0
    got = C.quant_host(H, J, L, Z, y, C.Quant(*P), max_iter=1, length=L * Z)
    assert got["app"][Z:, 0].tolist() == want  # Q + g(m1) with m1 = 0


def test_the_tier_table_follows_the_rule():
    assert len(ACCEPTED) == len(TIER) == len(SHAPES) - 1
    for s in ACCEPTED:
        assert (matrix_of(s) != -1).sum(1).max() <= 26
        assert TIER[s[:3]] == tier_by_rule(*s[:3]), shape_id(s)
    ws = {d for d, t in TIER.items() if t == "k_lq_ws"}
    assert ws == {(3, 8, 1056), (8, 16, 1000), (32, 34, 288)}
    weights = set(np.concatenate([(matrix_of(BY_DIMS[d]) != -1).sum(1) for d, t in TIER.items() if t == "k_lq"]).tolist())
    assert {2, 3, 25, 26} <= weights
    # the shipped matrices: all but the Z = 1280 one fit on-chip
    for name in os.listdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "data", "bldpc")):
        tok = name.split("_")
        if len(tok) == 4 and tok[3] == "BlockH.txt":
            J, L, Z = int(tok[0][1:]), int(tok[1][1:]), int(tok[2][1:])
            assert (tier_by_rule(J, L, Z) == "k_lq_ws") == (Z == 1280), name


# ---- host statement against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,J,L,Z,F", [("J4_L24_Z96_BlockH.txt", 4, 24, 96, 6), ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 6),
                                          ("J10_L60_Z160_BlockH.txt", 10, 60, 160, 4)])
def test_host_equals_numpy_on_shipped_matrices(C, name, J, L, Z, F):
    H = read_H(name, J, L)
    y = pair_input(L * Z, F)
    for P in PARAMS.values():
        hist, _ = np_quant_history(H, Z, y, MAX_ITER, P)
        check_against_history(C, H, J, L, Z, y, hist, P, name, all_rules(J, L, Z))


@pytest.mark.parametrize("s", ACCEPTED, ids=shape_id)
def test_host_equals_numpy_on_random_shapes(C, s):
    J, L, Z = s[:3]
    H = matrix_of(s)
    y = input_for(s)
    for name, P in PARAMS.items():
        hist = pair_history(s, name)[0] if name in GPU_PARAMS else np_quant_history(H, Z, y, MAX_ITER, P)[0]
        check_against_history(C, H, J, L, Z, y, hist, P, shape_id(s), all_rules(J, L, Z) if name in GPU_PARAMS else gpu_rules(s))


def test_host_has_no_upper_weight_limit(C):
    s = SHAPES[-1]
    J, L, Z = s[:3]
    H = matrix_of(s)
    assert (H != -1).sum(1).max() == 27
    y = pair_input(L * Z, 8)
    hist, _ = np_quant_history(H, Z, y, MAX_ITER, PARAMS["P1"])
    check_against_history(C, H, J, L, Z, y, hist, PARAMS["P1"], shape_id(s), gpu_rules(s))


@pytest.mark.parametrize("dims", [(3, 8, 1056), (5, 12, 32), (4, 27, 64)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_special_values(C, dims):
    """The inputs of test_quant_gpu.test_special_values_on_every_tier: the host statement against the restatement."""
    s = BY_DIMS[dims]
    J, L, Z = dims
    H = matrix_of(s)
    for name in ("P1", "P2", "P4"):
        P = PARAMS[name]
        y = special_input(L * Z, 8, P)
        hist, counts = np_quant_history(H, Z, y, MAX_ITER, P)
        assert counts["channel"] > 0
        check_against_history(C, H, J, L, Z, y, hist, P, shape_id(s) + " special", gpu_rules(s))


# ---- per-frame exit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ACCEPTED, ids=shape_id)
def test_per_frame_exit_equals_fixed_runs(C, s):
    J, L, Z = s[:3]
    H = matrix_of(s)
    y = input_for(s)
    for name in GPU_PARAMS:
        q = C.Quant(*PARAMS[name])
        hist = pair_history(s, name)[0]
        for rule in (STOP_SYNDROME, STOP_PREFIX):
            _, (_, _, want_it) = np_outputs(H, Z, hist, 0, rule)
            got = C.quant_host(H, J, L, Z, y, q, max_iter=MAX_ITER, exit_mode=EXIT_PER_FRAME, stop_rule=rule)
            assert np.array_equal(got["iters"], want_it)
            for it in np.unique(want_it):
                sel = want_it == it
                fixed = C.quant_host(H, J, L, Z, np.ascontiguousarray(y[:, sel]), q, max_iter=int(it), stop_rule=rule)
                assert np.array_equal(got["D"][:, sel], fixed["D"]), "D of the frames that stop after %d iterations" % it
                assert np.array_equal(got["app"][:, sel], fixed["app"])


# ---- conditions on the inputs of the GPU file, judged by the restatement alone ------------------------------------------------------
@pytest.mark.parametrize("s", ACCEPTED, ids=shape_id)
def test_gpu_inputs_meet_their_conditions(s):
    """For exactly the cases test_quant_gpu.test_random_shapes_match_host runs with F = 37.  The clamp of S cannot act on every
    matrix: |S| <= C + wc * g(Mx) for a column of weight wc, which stays within A for wc <= 3 under P0 and for wc <= 4 under P3
    (quant_cases.app_clamp_possible).  Where it can act it must, on this input; where it cannot, the count must be 0."""
    J, L, Z = s[:3]
    H = matrix_of(s)
    for name in GPU_PARAMS:
        hist, counts = pair_history(s, name)
        print("%s %s clamp counts %s" % (shape_id(s), name, counts))
        for c in CLAMPS if name == "P3" else ("app",):
            if c == "app" and not app_clamp_possible(H, PARAMS[name]):
                assert counts[c] == 0
            else:
                assert counts[c] > 0, "%s: the %s clamp never acts under %s" % (shape_id(s), c, name)
        for rule, length in gpu_rules(s):
            what = "%s %s rule %d length %d" % (shape_id(s), name, rule, length)
            (_, _, flags), (_, _, it) = np_outputs(H, Z, hist, length, rule)
            print("%s: iters %s" % (what, it.tolist()))
            assert (it < MAX_ITER).any() and (it == MAX_ITER).any(), "frames that stop and frames that never do: " + what
            assert (flags[:-1, it == MAX_ITER] == 0).all()
            assert np.unique(it).size >= 3, "three distinct iteration counts: " + what
            even, odd = it[0:F_PAIR - 1:2], it[1:F_PAIR:2]
            assert (even < odd).any(), "a pair whose even frame stops strictly earlier: " + what
            assert (odd < even).any(), "a pair whose odd frame stops strictly earlier: " + what


def test_the_clamp_of_S_acts_on_both_tiers():
    for name in GPU_PARAMS:
        tiers = {TIER[s[:3]] for s in ACCEPTED if app_clamp_possible(matrix_of(s), PARAMS[name])}
        assert tiers == {"k_lq", "k_lq_ws"}, name
    assert set(INPUT) <= set(TIER)


# ---- error rate ---------------------------------------------------------------------------------------------------------------------------
def test_quantised_halves_the_frame_errors_of_plain_min_sum(C):
    """The input of test_sum_product_halves_the_frame_errors_of_min_sum (J4_L24_Z96, sigma 0.52, seed 11, 400 frames of the all-zero
    word), 10 iterations: frames with any wrong bit.  Integer arithmetic: the counts are deterministic.  Measured: P1 (6, 8, 6),
    norm8 6, scale 16 leaves 9 against 40 of fp32 layered min-sum at alpha 1.0 (and 9 at alpha 0.75); scale 8 leaves 14, offset 1
    without normalisation at scale 16 leaves 10."""
    J, L, Z = 4, 24, 96
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = (1 + 0.52 * np.random.default_rng(11).standard_normal((2304, 400))).astype(np.float32)

    def errors(r):
        return int(r["D"][: L * Z].any(0).sum())

    n_q = errors(C.quant_host(H, J, L, Z, y, C.Quant(*PARAMS["P1"]), max_iter=10, want_app=False))
    n_ms = errors(C.layered_host(H, J, L, Z, y, max_iter=10, alpha=1.0, want_app=False))
    n_75 = errors(C.layered_host(H, J, L, Z, y, max_iter=10, alpha=0.75, want_app=False))
    n_8 = errors(C.quant_host(H, J, L, Z, y, C.Quant(6, 8, 6, 6, 0, 8.0), max_iter=10, want_app=False))
    n_off = errors(C.quant_host(H, J, L, Z, y, C.Quant(6, 8, 6, 8, 1, 16.0), max_iter=10, want_app=False))
    print("frames in error of 400: quantised P1 %d, fp32 layered min-sum alpha 1.0 %d, alpha 0.75 %d; quantised at scale 8 %d, "
          "offset 1 at scale 16 %d" % (n_q, n_ms, n_75, n_8, n_off))
    assert n_ms > 0 and 2 * n_q <= n_ms


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
GOOD = dict(bits_ch=6, bits_app=8, bits_msg=6, norm8=6, offset=0, llr_scale=16.0)
BAD = [dict(llr_scale=0.0), dict(llr_scale=-2.0), dict(llr_scale=float("nan")), dict(llr_scale=float("inf")), dict(llr_scale=float("-inf")),
       dict(bits_ch=1), dict(bits_ch=9), dict(bits_app=5), dict(bits_app=16), dict(bits_msg=1), dict(bits_msg=9, bits_app=12),
       dict(norm8=0), dict(norm8=9), dict(offset=-1), dict(offset=32)]
EDGE = [dict(bits_ch=2), dict(bits_ch=8), dict(bits_app=6), dict(bits_app=15), dict(bits_msg=2, bits_ch=2, bits_app=2), dict(bits_msg=8),
        dict(norm8=1), dict(norm8=8), dict(offset=31)]


def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError, bldpc_quant
    J, L, Z = 4, 24, 96
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = np.ones((L * Z, 2), np.float32)
    good = C.Quant(**GOOD)

    def raw(**kw):
        p = dict(GOOD, **kw)
        return bldpc_quant(p["llr_scale"], p["bits_ch"], p["bits_app"], p["bits_msg"], p["norm8"], p["offset"])

    def refused(code, quant=good, **kw):
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(%d\): .*\S" % code) as e:
                C.quant_host(H, J, L, Z, y, quant, **kw)
            said.append(str(e.value))
        assert said[0] == said[1]
        return said[0]

    for bad in BAD:  # every bound, on both sides
        with pytest.raises(ValueError, match=list(bad)[0]):
            C.Quant(**dict(GOOD, **bad))
        assert list(bad)[0] in refused(-1, quant=raw(**bad)), bad
    for ok in EDGE:  # the limits themselves are accepted, on both sides
        r = C.quant_host(H, J, L, Z, y, C.Quant(**dict(GOOD, **ok)), max_iter=1)
        assert r["iters"].tolist() == [1, 1]
        assert np.array_equal(C.quant_host(H, J, L, Z, y, raw(**ok), max_iter=1)["D"], r["D"])
    with pytest.raises(ValueError):
        C.Quant(bits_ch=6.5)
    with pytest.raises(ValueError):
        C.quant_host(H, J, L, Z, y, PARAMS["P1"])  # a tuple is no Quant
    assert "null" in refused(-1, quant=None)
    refused(-1, max_iter=0)
    refused(-1, max_iter=-3)
    refused(-1, length=L * Z + 1)
    refused(-1, length=-1)
    refused(-1, stop_rule=2)
    refused(-1, stop_rule=-1)
    refused(-1, exit_mode=EXIT_BATCH_GLOBAL)
    refused(-1, exit_mode=7)
    H1 = H.copy()
    H1[2, 1:] = -1  # a block row of weight 1
    with pytest.raises(LdpcError, match=r"\(-5\): .*weight 1\b"):
        C.quant_host(H1, J, L, Z, y, good)
    H0 = H.copy()
    H0[1, :] = -1  # and of weight 0
    with pytest.raises(LdpcError, match=r"\(-5\): .*weight 0\b"):
        C.quant_host(H0, J, L, Z, y, good)
    # two faults at once: the quantiser's parameters are checked first, before the rows; then F, max_iter, length, stop_rule, exit_mode
    who = "bldpc_decode_layered_quant_host"
    ref = lambda **kw: ctypes.byref(raw(**kw))  # noqa: E731
    assert raw_host_call(C, who, J, L, Z, H, y, 0, 5, ref(llr_scale=0.0), 0) == (-1, who + ": llr_scale=0 must be finite and positive")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 5, ref(bits_msg=1), -1) == (-1, who + ": bits_msg=1 outside [2,8]")
    assert raw_host_call(C, who, J, L, Z, H1, y, 2, 5, ref(norm8=9), 0) == (-1, who + ": norm8=9 outside [1,8]")
    assert raw_host_call(C, who, J, L, Z, H, y, 0, 0, ref(), -1) == (-1, who + ": F=0 must be positive")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 0, ref(), -1) == (-1, who + ": max_iter=0 must be at least 1")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 5, ref(), -1, stop_rule=2) == (-1, who + ": length=-1 outside [0,2304]")
    assert raw_host_call(C, who, J, L, Z, H1, y, 0, 5, ref(), 0)[0] == -5  # the rows come before the arguments
    D = np.zeros((L * Z + 1, 2), np.int32)
    for _ in range(2):
        rc = C._lib.lib.bldpc_decode_layered_quant_host(J, L, Z, H.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 2, 5,
                                                        ctypes.byref(good.c_struct()), 0, EXIT_PER_FRAME, STOP_PREFIX,
                                                        D.ctypes.data_as(ctypes.c_void_p), None, None)
        assert rc == -1 and b"iters" in C._lib.lib.bldpc_last_error()
    ok = C.quant_host(H, J, L, Z, y, good, max_iter=1, length=L * Z, exit_mode=EXIT_FIXED)
    assert ok["iters"].tolist() == [1, 1] and ok["D"][L * Z].tolist() == [1, 1] and (ok["app"] > 0).all()


# ---- the host statement under the host sanitizers, stand-alone ------------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def quant_exe(request, tmp_path_factory):
    """tests/cpp/quant_host_test.hip, built as test_bp_cpu.py builds bp_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("quant_host_" + request.param)
    exe = str(tmp / "quant_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "quant_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.mark.parametrize("dims", [(3, 5, 13), (5, 12, 96)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_host_statement_stand_alone(C, quant_exe, tmp_path, dims):
    s = BY_DIMS[dims]
    J, L, Z = dims
    H = matrix_of(s)
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F = 37
    y = generated_input(L * Z, F)
    for mode, max_iter, rule, name in ((EXIT_FIXED, FIXED_ITER, STOP_PREFIX, "P3"), (EXIT_PER_FRAME, MAX_ITER, STOP_SYNDROME, "P1")):
        P = PARAMS[name]
        want = C.quant_host(H, J, L, Z, y, C.Quant(*P), max_iter=max_iter, exit_mode=mode, stop_rule=rule)
        if mode == EXIT_PER_FRAME:
            assert np.unique(want["iters"]).size >= 2, "the generated input must hold frames that stop at different times"
        r = subprocess.run([quant_exe, path] + [str(a) for a in (J, L, Z, F, max_iter, mode, rule) + P], timeout=300, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        out = r.stdout.decode()
        assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
        assert "Sanitizer" not in out and "runtime error" not in out, out
        tok = out.strip().split("\n")[-1].split()
        assert int(tok[0], 16) == fnv64(want["D"], want["app"], want["iters"]), "D, app or iters differ from what quant_host returned in Python"
        if len(os.sched_getaffinity(0)) > 1:
            assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
