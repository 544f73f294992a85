"""The layered sum-product decoder without a GPU: the correction table against numpy's log1p(exp(.)), the accuracy of the table
box-plus against the exact rule (a derived bound), bldpc_decode_layered_bp_host (plain C++, the statement of the semantics inside
the product) against a numpy restatement of the specification in include/bldpc.h written here, bit for bit, on two shipped matrices
and on the random block matrices of tests/test_layered_shapes_cpu.py (every shape, the weight-27 one included); per-frame exit as
fixed runs; special values; the error rate against layered min-sum on the same noise; every refusal; and the host statement as a
stand-alone program (tests/cpp/bp_host_test.hip) under the address + undefined and the thread sanitizer.
tests/test_bp_gpu.py holds the device kernels against the host statement on the same matrices and inputs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_layered_cpu import (EXIT_BATCH_GLOBAL, EXIT_FIXED, EXIT_PER_FRAME, STOP_PREFIX, STOP_SYNDROME, raw_host_call, read_H, same_bits,
                              special_inputs)
from test_layered_shapes_cpu import F_RAMP, SHAPES, matrix_of, np_outputs, ramp_input, shape_id

FIXED_ITER, MAX_ITER = 5, 10
# SHAPES was laid out for the min-sum tiers: its (8, 16, 1000) holds 62 blocks, 312 000 bytes of S and R, and so runs the workspace
# kernel here.  One more shape puts Z = 1000 (24 idle lanes in the last wave) on the on-chip sum-product kernel.  The last field, the
# min-sum tier, is not used in these files: tests/test_bp_gpu.py holds the sum-product tiers.
EXTRA_SHAPES = [(3, 8, 1000, None, 31, None)]
BP_SHAPES = SHAPES + EXTRA_SHAPES
SCALE = 2.0
f32 = np.float32


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_T = {}


def table():
    """The product's table, read once (test_table_is_log1p_exp holds it against numpy): the restatement below looks it up."""
    if "T" not in _T:
        import cuda_ldpc_amd
        _T["T"] = cuda_ldpc_amd.BP_Table()
        _T["T"].setflags(write=False)
    return _T["T"]


# ---- the numpy restatement of the specification ---------------------------------------------------------------------------------------
def np_corr(T, x):
    inside = x < f32(8.0)
    idx = (np.where(inside, x, f32(0.0)) * f32(16.0)).astype(np.int64)
    return np.where(inside, T[idx], f32(0.0)).astype(np.float32)


def np_bp(T, a, b):
    aa, ab = np.abs(a), np.abs(b)
    m, p, d = np.minimum(aa, ab), aa + ab, np.abs(aa - ab)
    r = (m + np_corr(T, p)) - np_corr(T, d)
    r = np.where(r < 0, f32(0.0), r)
    return np.where(np.signbit(a) ^ np.signbit(b), -r, r).astype(np.float32)  # r >= +0: the negation sets the sign bit


def np_bp_pass(T, H, Z, S, R):
    """One iteration over S [N, F] and R {(j, l): [Z, F]} in place."""
    J, L = H.shape
    t = np.arange(Z)
    for j in range(J):
        cols = [l for l in range(L) if H[j, l] != -1]
        w = len(cols)
        v = [l * Z + (t + H[j, l]) % Z for l in cols]
        Q = [S[v[i]] - R[(j, cols[i])] for i in range(w)]
        Fw, Bw = [None] * w, [None] * w
        Fw[0] = Q[0]
        for i in range(1, w - 1):
            Fw[i] = np_bp(T, Fw[i - 1], Q[i])
        Bw[w - 1] = Q[w - 1]
        for i in range(w - 2, 0, -1):
            Bw[i] = np_bp(T, Q[i], Bw[i + 1])
        for i in range(w):
            r = Bw[1] if i == 0 else Fw[w - 2] if i == w - 1 else np_bp(T, Fw[i - 1], Bw[i + 1])
            S[v[i]] = Q[i] + r
            R[(j, cols[i])] = r


def np_bp_history(H, Z, y, iters, llr_scale):
    """S after every iteration, float32 [iters, N, F]: the layer passes do not depend on the stop rule, so one run serves every rule,
    every `length` and both exit modes (np_outputs of test_layered_shapes_cpu.py turns it into what each call must return)."""
    J, L = H.shape
    T = table()
    S = (f32(llr_scale) * y.astype(np.float32)).astype(np.float32)
    R = {(j, l): np.zeros((Z, y.shape[1]), np.float32) for j in range(J) for l in range(L) if H[j, l] != -1}
    hist = np.empty((iters,) + y.shape, np.float32)
    with np.errstate(all="ignore"):
        for it in range(iters):
            np_bp_pass(T, H, Z, S, R)
            hist[it] = S
    return hist


_hist = {}


def ramp_history(s):
    """The numpy history of the shape's ramp input, 10 iterations at llr_scale 2.0: computed once, never written to."""
    if s[:3] not in _hist:
        h = np_bp_history(matrix_of(s), s[2], ramp_input(s[1] * s[2], F_RAMP), MAX_ITER, SCALE)
        h.setflags(write=False)
        _hist[s[:3]] = h
    return _hist[s[:3]]


def rules_of(J, L, Z):
    N, K = L * Z, (L - J) * Z
    return [(STOP_SYNDROME, 0)] + [(STOP_PREFIX, n) for n in (0, 1, K - 1, N)]


def check_against_history(C, H, J, L, Z, y, hist, what):
    """Fixed runs of 5 iterations and per-frame runs of at most 10 under every rule: iters, flag row, hard bits, app as uint32."""
    for rule, length in rules_of(J, L, Z):
        w = "%s rule %d length %d" % (what, rule, length)
        (D, S, _), _ = np_outputs(H, Z, hist[:FIXED_ITER], length, rule)
        got = C.bp_host(H, J, L, Z, y, max_iter=FIXED_ITER, llr_scale=SCALE, length=length, stop_rule=rule)
        assert (got["iters"] == FIXED_ITER).all(), w
        assert np.array_equal(got["D"], D), "hard bits / flag row: " + w
        assert same_bits(got["app"], S), "a-posteriori bits: " + w
        _, (Dp, Sp, want_it) = np_outputs(H, Z, hist, length, rule)
        got = C.bp_host(H, J, L, Z, y, max_iter=MAX_ITER, llr_scale=SCALE, length=length, exit_mode=EXIT_PER_FRAME, stop_rule=rule)
        assert np.array_equal(got["iters"], want_it), "per-frame exit, iters: " + w
        assert np.array_equal(got["D"], Dp), "per-frame exit, hard bits / flag row: " + w
        assert same_bits(got["app"], Sp), "per-frame exit, a-posteriori bits: " + w


# ---- table and box-plus ---------------------------------------------------------------------------------------------------------------
def test_table_is_log1p_exp(C):
    T = C.BP_Table()
    assert T.dtype == np.float32 and T.shape == (128,) and np.array_equal(T, C.BP_Table())
    want = np.float32(np.log1p(np.exp(-(np.arange(128) + 0.5) / 16)))
    ulp = np.abs(T.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, "entries %s are %s ulp off" % (np.flatnonzero(ulp > 1), ulp[ulp > 1])
    assert (np.diff(T) < 0).all() and T[0] < np.log(2.0) and T[127] > np.log1p(np.exp(-8.0))


def test_box_plus_accuracy_against_the_exact_rule():
    """|table box-plus - exact box-plus| <= 1/32 + log1p(e^-8) + 1e-5 for |a|, |b| <= 32.  Derivation: c(x) = log1p(e^-x) has
    |c'| <= 1/2, a cell is 1/16 wide and holds c at its midpoint, so one look-up is off by at most 1/32 * 1/2 = 1/64 below 8 and by
    at most c(8) = log1p(e^-8) from 8 on (where it returns 0); two look-ups, 1/32 + c(8) with room (both cannot be at the tail's
    worst).  The clamp at 0 only moves a negative value towards the exact one, which is >= 0.  1e-5 covers the fp32 roundings of
    two additions below 64 (2 * 2^-19)."""
    rng = np.random.default_rng(3)
    a = np.clip(rng.standard_normal(2_000_000) * 8.0, -32, 32).astype(np.float32)
    b = np.clip(rng.standard_normal(2_000_000) * 8.0, -32, 32).astype(np.float32)
    a[:4], b[:4] = [32, -32, 0.0, 8.0], [32, 32, 5.0, -8.0]
    got = np_bp(table(), a, b).astype(np.float64)
    aa, ab = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
    exact = np.minimum(aa, ab) + np.log1p(np.exp(-(aa + ab))) - np.log1p(np.exp(-np.abs(aa - ab)))
    exact = np.where(np.signbit(a) ^ np.signbit(b), -exact, exact)
    small = (aa < 12) & (ab < 12)  # where the textbook form 2 atanh(tanh(a/2) tanh(b/2)) is still accurate in float64: the same rule
    textbook = 2 * np.arctanh(np.tanh(a[small].astype(np.float64) / 2) * np.tanh(b[small].astype(np.float64) / 2))
    assert small.sum() > 1_000_000 and np.allclose(exact[small], textbook, atol=1e-6, rtol=0)
    err = np.abs(got - exact).max()
    print("largest box-plus error over 2 M pairs: %.4f" % err)
    assert err <= 1 / 32 + np.log1p(np.exp(-8.0)) + 1e-5


def test_box_plus_sign_bit_is_the_xor_of_the_sign_bits():
    """A -0.0f input counts as negative; a zero magnitude (and a denormal one, absorbed by the table value) gives a zero of that sign."""
    T = table()
    a = np.array([0.0, -0.0, 3.0, -3.0, -0.0, 1e-45, 2.0, -2.0], np.float32)
    b = np.array([2.0, 2.0, -0.0, -0.0, -0.0, -1e-45, 5.0, 5.0], np.float32)
    r = np_bp(T, a, b)
    assert np.array_equal(np.signbit(r), [False, True, True, False, False, True, False, True])
    assert (r[:6] == 0).all() and r[6] == -r[7] and 1.9 < r[6] < 2.0


# ---- host statement against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,J,L,Z,F", [("J4_L24_Z96_BlockH.txt", 4, 24, 96, 6), ("J10_L60_Z160_BlockH.txt", 10, 60, 160, 4)])
def test_host_equals_numpy_on_shipped_matrices(C, name, J, L, Z, F):
    H = read_H(name, J, L)
    y = ramp_input(L * Z, F)
    check_against_history(C, H, J, L, Z, y, np_bp_history(H, Z, y, MAX_ITER, SCALE), name)


@pytest.mark.parametrize("s", BP_SHAPES, ids=shape_id)
def test_host_equals_numpy_on_random_shapes(C, s):
    J, L, Z = s[:3]
    check_against_history(C, matrix_of(s), J, L, Z, ramp_input(L * Z, F_RAMP), ramp_history(s), shape_id(s))


SPECIAL_SHAPES = [(3, 5, 13), (4, 27, 64), (3, 28, 64)]  # middle weights; 26, 2, 3, 25; 27


@pytest.mark.parametrize("dims", SPECIAL_SHAPES, ids=lambda d: "J%d_L%d_Z%d" % d)
def test_special_values(C, dims):
    """Zeros of both signs, denormals, 2^100 and exact ties (llr_scale 1.0: |llr_scale * y| stays within 2^100) on one shape per
    row-weight class; (4, 27, 64) holds the w = 2 row, which has no box-plus at all."""
    s = {x[:3]: x for x in SHAPES}[dims]
    J, L, Z = dims
    H = matrix_of(s)
    if dims == (4, 27, 64):
        assert {2, 3, 25, 26} <= set((H != -1).sum(1).tolist())
    y = special_inputs(L * Z, 8, np.random.default_rng(7))
    for scale in (1.0, 0.5):
        hist = np_bp_history(H, Z, y, 5, scale)
        assert not np.isnan(hist).any(), "the restatement must stay free of NaN on these inputs"
        for it in (1, 2, 5):
            (D, S, _), _ = np_outputs(H, Z, hist[:it], 0, STOP_PREFIX)
            got = C.bp_host(H, J, L, Z, y, max_iter=it, llr_scale=scale)
            assert np.array_equal(got["D"], D) and same_bits(got["app"], S), "llr_scale %g, %d iterations" % (scale, it)


# ---- per-frame exit -----------------------------------------------------------------------------------------------------------------------
THREE_COUNTS = {(3, 5, 13), (5, 8, 24), (5, 12, 32), (5, 12, 96), (32, 36, 16), (6, 12, 500)}


@pytest.mark.parametrize("s", BP_SHAPES, ids=shape_id)
def test_per_frame_exit_equals_fixed_runs(C, s):
    J, L, Z = s[:3]
    H = matrix_of(s)
    y = ramp_input(L * Z, F_RAMP)
    hist = ramp_history(s)
    for rule in (STOP_SYNDROME, STOP_PREFIX):
        (_, _, flags), (_, _, want_it) = np_outputs(H, Z, hist, 0, rule)
        # conditions on the input, judged by the restatement
        assert (want_it < MAX_ITER).any() and (want_it == MAX_ITER).any(), "frames that stop and frames that never do: %s" % want_it
        assert (flags[:-1, want_it == MAX_ITER] == 0).all()
        if s[:3] in THREE_COUNTS:
            assert np.unique(want_it).size >= 3, "iteration counts %s" % np.unique(want_it)
        got = C.bp_host(H, J, L, Z, y, max_iter=MAX_ITER, llr_scale=SCALE, exit_mode=EXIT_PER_FRAME, stop_rule=rule)
        assert np.array_equal(got["iters"], want_it)
        for it in np.unique(want_it):
            sel = want_it == it
            fixed = C.bp_host(H, J, L, Z, np.ascontiguousarray(y[:, sel]), max_iter=int(it), llr_scale=SCALE, stop_rule=rule)
            assert np.array_equal(got["D"][:, sel], fixed["D"]), "D of the frames that stop after %d iterations" % it
            assert same_bits(got["app"][:, sel], fixed["app"])


# ---- error rate ---------------------------------------------------------------------------------------------------------------------------
def test_sum_product_halves_the_frame_errors_of_min_sum(C):
    """J4_L24_Z96, sigma 0.52, 400 frames of the all-zero word, 10 layered iterations: frames with any wrong bit.  Everything is
    bit-exact, so the counts are deterministic; the numpy restatement gives 7 for sum-product against 40 for min-sum."""
    J, L, Z = 4, 24, 96
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = (1 + 0.52 * np.random.default_rng(11).standard_normal((2304, 400))).astype(np.float32)
    n_bp = int(C.bp_host(H, J, L, Z, y, max_iter=10, llr_scale=2 / 0.52 ** 2, want_app=False)["D"][: L * Z].any(0).sum())
    n_ms = int(C.layered_host(H, J, L, Z, y, max_iter=10, alpha=1.0, want_app=False)["D"][: L * Z].any(0).sum())
    print("frames in error of 400: sum-product %d, layered min-sum alpha 1.0 %d" % (n_bp, n_ms))
    assert n_ms > 0 and 2 * n_bp <= n_ms


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    J, L, Z = 4, 24, 96
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = np.ones((L * Z, 2), np.float32)

    def refused(code, **kw):
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(%d\): .*\S" % code) as e:
                C.bp_host(kw.get("H", H), J, L, Z, y, **{k: v for k, v in kw.items() if k != "H"})
            said.append(str(e.value))
        assert said[0] == said[1]

    for bad in (0.0, -2.0, float("nan"), float("inf"), float("-inf")):
        refused(-1, llr_scale=bad)
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
    refused(-5, H=H1)
    with pytest.raises(LdpcError, match=r"\(-5\): .*weight 1 sends nothing back \(the sum-product row update needs weight >= 2\)$"):
        C.bp_host(H1, J, L, Z, y)
    H0 = H.copy()
    H0[1, :] = -1  # and of weight 0
    refused(-5, H=H0)
    with pytest.raises(LdpcError, match=r"\(-5\): .*weight 0\b"):
        C.bp_host(H0, J, L, Z, y)
    import ctypes
    # two faults at once: the first one in the order of the checks is the one reported (F, max_iter, llr_scale, length, stop_rule, exit_mode)
    who = "bldpc_decode_layered_bp_host"
    assert raw_host_call(C, who, J, L, Z, H, y, 0, 5, ctypes.c_float(0.0), 0) == (-1, who + ": F=0 must be positive")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 5, ctypes.c_float(0.0), -1) == (-1, who + ": llr_scale=0 must be finite and positive")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 0, ctypes.c_float(0.0), -1) == (-1, who + ": max_iter=0 must be at least 1")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 5, ctypes.c_float(1.0), -1, stop_rule=2) == (-1, who + ": length=-1 outside [0,2304]")
    assert raw_host_call(C, who, J, L, Z, H1, y, 0, 5, ctypes.c_float(0.0), 0)[0] == -5  # the rows come before the arguments
    D = np.zeros((L * Z + 1, 2), np.int32)
    for _ in range(2):
        rc = C._lib.lib.bldpc_decode_layered_bp_host(J, L, Z, H.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 2, 5,
                                                     ctypes.c_float(1.0), 0, EXIT_PER_FRAME, STOP_PREFIX, D.ctypes.data_as(ctypes.c_void_p), None,
                                                     None)
        assert rc == -1 and b"iters" in C._lib.lib.bldpc_last_error()
    ok = C.bp_host(H, J, L, Z, y, max_iter=1, length=L * Z, exit_mode=EXIT_FIXED)  # the limits themselves are accepted
    assert ok["iters"].tolist() == [1, 1] and ok["D"][L * Z].tolist() == [1, 1]


# ---- the host statement under the host sanitizers, stand-alone ------------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def bp_exe(request, tmp_path_factory):
    """tests/cpp/bp_host_test.hip, built as test_enc_shapes_cpu.py builds encoder_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("bp_host_" + request.param)
    exe = str(tmp / "bp_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "bp_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


def generated_input(N, F):
    """What bp_host_test.hip generates, float32 [N, F]: y = 1 + (f / F) * g with g in [-2, 2) from a 32-bit integer hash of the
    element's index; integer arithmetic, one exact conversion, one division, one product and one sum in fp32."""
    i = np.arange(N * F, dtype=np.uint64)
    h = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    g = ((h >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * f32(2.0 ** -22)
    s = (np.arange(N * F) % F).astype(np.float32) / f32(F)
    return np.ascontiguousarray((f32(1.0) + s * g).astype(np.float32).reshape(N, F))


def fnv64(*arrays):
    h = 0xcbf29ce484222325
    for a in arrays:
        for byte in np.ascontiguousarray(a).tobytes():
            h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("dims", [(3, 5, 13), (5, 12, 96)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_host_statement_stand_alone(C, bp_exe, tmp_path, dims):
    s = {x[:3]: x for x in SHAPES}[dims]
    J, L, Z = dims
    H = matrix_of(s)
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F = 37
    y = generated_input(L * Z, F)
    for mode, max_iter, rule in ((EXIT_FIXED, FIXED_ITER, STOP_PREFIX), (EXIT_PER_FRAME, MAX_ITER, STOP_SYNDROME)):
        want = C.bp_host(H, J, L, Z, y, max_iter=max_iter, llr_scale=SCALE, exit_mode=mode, stop_rule=rule)
        if mode == EXIT_PER_FRAME:
            assert np.unique(want["iters"]).size >= 2, "the generated input must hold frames that stop at different times"
        r = subprocess.run([bp_exe, path] + [str(a) for a in (J, L, Z, F, max_iter, SCALE, mode, rule)], timeout=300, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        out = r.stdout.decode()
        assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
        assert "Sanitizer" not in out and "runtime error" not in out, out
        tok = out.strip().split("\n")[-1].split()
        assert int(tok[0], 16) == fnv64(want["D"], want["app"], want["iters"]), "D, app or iters differ from what bp_host returned in Python"
        if len(os.sched_getaffinity(0)) > 1:
            assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"
