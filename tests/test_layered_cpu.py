"""The layered normalised min-sum decoder without a GPU: bldpc_decode_layered_host (plain C++, the statement of the semantics
inside the product) against a numpy restatement of the specification in include/bldpc.h written here (block-wise gathers,
np.signbit, sort + first argmin), bit for bit on hard bits and a-posteriori values; per-frame exit under both stop rules;
special values; alpha = 1; the convergence claim against flooding on the same noise; every refusal; the host statement as a
stand-alone program (tests/cpp/layered_host_test.hip) under the address + undefined and the thread sanitizer; and the tier rules of
the three layered decoders against what the commit before their host sides were merged chose (tests/golden/layer_tier_choices.json)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DATA
from test_binary_crosscheck_cpu import CASES

BL = os.path.join(DATA, "bldpc")
EXIT_FIXED, EXIT_BATCH_GLOBAL, EXIT_PER_FRAME = 0, 1, 2
STOP_PREFIX, STOP_SYNDROME = 0, 1


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def read_H(name, J, L):
    return np.loadtxt(os.path.join(BL, name), dtype=np.int32).reshape(-1)[: J * L].reshape(J, L)


def np_layer_pass(H, Z, S, R, alpha, multiply=True):
    """One iteration over S [N, F] and R {(j, l): [Z, F]} in place.  multiply=False: the restatement without any multiplication."""
    J, L = H.shape
    t = np.arange(Z)
    for j in range(J):
        cols = [l for l in range(L) if H[j, l] != -1]
        v = [l * Z + (t + H[j, l]) % Z for l in cols]
        Q = np.stack([S[v[i]] - R[(j, cols[i])] for i in range(len(cols))])  # [w, Z, F]
        sg = np.signbit(Q)
        P = np.logical_xor.reduce(sg, axis=0)
        a = np.abs(Q)
        srt = np.sort(a, axis=0)
        m1, m2 = srt[0], srt[1]
        first = np.argmax(a == m1[None], axis=0)
        for i in range(len(cols)):
            mag = np.where(first == i, m2, m1)
            if multiply:
                mag = np.float32(alpha) * mag
            r = np.where(P ^ sg[i], -mag, mag).astype(np.float32)
            S[v[i]] = Q[i] + r
            R[(j, cols[i])] = r


def np_syndrome_ok(H, Z, d):
    J, L = H.shape
    t = np.arange(Z)
    bad = np.zeros(d.shape[1], bool)
    for j in range(J):
        x = np.zeros((Z, d.shape[1]), bool)
        for l in range(L):
            if H[j, l] != -1:
                x ^= d[l * Z + (t + H[j, l]) % Z]
        bad |= x.any(0)
    return ~bad


def np_layered(H, Z, y, iters, alpha=1.0, length=0, stop_rule=STOP_PREFIX, multiply=True):
    """Fixed run: (D [N+1, F], S [N, F]) after `iters` iterations, and the flag of every frame after each iteration [iters, F]."""
    J, L = H.shape
    N, F = y.shape
    length = length or N - J * Z
    S = y.astype(np.float32).copy()
    R = {(j, l): np.zeros((Z, F), np.float32) for j in range(J) for l in range(L) if H[j, l] != -1}
    flags = np.zeros((iters, F), np.int32)
    with np.errstate(all="ignore"):
        for it in range(iters):
            np_layer_pass(H, Z, S, R, alpha, multiply)
            d = S < 0
            flags[it] = np_syndrome_ok(H, Z, d) if stop_rule == STOP_SYNDROME else ~d[:length].any(0)
    D = np.concatenate([(S < 0).astype(np.int32), flags[-1:]], 0)
    return D, S, flags


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


ALPHAS = (1.0, 0.75, 0.8)


@pytest.mark.parametrize("name,J,L,Z,F,snr,its", CASES)
def test_host_equals_numpy_restatement(C, orc, name, J, L, Z, F, snr, its):
    H = read_H(name, J, L)
    y = orc.bldpc_awgn(np.array([173, 173, 173], np.int32), orc.bldpc_sigma(snr), L * Z, F).reshape(L * Z, F)
    for alpha in ALPHAS:
        for it in its:
            for rule in (STOP_PREFIX, STOP_SYNDROME):
                if rule == STOP_SYNDROME and it != its[-1]:
                    continue
                D, S, _ = np_layered(H, Z, y, it, alpha, stop_rule=rule)
                got = C.layered_host(H, J, L, Z, y, max_iter=it, alpha=alpha, stop_rule=rule)
                assert np.array_equal(got["D"], D), "hard bits / flag row, %d iterations, alpha %g, rule %d" % (it, alpha, rule)
                assert same_bits(got["app"], S), "a-posteriori bits, %d iterations, alpha %g" % (it, alpha)
                assert (got["iters"] == it).all()


@pytest.mark.parametrize("rule", [STOP_PREFIX, STOP_SYNDROME])
@pytest.mark.parametrize("alpha", [1.0, 0.75])
def test_per_frame_exit_equals_fixed_runs(C, orc, rule, alpha):
    J, L, Z, F, max_iter = 4, 24, 96, 48, 12
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = orc.bldpc_awgn(np.array([173, 173, 173], np.int32), orc.bldpc_sigma(2.6), L * Z, F).reshape(L * Z, F)
    got = C.layered_host(H, J, L, Z, y, max_iter=max_iter, alpha=alpha, exit_mode=EXIT_PER_FRAME, stop_rule=rule)
    _, _, flags = np_layered(H, Z, y, max_iter, alpha, stop_rule=rule)
    want_it = np.where(flags.any(0), flags.argmax(0) + 1, max_iter)
    assert np.array_equal(got["iters"], want_it)
    assert (want_it == max_iter).any() and (want_it < max_iter).any(), "the case must hold converged and unconverged frames"
    assert (flags[:, want_it == max_iter][:-1] == 0).all()
    for it in np.unique(want_it):
        sel = want_it == it
        fixed = C.layered_host(H, J, L, Z, np.ascontiguousarray(y[:, sel]), max_iter=int(it), alpha=alpha, stop_rule=rule)
        assert np.array_equal(got["D"][:, sel], fixed["D"]), "D of the frames that stop after %d iterations" % it
        assert same_bits(got["app"][:, sel], fixed["app"])
        D, S, _ = np_layered(H, Z, y[:, sel], int(it), alpha, stop_rule=rule)
        assert np.array_equal(fixed["D"], D) and same_bits(fixed["app"], S)


def special_inputs(N, F, rng):
    """Channel values that exercise zeros of both signs, denormals, large magnitudes and exact ties of two and of many minima,
    without overflow: |y| <= 2^100, so sums of the at most Wv + 1 terms of an a-posteriori value stay finite."""
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.0, -1.0, 1.0, -1.0, 0.5, -0.5, 2.0 ** 100, -2.0 ** 100, 3.0, -3.0,
                     1.1754944e-38, -1.1754944e-38, 7.0, 0.25], np.float32)
    y = pool[rng.integers(0, pool.size, (N, F))]
    y[:, 0] = 1.0  # every magnitude ties
    y[:, 1] = np.where(rng.random(N) < 0.5, np.float32(0.0), np.float32(-0.0))
    y[:, 2] = np.float32(1e-45) * rng.choice(np.array([-1, 1], np.float32), N)
    return np.ascontiguousarray(y)


@pytest.mark.parametrize("name,J,L,Z", [("J4_L24_Z96_BlockH.txt", 4, 24, 96), ("J32_L64_Z64_BlockH.txt", 32, 64, 64)])
def test_special_values(C, name, J, L, Z):
    H = read_H(name, J, L)
    y = special_inputs(L * Z, 8, np.random.default_rng(7))
    for alpha in ALPHAS:
        for it in (1, 2, 5):
            D, S, _ = np_layered(H, Z, y, it, alpha)
            assert not np.isnan(S).any(), "the restatement must stay free of NaN on these inputs"
            got = C.layered_host(H, J, L, Z, y, max_iter=it, alpha=alpha)
            assert np.array_equal(got["D"], D) and same_bits(got["app"], S), "alpha %g, %d iterations" % (alpha, it)


def test_alpha_one_is_no_multiplication(C, orc):
    J, L, Z, F = 4, 24, 96, 8
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    ys = [orc.bldpc_awgn(np.array([173, 173, 173], np.int32), orc.bldpc_sigma(2.0), L * Z, F).reshape(L * Z, F),
          special_inputs(L * Z, F, np.random.default_rng(11))]
    for y in ys:
        for it in (1, 3, 8):
            D, S, _ = np_layered(H, Z, y, it, multiply=False)
            got = C.layered_host(H, J, L, Z, y, max_iter=it, alpha=1.0)
            assert np.array_equal(got["D"], D) and same_bits(got["app"], S)


def test_layered_25_beats_flooding_50_on_the_same_noise(C, orc):
    """J4_L24_Z96, Es/N0 2.6 dB, seeds 173/173/173, 1024 frames of the host channel: frames with any wrong bit among all N.
    Everything is bit-exact, so the counts are deterministic: 25 layered iterations (alpha 1.0) must not lose to 50 flooding
    iterations of the C oracle, and alpha 0.75 must not lose to alpha 1.0."""
    J, L, Z, F = 4, 24, 96, 1024
    name = "J4_L24_Z96_BlockH.txt"
    H = read_H(name, J, L)
    y = orc.bldpc_awgn(np.array([173, 173, 173], np.int32), orc.bldpc_sigma(2.6), L * Z, F)
    flood = orc.bldpc_decode(orc.BinaryCode(os.path.join(BL, name), J, L, Z), y, F, 50, early_exit=0)
    n_flood = int(flood["D"][: L * Z * F].reshape(L * Z, F).any(0).sum())
    y2 = y.reshape(L * Z, F)
    n_lay = int(C.layered_host(H, J, L, Z, y2, max_iter=25, alpha=1.0, want_app=False)["D"][: L * Z].any(0).sum())
    n_lay75 = int(C.layered_host(H, J, L, Z, y2, max_iter=25, alpha=0.75, want_app=False)["D"][: L * Z].any(0).sum())
    print("frames in error of %d: flooding 50 it. %d, layered 25 it. alpha 1.0 %d, alpha 0.75 %d" % (F, n_flood, n_lay, n_lay75))
    assert n_lay <= n_flood
    assert n_lay75 <= n_lay


def raw_host_call(C, name, J, L, Z, H, y, F, max_iter, param, length, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX):
    """A layered host statement called past the Python wrapper's own checks (F = 0 never reaches C through it): (status, error text).
    param: the decoder's own argument, a ctypes value."""
    import ctypes
    D = np.zeros((L * Z + 1, max(F, 1)), np.int32)
    iters = np.zeros(max(F, 1), np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = getattr(C._lib.lib, name)(J, L, Z, ptr(H), ptr(y), F, max_iter, param, length, exit_mode, stop_rule, ptr(D), None, ptr(iters))
    return rc, C._lib.lib.bldpc_last_error().decode()


def test_refusals(C):
    import ctypes
    from cuda_ldpc_amd._lib import LdpcError
    J, L, Z = 4, 24, 96
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = np.ones((L * Z, 2), np.float32)

    def refused(code, **kw):
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=r"\(%d\): .*\S" % code) as e:
                C.layered_host(kw.get("H", H), J, L, Z, y, **{k: v for k, v in kw.items() if k != "H"})
            said.append(str(e.value))
        assert said[0] == said[1]

    # two faults at once: the first one in the order of the checks is the one reported (F, max_iter, alpha, length, stop_rule, exit_mode)
    who = "bldpc_decode_layered_host"
    assert raw_host_call(C, who, J, L, Z, H, y, 0, 5, ctypes.c_float(0.0), 0) == (-1, who + ": F=0 must be positive")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 5, ctypes.c_float(2.0), -1) == (-1, who + ": alpha=2 outside (0, 1]")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 0, ctypes.c_float(2.0), -1) == (-1, who + ": max_iter=0 must be at least 1")
    assert raw_host_call(C, who, J, L, Z, H, y, 2, 5, ctypes.c_float(1.0), -1, stop_rule=2) == (-1, who + ": length=-1 outside [0,2304]")

    refused(-1, max_iter=0)
    refused(-1, alpha=0.0)
    refused(-1, alpha=1.5)
    refused(-1, alpha=-0.5)
    refused(-1, alpha=float("nan"))
    refused(-1, alpha=float("inf"))
    refused(-1, stop_rule=2)
    refused(-1, exit_mode=EXIT_BATCH_GLOBAL)
    refused(-1, exit_mode=7)
    refused(-1, length=L * Z + 1)
    H1 = H.copy()
    H1[2, 1:] = -1  # a block row of weight 1
    refused(-5, H=H1)
    with pytest.raises(LdpcError, match=r"\(-5\): .*weight 1 has no second minimum \(layered min-sum needs weight >= 2\)$"):
        C.layered_host(H1, J, L, Z, y)
    H0 = H.copy()
    H0[1, :] = -1  # and of weight 0
    with pytest.raises(LdpcError, match=r"\(-5\): .*weight 0\b"):
        C.layered_host(H0, J, L, Z, y)
    assert raw_host_call(C, who, J, L, Z, H1, y, 0, 5, ctypes.c_float(0.0), 0)[0] == -5  # the rows come before the arguments
    D = np.zeros((L * Z + 1, 2), np.int32)
    rc = C._lib.lib.bldpc_decode_layered_host(J, L, Z, H.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 2, 5,
                                              ctypes.c_float(1.0), 0, EXIT_PER_FRAME, STOP_PREFIX, D.ctypes.data_as(ctypes.c_void_p), None, None)
    assert rc == -1 and b"iters" in C._lib.lib.bldpc_last_error()
    assert C.STOP_PREFIX == 0 and C.STOP_SYNDROME == 1


# ---- the host statement under the host sanitizers, stand-alone ------------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


def build_cpp(name, tmp, flags):
    """tests/cpp/<name>.hip as a program in `tmp`, built as test_bp_cpu.py builds bp_host_test.hip."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp / name)
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + flags
                          + [os.path.join(here, "cpp", name + ".hip"), "-o", exe], cwd=str(tmp))
    return exe


@pytest.fixture(scope="module", params=list(SANITIZERS))
def layered_exe(request, tmp_path_factory):
    return build_cpp("layered_host_test", tmp_path_factory.mktemp("layered_host_" + request.param), SANITIZERS[request.param])


@pytest.mark.parametrize("dims", [(3, 5, 13), (5, 12, 96)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_host_statement_stand_alone(C, layered_exe, tmp_path, dims):
    """The input of bp_host_test.hip, alpha 0.75: the host statement gives the per-frame case stop iterations 1, 2, 3, 4, 5 and 10 on
    (3, 5, 13) and 1, 2, 3, 5 and 10 on (5, 12, 96)."""
    from test_bp_cpu import fnv64, generated_input  # these import this module
    from test_layered_shapes_cpu import SHAPES, matrix_of
    J, L, Z = dims
    H = matrix_of({x[:3]: x for x in SHAPES}[dims])
    path = str(tmp_path / "H.txt")
    np.savetxt(path, H, fmt="%d")
    F, alpha = 37, 0.75
    y = generated_input(L * Z, F)
    for mode, max_iter, rule in ((EXIT_FIXED, 5, STOP_PREFIX), (EXIT_PER_FRAME, 10, STOP_SYNDROME)):
        want = C.layered_host(H, J, L, Z, y, max_iter=max_iter, alpha=alpha, exit_mode=mode, stop_rule=rule)
        if mode == EXIT_PER_FRAME:
            assert np.unique(want["iters"]).size >= 2, "the generated input must hold frames that stop at different times"
        r = subprocess.run([layered_exe, path] + [str(a) for a in (J, L, Z, F, max_iter, alpha, mode, rule)], timeout=300, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT)
        out = r.stdout.decode()
        assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
        assert "Sanitizer" not in out and "runtime error" not in out, out
        tok = out.strip().split("\n")[-1].split()
        assert int(tok[0], 16) == fnv64(want["D"], want["app"], want["iters"]), "D, app or iters differ from what layered_host returned in Python"
        if len(os.sched_getaffinity(0)) > 1:
            assert int(tok[1]) > 1, "the frames ran on one thread: nothing for the race detector to see"


# ---- the tier rules ---------------------------------------------------------------------------------------------------------------------
def test_tier_choices_equal_the_parent_commit_under_host_sanitizers(tmp_path):
    """choose_tier of the three layered decoders (csrc/bldpc_layered_host.hpp, bldpc_bp_host.hpp, bldpc_quant_host.hpp, all over the
    one search of csrc/bldpc_layer_host.hpp), run by a stand-alone program under AddressSanitizer and UBSan over the grid of
    tests/golden/layer_tier_choices.json: J in {3, 4, 5, 6, 8, 12, 15, 32} times 16 values of Z from 1 to 1280, N % 64 zero and not,
    light and heavy rows, a shape just inside and just outside the LDS budget and the thread cap of every decoder, and the shipped
    matrices.  The file holds what the three separate choose_tier functions of the commit named in it chose: kernel, units per
    workgroup, threads, LDS bytes and the register variant's J.  Exact: integers."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_tier_choices.json")) as f:
        want = json.load(f)["cases"]
    assert len(want) > 1000
    for dec, names in (("layered", {"k_lay", "k_lay_reg", "k_lay_ws"}), ("bp", {"k_lbp", "k_lbp_ws"}), ("quant", {"k_lq", "k_lq_ws"})):
        assert {c[dec][0] for c in want.values()} == names, "the grid must reach every tier of " + dec
    exe = build_cpp("layer_tier_host_test", tmp_path, SANITIZERS["asan_ubsan"])
    inp = "".join("%d %d %d %d %d\n" % (c["J"], c["Z"], c["N"], c["M"], c["EZ"]) for c in want.values())
    r = subprocess.run([exe], input=inp.encode(), timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    lines = r.stdout.decode().strip().split("\n")
    assert r.returncode == 0 and lines[-1] == "OK %d" % len(want), r.stdout.decode()[-2000:]
    for (cid, c), line in zip(want.items(), lines):
        t = line.split()
        got = [[t[5 * k]] + [int(x) for x in t[5 * k + 1:5 * k + 5]] for k in range(3)]
        assert got == [c["layered"], c["bp"], c["quant"]], cid
