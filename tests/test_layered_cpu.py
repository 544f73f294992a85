"""The layered normalised min-sum decoder without a GPU: bldpc_decode_layered_host (plain C++, the statement of the semantics
inside the product) against a numpy restatement of the specification in include/bldpc.h written here (block-wise gathers,
np.signbit, sort + first argmin), bit for bit on hard bits and a-posteriori values; per-frame exit under both stop rules;
special values; alpha = 1; the convergence claim against flooding on the same noise; every refusal."""
import os

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


def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    J, L, Z = 4, 24, 96
    H = read_H("J4_L24_Z96_BlockH.txt", J, L)
    y = np.ones((L * Z, 2), np.float32)

    def refused(code, **kw):
        with pytest.raises(LdpcError, match=r"\(%d\): .*\S" % code):
            C.layered_host(kw.pop("H", H), J, L, Z, y, **kw)

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
    import ctypes
    D = np.zeros((L * Z + 1, 2), np.int32)
    rc = C._lib.lib.bldpc_decode_layered_host(J, L, Z, H.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 2, 5,
                                              ctypes.c_float(1.0), 0, EXIT_PER_FRAME, STOP_PREFIX, D.ctypes.data_as(ctypes.c_void_p), None, None)
    assert rc == -1 and b"iters" in C._lib.lib.bldpc_last_error()
    assert C.STOP_PREFIX == 0 and C.STOP_SYNDROME == 1
