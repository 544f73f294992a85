"""Normalised min-sum on the flooding decoders without a GPU: bldpc_decode_normalised_host (plain C++, the statement of the
semantics inside the product, include/bldpc.h) against the CPU oracle at alpha = 1 and against a numpy restatement written here
(np_minsum of test_binary_crosscheck_cpu.py plus the one multiplication) at alpha < 1, bit for bit on hard bits, flag row and
a-posteriori sums; per-frame exit; the gain in unflagged frames; every refusal."""
import numpy as np
import pytest

import qc_variant_cases as Q

EXIT_FIXED, EXIT_BATCH_GLOBAL, EXIT_PER_FRAME = 0, 1, 2
MAXIT = 40

# (matrix of qc_variant_cases, Es/N0 dB, F)
MATRICES = [(("shipped", "J4_L24_Z96"), 2.7, 5), (("shipped", "J32_L64_Z64"), -0.9, 5), (("random", 96, 3, 9), 1.0, 5),
            (("shipped", "PON_LDPC"), 2.5, 2)]
IDS = ["_".join(str(x) for x in m[0][1:]) for m in MATRICES]


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def np_norm_minsum(H, Z, y, iters, alpha, length=0):
    """np_minsum with mag = alpha * (min2 on the first index of the minimum, else min1), one fp32 multiplication, then
    R = (float)(P * sg) * mag.  Returns (D [N+1, F] with the flag row of the last iteration, S [N, F])."""
    J, L = H.shape
    F = y.shape[1]
    wc = (H != -1).sum(1)
    Wc = int(wc.max())
    RQ = np.zeros((J * Z * Wc, F), np.float32)
    pos = np.cumsum(H != -1, axis=1) - 1
    c = np.arange(Z)
    slots = {(j, l): (j * Z + (c - H[j, l]) % Z) * Wc + pos[j, l] for j in range(J) for l in range(L) if H[j, l] != -1}
    S_all = np.zeros((L * Z, F), np.float32)
    al = np.float32(alpha)
    with np.errstate(all="ignore"):
        for it in range(1, iters + 1):
            for l in range(L):
                blocks = [slots[(j, l)] for j in range(J) if (j, l) in slots]
                R = [RQ[s] for s in blocks]
                S = np.zeros((Z, F), np.float32)
                for r in R:
                    S = S + r
                S = S + y[l * Z:(l + 1) * Z]
                S_all[l * Z:(l + 1) * Z] = S
                for s, r in zip(blocks, R):
                    RQ[s] = S - r
            if it == iters:
                break
            for j in range(J):
                w = int(wc[j])
                base = (j * Z + c) * Wc
                Qv = np.stack([RQ[base + i] for i in range(w)])
                sg = np.where(Qv < 0, -1, 1).astype(np.int32)
                a = np.where(Qv < 0, -Qv, Qv)
                P = np.prod(sg, axis=0)
                srt = np.sort(a, axis=0)
                min1, min2 = srt[0], srt[1]
                idx = np.argmax(a == min1[None], axis=0)
                for i in range(w):
                    mag = (al * np.where(idx == i, min2, min1)).astype(np.float32)
                    RQ[base + i] = (P * sg[i]).astype(np.float32) * mag
    length = length or (L - J) * Z
    d = (S_all < 0).astype(np.int32)
    flag = (~d[:length].any(0)).astype(np.int32)
    return np.concatenate([d, flag[None]], 0), S_all


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _host(C, spec, y, its, alpha, **kw):
    _, H, J, L, Z = Q.matrix(spec)
    return C.normalised_host(H, J, L, Z, y, max_iter=its, alpha=alpha, **kw)


@pytest.mark.parametrize("spec,snr,F", MATRICES, ids=IDS)
def test_host_equals_oracle_at_alpha_one(C, orc, spec, snr, F):
    _, _, _, L, Z = Q.matrix(spec)
    N = L * Z
    y = Q.channel(orc, spec, snr, F)
    oc = Q.ocode(orc, spec)
    for its in (1, 2, 3, 12):
        want = orc.bldpc_decode(oc, y, F, its, early_exit=0, want_app=True)
        got = _host(C, spec, y.reshape(N, F), its, 1.0)
        assert np.array_equal(got["D"].reshape(-1), want["D"]), "hard bits / flag row, %d iterations" % its
        assert same_bits(got["app"].reshape(-1), want["app"]), "a-posteriori bits, %d iterations" % its
        assert np.all(got["iters"] == its)
    Dw, appw, itw = Q.oracle_per_frame(orc, oc, y, F, MAXIT)
    got = _host(C, spec, y.reshape(N, F), MAXIT, 1.0, exit_mode=EXIT_PER_FRAME)
    assert np.array_equal(got["iters"], itw), (got["iters"], itw)
    assert np.array_equal(got["D"], Dw) and same_bits(got["app"], appw)


@pytest.mark.parametrize("spec,snr,F", MATRICES, ids=IDS)
def test_host_equals_numpy_restatement(C, orc, spec, snr, F):
    _, H, _, L, Z = Q.matrix(spec)
    N = L * Z
    y = Q.channel(orc, spec, snr, F).reshape(N, F)
    for alpha, its in ((0.75, 1), (0.75, 2), (0.75, 6), (0.8125, 3), (0.9, 5)):
        D, S = np_norm_minsum(H, Z, y, its, alpha)
        got = _host(C, spec, y, its, alpha)
        assert np.array_equal(got["D"], D), "hard bits / flag row, alpha %g, %d iterations" % (alpha, its)
        assert same_bits(got["app"], S), "a-posteriori bits, alpha %g, %d iterations" % (alpha, its)


@pytest.mark.parametrize("spec,snr,F", MATRICES, ids=IDS)
def test_special_values_and_denormal_products(C, spec, snr, F):
    """+-0, denormals, +-3e38 and tied +-0.5: alpha * 1e-41 and alpha * 3e-42 are denormal products that must not be flushed."""
    _, H, _, L, Z = Q.matrix(spec)
    N, F = L * Z, 3
    y = Q.special_values(N, F).reshape(N, F)
    for alpha in (0.75, 0.8125, 0.9):
        D, S = np_norm_minsum(H, Z, y, 6, alpha)
        got = _host(C, spec, y, 6, alpha)
        assert np.array_equal(got["D"], D) and same_bits(got["app"], S), "alpha %g" % alpha
    # every channel value denormal: every product alpha * min is denormal, and flushed products would leave S = y after 2 iterations
    y = np.full((N, 2), 1e-41, np.float32)
    y[::3, 0] = -3e-42
    D, S = np_norm_minsum(H, Z, y, 2, 0.75)
    got = _host(C, spec, y, 2, 0.75)
    assert np.array_equal(got["D"], D) and same_bits(got["app"], S)
    assert np.all(np.abs(S) < np.float32(1.2e-38)) and np.all(S[:, 1] > y[:, 1]), "the sums must hold denormal products"


def test_the_multiplication_is_exercised(C, orc):
    spec = ("shipped", "J4_L24_Z96")
    _, _, _, L, Z = Q.matrix(spec)
    N, F = L * Z, 8
    y = Q.channel(orc, spec, 2.7, F).reshape(N, F)
    a = _host(C, spec, y, 2, 1.0)["app"]
    b = _host(C, spec, y, 2, 0.75)["app"]
    differ = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    print("words that differ after 2 iterations: %d of %d" % (differ, N * F))
    assert differ > N * F // 2


@pytest.mark.parametrize("spec,snr,F", MATRICES[:3], ids=IDS[:3])
@pytest.mark.parametrize("length", [0, -1])
def test_per_frame_exit_is_consistent(C, orc, spec, snr, F, length):
    """Frame f of a per-frame run = a fixed run of iters[f] iterations on that frame alone; length = Z + 37 ends inside a block."""
    _, _, _, L, Z = Q.matrix(spec)
    N = L * Z
    length = Z + 37 if length < 0 else 0
    y = Q.channel(orc, spec, snr, F).reshape(N, F)
    got = _host(C, spec, y, MAXIT, 0.75, exit_mode=EXIT_PER_FRAME, length=length)
    assert got["iters"].min() >= 1 and got["iters"].max() <= MAXIT
    for f in range(F):
        one = _host(C, spec, np.ascontiguousarray(y[:, f:f + 1]), int(got["iters"][f]), 0.75, length=length)
        assert np.array_equal(one["D"][:, 0], got["D"][:, f]) and same_bits(one["app"][:, 0], got["app"][:, f]), "frame %d" % f
        assert got["D"][N, f] == 1 or got["iters"][f] == MAXIT
        if got["iters"][f] > 1:  # it did not stop earlier: the flag of the iteration before was down
            assert _host(C, spec, np.ascontiguousarray(y[:, f:f + 1]), int(got["iters"][f]) - 1, 0.75, length=length)["D"][N, 0] == 0


def test_the_gain_is_real(C, orc):
    """J4_L24_Z96 at 2.7 dB, 1024 frames of the seed (173, 173, 173), 50 fixed iterations: frames left unflagged.  A numpy
    restatement gave u(1.0) = 63 and u(0.75) = 11; inequalities only, so another libm in the channel generator cannot break it."""
    spec = ("shipped", "J4_L24_Z96")
    _, _, _, L, Z = Q.matrix(spec)
    N, F = L * Z, 1024
    y = Q.channel(orc, spec, 2.7, F).reshape(N, F)
    u = {}
    for alpha in (1.0, 0.75):
        u[alpha] = int((_host(C, spec, y, 50, alpha, want_app=False)["D"][N] == 0).sum())
    print("unflagged frames of %d: alpha 1.0: %d, alpha 0.75: %d" % (F, u[1.0], u[0.75]))
    assert u[1.0] >= 20
    assert 3 * u[0.75] <= u[1.0]


def test_refusals(C):
    from cuda_ldpc_amd._lib import LdpcError
    spec = ("shipped", "J4_L24_Z96")
    _, H, J, L, Z = Q.matrix(spec)
    N = L * Z
    y = np.ones((N, 2), np.float32)
    for alpha in (0.0, 1.25, float("nan"), -0.5, float("inf")):
        with pytest.raises(LdpcError, match="alpha"):
            C.normalised_host(H, J, L, Z, y, 3, alpha)
    with pytest.raises(LdpcError, match="max_iter"):
        C.normalised_host(H, J, L, Z, y, 0, 0.75)
    with pytest.raises(LdpcError, match="BATCH_GLOBAL"):
        C.normalised_host(H, J, L, Z, y, 3, 0.75, exit_mode=EXIT_BATCH_GLOBAL)
    with pytest.raises(LdpcError, match="exit_mode"):
        C.normalised_host(H, J, L, Z, y, 3, 0.75, exit_mode=7)
    with pytest.raises(LdpcError, match="length"):
        C.normalised_host(H, J, L, Z, y, 3, 0.75, length=N + 1)
    with pytest.raises(LdpcError, match="shift"):
        bad = H.copy()
        bad[0, 0] = Z
        C.normalised_host(bad, J, L, Z, y, 3, 0.75)
    with pytest.raises(ValueError):
        C.normalised_host(H, J, L, Z, y[:-1], 3, 0.75)
    assert C.normalised_host(H, J, L, Z, y, 3, 1.0, length=N)["D"][N].tolist() == [1, 1]
