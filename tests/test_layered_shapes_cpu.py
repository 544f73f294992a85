"""The layered decoder's host statement (bldpc_decode_layered_host) against the numpy restatement of test_layered_cpu.py on
random block matrices at the shapes the shipped matrices do not have: N not a multiple of 64 (and of 32), Z below 64 and not a
multiple of 32, Z above 1024, block-row weights 2, 3, 25, 26 and 27, shifts 0 and Z - 1, every `length` of the prefix rule.
The matrices, the input and the shape table are shared with tests/test_layered_shapes_gpu.py, which holds the device kernels
against the host statement on the same cases: this file is what vouches for that reference there."""
import numpy as np
import pytest

from test_layered_cpu import EXIT_PER_FRAME, STOP_PREFIX, STOP_SYNDROME, np_layer_pass, np_layered, np_syndrome_ok, same_bits

MAX_ITER = 10
F_RAMP = 37

# (J, L, Z, block-row weights or None, seed of the matrix, tier bldpc_decode_layered must pick -- None: the device refuses it)
SHAPES = [
    (3, 5, 13, None, 1, "k_lay_ws"),      # N = 65: one bit in the last word, Z < 64
    (4, 10, 7, None, 2, "k_lay_ws"),      # N = 70
    (3, 7, 33, None, 203, "k_lay_ws"),      # N = 231, odd Z just above 32
    (3, 9, 50, None, 4, "k_lay_ws"),      # N = 450, N % 32 = 2
    (3, 9, 96, None, 5, "k_lay_ws"),      # N = 864: N % 32 = 0 but N % 64 = 32
    (6, 12, 500, None, 6, "k_lay_ws"),    # N = 6000, Z > 256 and no multiple of 256: uneven t loop
    (3, 8, 1056, None, 7, "k_lay_ws"),    # Z just above 1024
    (4, 24, 8, None, 108, "k_lay_reg"),     # 8 frames in one wave
    (32, 36, 16, None, 9, "k_lay_reg"),   # J = 32 in registers, 4 frames in one wave
    (4, 10, 640, None, 10, "k_lay_reg"),  # 640-thread workgroups
    (4, 12, 1024, None, 11, "k_lay_reg"),  # 1024-thread workgroups
    (8, 16, 1000, None, 12, "k_lay_reg"),  # Z no multiple of 32: 24 idle lanes in the last wave
    (3, 16, 4, None, 213, "k_lay"),        # 16 frames in one wave
    (5, 8, 24, None, 14, "k_lay"),        # 8 frames over three waves, frames straddle the wave boundaries
    (5, 12, 32, None, 15, "k_lay"),       # row states in LDS, two frames per workgroup, one wave
    (5, 12, 96, None, 16, "k_lay"),       # row states in LDS, two frames per workgroup
    (3, 8, 1024, None, 17, "k_lay"),      # 1024 threads, row states in LDS
    (32, 34, 288, None, 18, "k_lay"),     # J = 32 too wide for the register variant
    (2, 27, 64, (26, 25), 19, "k_lay"),   # weights 26 and 25
    (4, 27, 64, (26, 2, 3, 25), 20, "k_lay_reg"),  # 26 next to the all-tail rows
    (3, 28, 64, (27, 5, 5), 21, None),    # weight 27: the host statement has no weight limit
]
SEVERAL_FRAMES_PER_WAVE = {(4, 24, 8), (32, 36, 16), (3, 16, 4), (5, 8, 24), (5, 12, 32)}


def shape_id(s):
    return "J%d_L%d_Z%d" % s[:3]


def random_blockh(J, L, Z, seed, weights=None, max_col=16):
    """int32 [J, L] block shifts, -1 = zero block, deterministic in `seed`.  Row j holds weights[j] blocks, or a random number in
    [2, min(L, 26)] of them; they sit at random columns with random shifts in [0, Z); every block column keeps at least one
    block (the columns are dealt to random rows first, then the rows are filled up) and at most `max_col`: 16 is the most a
    code object takes (bldpc_code_create_qc), which binds for J > 16 only -- there the random weights are capped such that the
    matrix exists, and a draw that can not be completed is drawn again.  The first block of the matrix in row-major order has
    shift 0 and the last one Z - 1: the two ends of the address rotation."""
    rng = np.random.default_rng(seed)
    hi = min(L, 26, L * max_col // J)
    while True:
        if weights is None:
            w = rng.integers(2, hi + 1, size=J)
            while w.sum() < L:  # too few blocks to cover the columns: one more in a random row that has room
                j = int(rng.choice(np.flatnonzero(w < hi)))
                w[j] += 1
        else:
            w = np.asarray(weights, np.int64)
            assert w.shape == (J,) and w.min() >= 1 and w.max() <= L and L <= w.sum() <= L * max_col
        rows = [[] for _ in range(J)]
        load = np.zeros(L, np.int64)
        for c in rng.permutation(L):
            j = int(rng.choice([j for j in range(J) if len(rows[j]) < w[j]]))
            rows[j].append(int(c))
            load[c] += 1
        ok = True
        for j in rng.permutation(J):
            free = [c for c in range(L) if c not in rows[j] and load[c] < max_col]
            need = int(w[j]) - len(rows[j])
            if need > len(free):
                ok = False
                break
            for c in rng.choice(free, size=need, replace=False) if need else []:
                rows[j].append(int(c))
                load[c] += 1
        if ok:
            break
    H = np.full((J, L), -1, np.int32)
    for j in range(J):
        H[j, rows[j]] = rng.integers(0, Z, size=len(rows[j]))
    nz = np.flatnonzero(H.reshape(-1) != -1)
    H.reshape(-1)[nz[0]] = 0
    H.reshape(-1)[nz[-1]] = Z - 1
    return H


def ramp_input(N, F):
    """The all-zero codeword with a noise ramp over the frames, y[:, f] = 1 + sigma_f * g, sigma_f from 0 to 1.3: frame 0 stops
    after the first iteration, the last frames never, and those in between at different iterations."""
    g = np.random.default_rng(5).standard_normal((N, F))
    return np.ascontiguousarray((1.0 + np.linspace(0.0, 1.3, F)[None, :] * g).astype(np.float32))


_H = {}


def matrix_of(s):
    """The shape's matrix: made once, shared by both test files, never written to."""
    if s[:3] not in _H:
        J, L, Z, weights, seed, _ = s
        H = random_blockh(J, L, Z, seed, weights)
        H.setflags(write=False)
        _H[s[:3]] = H
    return _H[s[:3]]


def np_history(H, Z, y, iters, alpha):
    """np_layered's loop (the same np_layer_pass) that keeps S after every iteration, float32 [iters, N, F]: the layer passes do
    not depend on the stop rule, so one run serves every rule and every `length`."""
    J, L = H.shape
    S = y.astype(np.float32).copy()
    R = {(j, l): np.zeros((Z, y.shape[1]), np.float32) for j in range(J) for l in range(L) if H[j, l] != -1}
    hist = np.empty((iters,) + y.shape, np.float32)
    with np.errstate(all="ignore"):
        for it in range(iters):
            np_layer_pass(H, Z, S, R, alpha)
            hist[it] = S
    return hist


def np_outputs(H, Z, hist, length, stop_rule):
    """What np_layered returns for this rule, (D, S, flags), and what per-frame exit must return, (D, S, iters): every frame as the
    first iteration with its flag set left it, or the last one."""
    iters, N, F = hist.shape
    length = length or N - H.shape[0] * Z
    if stop_rule == STOP_SYNDROME:
        flags = np.stack([np_syndrome_ok(H, Z, hist[it] < 0) for it in range(iters)]).astype(np.int32)
    else:
        flags = (~(hist[:, :length] < 0).any(1)).astype(np.int32)
    stop = np.where(flags.any(0), flags.argmax(0) + 1, iters).astype(np.int32)
    f = np.arange(F)
    Sp = hist[stop - 1, :, f].T
    D = np.concatenate([(hist[-1] < 0).astype(np.int32), flags[-1:]], 0)
    Dp = np.concatenate([(Sp < 0).astype(np.int32), flags[stop - 1, f][None]], 0)
    return (D, hist[-1], flags), (Dp, Sp, stop)


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def test_generator_keeps_its_promises():
    for s in SHAPES:
        J, L, Z, weights, seed, _ = s
        H = matrix_of(s)
        assert H.shape == (J, L) and H.dtype == np.int32 and H.min() >= -1 and H.max() < Z
        nz = H != -1
        w = nz.sum(1)
        if weights is None:
            assert w.min() >= 2 and w.max() <= min(L, 26)
        else:
            assert tuple(w) == tuple(weights)
        assert nz.sum(0).min() >= 1 and nz.sum(0).max() <= 16
        flat = H.reshape(-1)[nz.reshape(-1)]
        assert flat[0] == 0 and flat[-1] == Z - 1
        assert np.array_equal(H, random_blockh(J, L, Z, seed, weights)), "deterministic in the seed"
        assert not np.array_equal(H, random_blockh(J, L, Z, seed + 100, weights))
    ws = np.concatenate([(matrix_of(s) != -1).sum(1) for s in SHAPES])
    assert {2, 3, 25, 26, 27} <= set(ws.tolist())
    y = ramp_input(70, 5)
    assert y.dtype == np.float32 and (y[:, 0] == 1.0).all() and np.array_equal(y, ramp_input(70, 5))
    assert np.allclose(y.std(0), np.linspace(0, 1.3, 5), rtol=0.3)


@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_host_equals_numpy_on_random_shapes(C, s):
    J, L, Z = s[:3]
    H = matrix_of(s)
    N, K = L * Z, (L - J) * Z
    y = ramp_input(N, F_RAMP)
    for alpha in (0.75, 1.0):
        hist = np_history(H, Z, y, MAX_ITER, alpha)
        D, S, flags = np_layered(H, Z, y, MAX_ITER, alpha, stop_rule=STOP_SYNDROME)  # the history is np_layered's
        fixed, _ = np_outputs(H, Z, hist, 0, STOP_SYNDROME)
        assert np.array_equal(fixed[0], D) and same_bits(fixed[1], S) and np.array_equal(fixed[2], flags)
        for rule, lengths in ((STOP_SYNDROME, (0,)), (STOP_PREFIX, (0, 1, K - 1, N))):
            for length in lengths:
                what = "alpha %g, rule %d, length %d" % (alpha, rule, length)
                (D, S, flags), (Dp, Sp, want_it) = np_outputs(H, Z, hist, length, rule)
                if rule == STOP_SYNDROME or length in (0, N):  # a condition on the input, judged by the restatement
                    assert want_it[0] == 1 and (want_it < MAX_ITER).any() and (want_it == MAX_ITER).any(), \
                        "the batch must hold frames that stop and frames that never do: " + what
                    assert (flags[:-1, want_it == MAX_ITER] == 0).all()
                got = C.layered_host(H, J, L, Z, y, max_iter=MAX_ITER, alpha=alpha, length=length, stop_rule=rule)
                assert np.array_equal(got["D"], D), "hard bits / flag row: " + what
                assert same_bits(got["app"], S), "a-posteriori bits: " + what
                assert (got["iters"] == MAX_ITER).all(), what
                got = C.layered_host(H, J, L, Z, y, max_iter=MAX_ITER, alpha=alpha, length=length, exit_mode=EXIT_PER_FRAME,
                                     stop_rule=rule)
                assert np.array_equal(got["iters"], want_it), "per-frame exit, iters: " + what
                assert np.array_equal(got["D"], Dp), "per-frame exit, hard bits / flag row: " + what
                assert same_bits(got["app"], Sp), "per-frame exit, a-posteriori bits: " + what


def test_weight_27_is_refused_where_the_code_object_is_made(C):
    """bldpc_decode_layered's own limit of 26 blocks per block row equals the limit of bldpc_code_create_qc, which therefore
    refuses such a matrix before the decoder sees it (no device is touched before that verdict); the host statement takes it."""
    from cuda_ldpc_amd._lib import LdpcError
    J, L, Z = 3, 28, 64
    H = matrix_of(SHAPES[-1])
    assert (H != -1).sum(1).max() == 27
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*\S"):
            C.BinaryCode.from_shifts(H, J, L, Z)
    y = ramp_input(L * Z, 2)
    assert C.layered_host(H, J, L, Z, y, max_iter=2)["iters"].tolist() == [2, 2]
