"""Cases shared by tests/test_erasure_cpu.py and tests/test_erasure_gpu.py: the block matrices, batch sizes and inputs of the peeling
decoder (bldpc_decode_erasure, include/bldpc.h "erasure decoding") and an integer-only numpy restatement of its definition that shares no
code with the host statement.  test_erasure_cpu.py holds the host statement against the restatement and checks the conditions on the
inputs; test_erasure_gpu.py holds the kernels against the host statement on the same cases.  Shapes, layout helpers and codewords are
those of bitflip_cases.py."""
import numpy as np

from bitflip_cases import (_SHARED, BATCHES, BOUND_JL, EXTREME, F_MAX, LDS_BOUND, codewords, dims_id, garbage_padding, matrix,  # noqa: F401
                           np_pack, np_syndrome, np_unpack)
from test_layered_shapes_cpu import random_blockh

MAX_ITER = 64  # above the longest peeling chain of every ramp below (52): every frame ends by itself

# frames of the input that are not part of the ramp
ALL_ERASED = 2            # every position erased: flag 0, and iters 0 unless a block row has weight 1 (EXTREME)
RANDOM_KNOWN = (3, 4, 5, 6)  # known bits random, no codeword: the checks disagree, the OR rule decides
X_ROW1, X_COL0, X_COL16 = 7, 8, 9  # EXTREME only: the weight-1 block row, the weight-0 and the weight-16 block column
X_ROW1_VAR = 3 * 24 + 5   # a variable of block column 3, whose block in block row 16 is that row's only one
X_COL0_VAR = 2 * 24 + 7   # a variable of the all-zero block column 2
X_COL16_VAR = 0 * 24 + 3  # a variable of block column 0, weight 16

# (step, seed, seed of the random-known frames) per shape: ramp frame f has int(f * step) erased positions drawn from `seed`.  Tuned on
# the CPU with the restatement until iters takes at least three distinct values, 0 among them, and at least one frame ends with erasures
# left after one or more productive iterations (test_erasure_cpu.py test_inputs_meet_their_conditions).
RAMP = {
    (3, 5, 13): (0.567, 1, 11),
    (4, 10, 7): (0.278, 1, 11),
    (3, 7, 33): (1.283, 1, 11),
    (3, 9, 96): (0.8, 1, 11),
    (6, 12, 500): (42.857, 1, 11),
    (3, 8, 1056): (46.933, 1, 11),
    (4, 27, 64): (1.5, 1, 11),
    EXTREME: (1.0, 1, 11),
    "bound": (10.0, 1, 11),
}

_cache = {}


def bound_shapes():
    """((J, L, Z) of the largest Z whose state fits the LDS bound, (J, L, Z + 1)): read off erasure_plan_host's figure."""
    if "bound" not in _cache:
        import cuda_ldpc_amd as C
        J, L = BOUND_JL
        Z = 64
        while C.erasure_plan_host(random_blockh(J, L, Z + 1, 31), J, L, Z + 1)["lds_bytes"] <= LDS_BOUND:
            Z += 1
        assert Z > 64
        _cache["bound"] = ((J, L, Z), (J, L, Z + 1))
    return _cache["bound"]


def accepted_dims():
    return _SHARED + [EXTREME, bound_shapes()[0]]


def ramp_frames():
    fixed = {ALL_ERASED, X_ROW1, X_COL0, X_COL16} | set(RANDOM_KNOWN)
    return [f for f in range(F_MAX) if f not in fixed]


def erased_input(dims):
    """(bits int32 [N, F_MAX] with 0 at the erased positions, erased int32 [N, F_MAX], the words sent): the erasure ramp over the frames
    with the fixed frames of this file at their indices.  The frames of a smaller batch are its first columns."""
    dims = tuple(dims)
    key = ("in", dims)
    if key not in _cache:
        N = dims[1] * dims[2]
        step, seed, rk_seed = RAMP[dims] if dims in RAMP else RAMP["bound"]
        cw = codewords(dims, F_MAX).copy()
        rng = np.random.default_rng(seed)
        er = np.zeros((N, F_MAX), np.int32)
        for f in range(F_MAX):
            er[rng.choice(N, size=min(int(f * step), N), replace=False), f] = 1
        er[:, ALL_ERASED] = 1
        rk = np.random.default_rng(rk_seed)
        for f in RANDOM_KNOWN:
            cw[:, f] = rk.integers(0, 2, size=N)
            er[:, f] = 0
            er[rk.choice(N, size=min(N, max(2, int(20 * step))), replace=False), f] = 1
        for f, v in ((X_ROW1, X_ROW1_VAR), (X_COL0, X_COL0_VAR), (X_COL16, X_COL16_VAR)):
            er[:, f] = 0
            if dims == EXTREME:
                er[v, f] = 1
        bits = cw * (1 - er)
        for a in (bits, er, cw):
            a.setflags(write=False)
        _cache[key] = (bits, er, cw)
    return _cache[key]


def dirty_input(dims, F):
    """The packed words of the first F frames with garbage in the padding of both arrays and in the value bits of the erased positions."""
    bits, er, _ = erased_input(dims)
    g = np.random.default_rng(5).integers(0, 2, size=(bits.shape[0], F)).astype(np.int32)
    return garbage_padding(np_pack(bits[:, :F] | (g & er[:, :F])), F, seed=9), garbage_padding(np_pack(er[:, :F]), F, seed=10)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def np_peel(H, Z, bits, erased, max_iter):
    """All frames at once, integers only.  Returns dict(x, er: the state after every iteration [max_iter, N, F]; prod: the iteration
    resolved something [max_iter, F]; split: variables that were resolved by checks with different values, per frame [F])."""
    H = np.asarray(H)
    J, L = H.shape
    er = np.asarray(erased).astype(np.int64) & 1
    x = (np.asarray(bits).astype(np.int64) & 1) & (1 - er)
    F = x.shape[1]
    xs, ers, prod = [], [], []
    split = np.zeros(F, np.int64)
    blocks = [(j, l, int(H[j, l])) for j in range(J) for l in range(L) if H[j, l] != -1]
    for _ in range(max_iter):
        n = np.zeros((J * Z, F), np.int64)
        a = np.zeros((J * Z, F), np.int64)
        for j, l, s in blocks:  # check row j*Z + t has the variable l*Z + (t + s) % Z
            n[j * Z:(j + 1) * Z] += np.roll(er[l * Z:(l + 1) * Z], -s, axis=0)
            a[j * Z:(j + 1) * Z] ^= np.roll(x[l * Z:(l + 1) * Z] * (1 - er[l * Z:(l + 1) * Z]), -s, axis=0)
        one = (n == 1).astype(np.int64)
        hits = np.zeros_like(x)  # checks with one erasure at this variable, and how many of them carry a 1
        ones = np.zeros_like(x)
        for j, l, s in blocks:
            hits[l * Z:(l + 1) * Z] += np.roll(one[j * Z:(j + 1) * Z], s, axis=0)
            ones[l * Z:(l + 1) * Z] += np.roll(one[j * Z:(j + 1) * Z] * a[j * Z:(j + 1) * Z], s, axis=0)
        res = (hits > 0) & (er == 1)
        split += (res & (ones > 0) & (ones < hits)).sum(0)
        x = np.where(res, (ones > 0).astype(np.int64), x)
        er = er * (1 - res)
        xs.append(x.astype(np.int8))  # the history is kept small: 64 iterations of the shape at the bound
        ers.append(er.astype(np.int8))
        prod.append(res.any(0))
    return dict(x=np.stack(xs), er=np.stack(ers), prod=np.stack(prod), split=split)


def np_outputs(H, Z, h, k=None):
    """(D [N+1, F], E [N, F], iters [F]) after k iterations (None: all) of np_peel's history."""
    k = h["x"].shape[0] if k is None else k
    x, er = h["x"][k - 1].astype(np.int64), h["er"][k - 1].astype(np.int64)
    flag = ~er.any(0) & ~np_syndrome(np.asarray(H), Z, x).any(0)
    D = np.concatenate([x, flag[None].astype(np.int64)], 0).astype(np.int32)
    return D, er.astype(np.int32), h["prod"][:k].sum(0).astype(np.int32)  # productive iterations are a prefix: their count is the last index
