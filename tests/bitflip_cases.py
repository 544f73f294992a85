"""Cases shared by tests/test_bitflip_cpu.py and tests/test_bitflip_gpu.py: the block matrices, batch sizes and inputs of the bit-flipping
decoder (bldpc_decode_bitflip, include/bldpc.h "hard-decision decoding"), the packed-bit layout in numpy, and an integer-only numpy
restatement of both rules that shares no code with the host statement.  test_bitflip_cpu.py holds the host statement against the
restatement and checks the condition on the inputs; test_bitflip_gpu.py holds the kernels against the host statement on the same cases."""
import numpy as np

from test_layered_shapes_cpu import SHAPES, matrix_of, random_blockh

BF_THRESHOLD, BF_GRADIENT = 0, 1
EXIT_FIXED, EXIT_BATCH_GLOBAL, EXIT_PER_FRAME = 0, 1, 2
RULES = (BF_THRESHOLD, BF_GRADIENT)
MAX_ITER = 10
BATCHES = (1, 33, 37, 64)  # one frame; one bit in the second word; a partly filled word; full words
F_MAX = max(BATCHES)
LDS_BOUND = 160 * 1024 - 1024  # the dynamic LDS a workgroup may ask for (bldpc_layer_host.hpp kLdsBytes)

_BY_DIMS = {s[:3]: s for s in SHAPES}
# the shapes of test_layered_shapes_cpu.py at which a mapping decision of k_bf can fail
_SHARED = [(3, 5, 13),     # N = 65 and Z < 32
           (4, 10, 7),
           (3, 7, 33),     # odd Z above a half-wave
           (3, 9, 96),     # N a multiple of 32 but not of 64
           (6, 12, 500),   # an uneven stride loop
           (3, 8, 1056),   # Z above 1024
           (4, 27, 64)]    # row weights 26, 2, 3 and 25
EXTREME = (17, 20, 24)     # block column weights 16, 1 and 0, a block row of weight 1
BOUND_JL = (3, 29)         # the two shapes at the LDS bound: Z from bitflip_plan_host's own figure (bound_shapes)

# (step, seed) of the error ramp per shape: frame f gets int(f * step) flipped bits at positions drawn from `seed`.  Tuned on the CPU
# until per-frame exit gives at least three distinct iteration counts, 1 and MAX_ITER among them, under both rules
# (test_bitflip_cpu.py test_inputs_meet_their_condition).
RAMP = {
    (3, 5, 13): (0.05, 1),
    (4, 10, 7): (0.1, 1),
    (3, 7, 33): (0.05, 1),
    (3, 9, 96): (0.05, 1),
    (6, 12, 500): (0.75, 1),
    (3, 8, 1056): (0.35, 2),
    (4, 27, 64): (0.05, 1),
    EXTREME: (0.1, 1),
    "bound": (0.1, 2),
}


def dims_id(d):
    return "J%d_L%d_Z%d" % tuple(d)


def extreme_matrix():
    """int32 [17, 20]: block column 0 has weight 16 (with the error bit u + e reaches 17: the fifth counter plane), block column 1 weight 1,
    block column 2 is all zero, block row 16 has weight 1; the other columns hold two to four blocks in rows 0 .. 15."""
    J, L, Z = EXTREME
    rng = np.random.default_rng(77)
    H = np.full((J, L), -1, np.int32)
    H[:16, 0] = rng.integers(0, Z, 16)
    H[3, 1] = 5
    H[16, 3] = Z - 1
    for l in range(3, L):
        for j in rng.choice(16, size=int(rng.integers(2, 5)), replace=False):
            H[j, l] = rng.integers(0, Z)
    w = (H != -1).sum(0)
    assert w[0] == 16 and w[1] == 1 and w[2] == 0 and (H[16] != -1).sum() == 1
    return H


_cache = {}


def bound_shapes():
    """((J, L, Z) of the largest Z whose state fits the LDS bound, (J, L, Z + 1)): read off bitflip_plan_host's figure."""
    if "bound" not in _cache:
        import cuda_ldpc_amd as C
        J, L = BOUND_JL
        Z = 64
        while C.bitflip_plan_host(random_blockh(J, L, Z + 1, 31), J, L, Z + 1)["lds_bytes"] <= LDS_BOUND:
            Z += 1
        assert Z > 64
        _cache["bound"] = ((J, L, Z), (J, L, Z + 1))
    return _cache["bound"]


def accepted_dims():
    return _SHARED + [EXTREME, bound_shapes()[0]]


def matrix(dims):
    dims = tuple(dims)
    if dims not in _cache:
        if dims in _BY_DIMS:
            H = matrix_of(_BY_DIMS[dims])
        elif dims == EXTREME:
            H = extreme_matrix()
        else:
            H = random_blockh(dims[0], dims[1], dims[2], 31)
        H = np.array(H, np.int32)
        H.setflags(write=False)
        _cache[dims] = H
    return _cache[dims]


# ---- the packed layout ------------------------------------------------------------------------------------------------------------------
def np_pack(b):
    """bits [rows, F] of 0 / 1 -> uint32 [rows, ceil(F/32)], frame f in bit f % 32 of word f // 32, padding 0."""
    b = np.asarray(b).astype(np.uint64)
    rows, F = b.shape
    W = (F + 31) // 32
    p = np.zeros((rows, W * 32), np.uint64)
    p[:, :F] = b
    return (p.reshape(rows, W, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def np_unpack(bits, F):
    bits = np.asarray(bits).astype(np.uint32)
    f = np.arange(F)
    return ((bits[:, f // 32] >> (f % 32).astype(np.uint32)) & 1).astype(np.int32)


def garbage_padding(bits, F, seed=9):
    """The same words with random bits in the padding of the last word of every row."""
    bits = np.array(bits, np.uint32)
    if F % 32:
        g = np.random.default_rng(seed).integers(0, 1 << 32, size=bits.shape[0], dtype=np.uint64).astype(np.uint32)
        bits[:, -1] |= g & np.uint32((0xFFFFFFFF << (F % 32)) & 0xFFFFFFFF)
    return bits


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------
def codewords(dims, F):
    """int32 [N, F]: random codewords from the host generator where it gives one with information bits, the all-zero word otherwise."""
    import cuda_ldpc_amd as C
    J, L, Z = dims
    N = L * Z
    if N > 8192:  # the generator's elimination is cubic: the long shapes send the all-zero word
        return np.zeros((N, F), np.int32)
    try:
        g = C.generator_host(matrix(dims), J, L, Z)
    except C._lib.LdpcError:
        return np.zeros((N, F), np.int32)
    K, pos = g["K_info"], g["info_pos"]
    msg = np.random.default_rng(1000 + N).integers(0, 2, size=(K, F)).astype(np.uint64)
    Pb = ((g["P"][:, np.arange(K) // 64] >> (np.arange(K) % 64).astype(np.uint64)) & np.uint64(1))  # [rank, K]
    par = (Pb @ msg) & np.uint64(1)
    cw = np.zeros((N, F), np.int32)
    cw[pos] = msg
    rest = np.setdiff1d(np.arange(N), pos)
    cw[rest[:par.shape[0]]] = par
    return cw


def ramp_input(dims, zero_word=False):
    """(received bits int32 [N, F_MAX], the word sent): an error ramp over the frames, frame f with int(f * step) flipped bits, frame 0
    with none.  The frames of a smaller batch are its first columns."""
    dims = tuple(dims)
    key = ("in", dims, zero_word)
    if key not in _cache:
        N = dims[1] * dims[2]
        step, seed = RAMP[dims] if dims in RAMP else RAMP["bound"]
        cw = np.zeros((N, F_MAX), np.int32) if zero_word else codewords(dims, F_MAX)
        rng = np.random.default_rng(seed)
        r = cw.copy()
        for f in range(F_MAX):
            k = min(int(f * step), N)
            r[rng.choice(N, size=k, replace=False), f] ^= 1
        if dims == EXTREME:  # frame 1: one error in the block column of weight 16, so that 16 checks fail at once (the fifth plane)
            r[:, 1] = cw[:, 1]
            r[0, 1] ^= 1
        r.setflags(write=False)
        cw.setflags(write=False)
        _cache[key] = (r, cw)
    return _cache[key]


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def np_syndrome(H, Z, x):
    """s [J*Z, F] of the bits x [N, F]: check row j*Z + t sums the variables l*Z + (t + H[j, l]) % Z."""
    J, L = H.shape
    s = np.zeros((J * Z, x.shape[1]), np.int64)
    for j in range(J):
        for l in range(L):
            if H[j, l] != -1:
                s[j * Z:(j + 1) * Z] ^= np.roll(x[l * Z:(l + 1) * Z], -int(H[j, l]), axis=0)
    return s


def np_bitflip(H, Z, r, max_iter, rule):
    """All frames at once, integers only.  Returns (x after every iteration [max_iter, N, F], flag after every iteration [max_iter, F])."""
    H = np.asarray(H)
    J, L = H.shape
    r = np.asarray(r).astype(np.int64)
    x = r.copy()
    d = np.repeat((H != -1).sum(0), Z)[:, None]
    xs, flags = [], []
    for _ in range(max_iter):
        s = np_syndrome(H, Z, x)
        active = s.any(0)  # the frames that flip at all
        u = np.zeros_like(x)
        for j in range(J):
            for l in range(L):
                if H[j, l] != -1:
                    u[l * Z:(l + 1) * Z] += np.roll(s[j * Z:(j + 1) * Z], int(H[j, l]), axis=0)
        e = x ^ r
        if rule == BF_THRESHOLD:
            flip = 2 * u + e > d
        else:
            E = u + e
            flip = E == E.max(0, keepdims=True)
        x = x ^ (flip & active[None, :])
        xs.append(x.copy())
        flags.append(~np_syndrome(H, Z, x).any(0))
    return np.stack(xs), np.stack(flags)


def np_outputs(xs, flags):
    """(D [N+1, F], per-frame iters [F]) from np_bitflip's history: a converged frame never flips again, so D is the last state in
    either mode; the per-frame count is the first iteration that leaves the flag set, or max_iter."""
    K = xs.shape[0]
    D = np.concatenate([xs[-1], flags[-1:].astype(np.int64)], 0).astype(np.int32)
    iters = np.where(flags.any(0), flags.argmax(0) + 1, K).astype(np.int32)
    return D, iters
