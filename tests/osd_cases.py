"""Cases shared by tests/test_osd_cpu.py and tests/test_osd_gpu.py: the shapes, batch sizes and inputs of ordered-statistics
reprocessing (bldpc_decode_osd, include/bldpc.h) and a restatement of its definition that shares no code with the host statement: the
columns of H as Python integers, a greedy walk in sorted((key, v)) order that tests independence by reducing the column against the
basis so far, then a solve by reducing the syndrome against the same basis.  test_osd_cpu.py holds the host statement against the
restatement and asserts what the fixed frames are for; test_osd_gpu.py holds the kernels against the host statement on the same cases.
Shapes, codewords and np_syndrome are those of erasure_ml_cases.py, and one shape more whose matrix is rank deficient."""
import numpy as np

import bitflip_cases
from erasure_ml_cases import DIMS as ML_DIMS
from erasure_ml_cases import BATCHES, EXTREME, F_MAX, WORKSPACE_DIMS, _codewords, dims_id, matrix, np_syndrome, row_variables  # noqa: F401

DEFICIENT = (4, 9, 11)  # every block present: every column has weight 4, so the check rows sum to zero and rank(H) < M
DIMS = ML_DIMS + [DEFICIENT]


def deficient_matrix():
    J, L, Z = DEFICIENT
    H = np.random.default_rng(41).integers(0, Z, size=(J, L)).astype(np.int32)
    H.setflags(write=False)
    return H


bitflip_cases._cache.setdefault(DEFICIENT, deficient_matrix())  # matrix(DEFICIENT), and with it the shared codewords, are of this one

# frames of the input that are not part of the noise ramp
CODEWORD = 2      # y already a codeword: flips == 0
ALL_PLUS_ZERO = 3  # every value +0.0: y = 0, every key ties, the order is the positions
MIXED_ZEROS = 4   # +0.0 and -0.0: y = 0 everywhere all the same
SMALL_INTS = 5    # integers -3 .. 3: nearly every key ties
INF_AND_BIG = 6   # +-inf and values of magnitude 1e4
RELIABLE_WRONG = 7  # the word sent with one position wrong at magnitude 50: the result is another codeword
FIXED = (CODEWORD, ALL_PLUS_ZERO, MIXED_ZEROS, SMALL_INTS, INF_AND_BIG, RELIABLE_WRONG)
SIGMA = (0.3, 1.2)  # the ramp: frame f has noise of standard deviation SIGMA[0] + (SIGMA[1] - SIGMA[0]) f / (F_MAX - 1)
WORKSPACE_PROCESSED = 8  # WORKSPACE_DIMS: at most this many frames of a call are processed (a frame costs seconds in the restatement)

_cache = {}


def osd_input(dims):
    """(app float32 [N, F_MAX], the words sent int32 [N, F_MAX]).  The frames of a smaller batch are its first columns."""
    dims = tuple(dims)
    key = ("in", dims)
    if key not in _cache:
        N = dims[1] * dims[2]
        cw = _codewords(dims)
        rng = np.random.default_rng(2000 + N)
        sig = np.linspace(SIGMA[0], SIGMA[1], F_MAX)
        app = (1.0 - 2.0 * cw + rng.standard_normal((N, F_MAX)) * sig[None, :]).astype(np.float32)
        app[:, CODEWORD] = ((1.0 - 2.0 * cw[:, CODEWORD]) * rng.uniform(0.1, 2.0, N)).astype(np.float32)
        app[:, ALL_PLUS_ZERO] = 0.0
        app[:, MIXED_ZEROS] = np.where(rng.integers(0, 2, N) == 1, np.float32(-0.0), np.float32(0.0))
        app[:, SMALL_INTS] = rng.integers(-3, 4, N).astype(np.float32)
        big = (1.0 - 2.0 * cw[:, INF_AND_BIG]) * np.where(rng.integers(0, 2, N) == 1, np.inf, 1.0e4)
        big[rng.choice(N, size=max(2, N // 16), replace=False)] *= -1.0  # wrong and as reliable as anything
        app[:, INF_AND_BIG] = big.astype(np.float32)
        wrong = (1.0 - 2.0 * cw[:, RELIABLE_WRONG]) * rng.uniform(0.5, 2.0, N)
        wrong[reliable_wrong_position(dims)] *= -50.0
        app[:, RELIABLE_WRONG] = wrong.astype(np.float32)
        app.setflags(write=False)
        _cache[key] = (app, cw)
    return _cache[key]


def reliable_wrong_position(dims):
    """A position of RELIABLE_WRONG that no basis needs: one of block column 0, which has a block on every shape.  EXTREME has rank 408
    on 456 positions that are in a check, so nearly every one joins: there it is a position of the empty block column 2, which never
    does (flipping it in a codeword gives a codeword)."""
    return 2 * dims[2] + 7 if tuple(dims) == EXTREME else 1


def kept_input(dims, F):
    """D_in int32 [N+1, F] for the first F frames: about half the frames kept (flag row not 0: 1, and other values), the kept columns of
    arbitrary content; on WORKSPACE_DIMS all but WORKSPACE_PROCESSED frames are kept.  The fixed frames are never kept."""
    dims = tuple(dims)
    N = dims[1] * dims[2]
    rng = np.random.default_rng(77)
    D = rng.integers(-5, 6, size=(N + 1, F_MAX)).astype(np.int32)
    keep = rng.integers(0, 2, F_MAX) == 1
    keep[list(FIXED)] = False
    keep[0] = False   # a lone frame (F = 1) is processed
    keep[1] = True
    if dims == WORKSPACE_DIMS:
        keep[:] = True
        keep[processed_on_workspace()] = False
    D[N] = np.where(keep, np.where(np.arange(F_MAX) % 3 == 0, 1, np.arange(F_MAX) + 2), 0)
    return np.ascontiguousarray(D[:, :F])


def processed_on_workspace():
    """The frames of WORKSPACE_DIMS that a call processes: the fixed ones, a clean and a noisy ramp frame."""
    return list(FIXED) + [0, 36]


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def columns(H, Z):
    """[N] Python integers: bit c of entry v is set iff check row c has variable v."""
    rows_v = row_variables(H, Z)
    N = np.asarray(H).shape[1] * Z
    cols = [0] * N
    for c, vs in enumerate(rows_v):
        for v in vs.tolist():
            cols[v] ^= 1 << c
    return cols


def osd_frame(cols, M, a):
    """One frame on Python integers.  a: float32 [N].  Returns (c int [N], flips, scanned, B as a list of positions)."""
    a = np.ascontiguousarray(a, np.float32)
    y = (a < 0).astype(np.int64)
    keys = (a.view(np.uint32) & np.uint32(0x7FFFFFFF)).tolist()
    order = sorted((k, v) for v, k in enumerate(keys))
    basis = {}  # lowest check of a reduced column -> (the reduced column, the members of B it is the sum of, as bits by order of joining)
    B = []
    scanned = 0
    for place, (_, v) in enumerate(order):
        vec, combo = cols[v], 1 << len(B)
        while vec:
            low = (vec & -vec).bit_length() - 1
            if low not in basis:
                basis[low] = (vec, combo)
                B.append(v)
                scanned = place + 1
                break
            vec ^= basis[low][0]
            combo ^= basis[low][1]
        if len(B) == M:
            break
    s = 0
    for v in np.flatnonzero(y).tolist():
        s ^= cols[v]
    combo = 0
    while s:
        low = (s & -s).bit_length() - 1
        assert low in basis, "the syndrome is in the column space"
        s ^= basis[low][0]
        combo ^= basis[low][1]
    c = y.copy()
    flips = 0
    for i, v in enumerate(B):
        if (combo >> i) & 1:
            c[v] ^= 1
            flips += 1
    return c, flips, scanned, B


def np_osd_all(dims):
    """The restatement on osd_input(dims), every frame processed (on WORKSPACE_DIMS only processed_on_workspace(); the rest holds -99):
    dict(c [N, F_MAX], flips, scanned [F_MAX], B: frame -> positions), computed once."""
    dims = tuple(dims)
    key = ("osd", dims)
    if key not in _cache:
        J, L, Z = dims
        app, _ = osd_input(dims)
        cols = columns(matrix(dims), Z)
        N = L * Z
        c = np.full((N, F_MAX), -99, np.int32)
        flips, scanned, B = np.full(F_MAX, -99, np.int32), np.full(F_MAX, -99, np.int32), {}
        for f in (processed_on_workspace() if dims == WORKSPACE_DIMS else range(F_MAX)):
            c[:, f], flips[f], scanned[f], B[f] = osd_frame(cols, J * Z, app[:, f])
        _cache[key] = dict(c=c, flips=flips, scanned=scanned, B=B)
    return _cache[key]


def np_outputs(dims, F, D_in=None):
    """(D [N+1, F], flips [F], scanned [F]) of the first F frames: processed where D_in is None or its flag row is 0, kept elsewhere."""
    a = np_osd_all(dims)
    N = dims[1] * dims[2]
    D = np.concatenate([a["c"][:, :F], np.ones((1, F), np.int32)], 0).astype(np.int32)
    flips, scanned = a["flips"][:F].copy(), a["scanned"][:F].copy()
    if D_in is not None:
        kept = D_in[N] != 0
        D[:, kept] = D_in[:, kept]
        flips[kept], scanned[kept] = -1, 0
    assert (D[:N] != -99).all() and (flips != -99).all(), "a frame of WORKSPACE_DIMS outside processed_on_workspace() is processed"
    return D, flips, scanned
