"""Cases shared by tests/test_erasure_ml_cpu.py and tests/test_erasure_ml_gpu.py: the shapes, batch sizes and inputs of erasure decoding
by elimination (bldpc_decode_erasure_ml, include/bldpc.h) and a restatement of its definition that shares no code with the host
statement: elimination on Python integers as rows, and "determined" decided through a basis of the null space (an unknown is determined
iff no basis vector has it).  test_erasure_ml_cpu.py holds the host statement against the restatement and asserts the case table of the
inputs; test_erasure_ml_gpu.py holds the kernels against the host statement on the same cases.  Shapes, layout helpers and codewords are
those of erasure_cases.py."""
import numpy as np

from erasure_cases import (ALL_ERASED, BATCHES, EXTREME, F_MAX, RANDOM_KNOWN, X_COL0, X_COL0_VAR, codewords, dims_id, garbage_padding,  # noqa: F401
                           matrix, np_pack, np_syndrome, np_unpack)

ML_NONE, ML_SOLVED, ML_PARTIAL, ML_STUCK, ML_INCONSISTENT, ML_SKIPPED = range(6)
WORKSPACE_DIMS = (6, 12, 500)  # AUTO lands on the workspace tier at max_erased = M
DIMS = [(3, 5, 13), (4, 10, 7), (3, 7, 33), (3, 9, 96), EXTREME, WORKSPACE_DIMS]

# frames of the input that are not part of the ramp, beside erasure_cases.py's ALL_ERASED (2), RANDOM_KNOWN (3 .. 6) and X_COL0 (8)
PARTIAL_XOR = 10             # the support of the XOR of two codewords erased, and a few positions outside it
COUNTED = {11: 31, 12: 32, 13: 33, 14: 34}  # frame: erased positions.  With max_erased 31, 32 and 33 one is at the bound and one just above
HEAVY = {15: 2500, 16: 2900, 17: 3000, 18: 3001, 19: 3300}  # WORKSPACE_DIMS only: around M = 3000, where whole solutions end

# (step, seed, positions outside the support in PARTIAL_XOR, their seed): ramp frame f has int(f * step) erased positions drawn from `seed`.  The
# ramp ends near 1.3 M, beyond what elimination solves whole; on WORKSPACE_DIMS it stays light and HEAVY holds the large systems.
# Tuned on the CPU with the restatement until the case table holds (test_erasure_ml_cpu.py test_inputs_meet_their_conditions).
RAMP = {
    (3, 5, 13): (0.8, 1, 2, 1),
    (4, 10, 7): (0.58, 1, 2, 2),
    (3, 7, 33): (2.0, 1, 3, 2),
    (3, 9, 96): (3.0, 1, 3, 8),
    EXTREME: (0.5, 1, 3, 1),
    WORKSPACE_DIMS: (6.0, 1, 3, 1),
}

_cache = {}


def max_erased_values(dims):
    """The max_erased of the calls: the default (M), the three around a word of the row, and N."""
    return (0, 31, 32, 33, dims[1] * dims[2])


def _codewords(dims):
    """codewords(dims, F_MAX), computed once: the generator of the longest shape takes seconds."""
    key = ("cw", tuple(dims))
    if key not in _cache:
        _cache[key] = codewords(dims, F_MAX)
    return _cache[key]


def xor_support(dims):
    """(the support of the XOR of the two codewords of codewords() that differ in the fewest positions, the first of the two).  The
    fewest: on the longer shapes the XOR of two random codewords covers half of N, which is about all that elimination recovers."""
    key = ("xor", tuple(dims))
    if key in _cache:
        return _cache[key]
    cw = _codewords(dims).astype(np.int64)
    N = cw.shape[0]
    best = (N + 1, 0, 0)
    for a in range(F_MAX):
        d = (cw[:, a:a + 1] ^ cw).sum(0)
        d[d == 0] = N + 1
        b = int(d.argmin())
        if d[b] < best[0]:
            best = (int(d[b]), a, b)
    assert best[0] <= N, "codewords() holds one word only"
    _cache[key] = (np.flatnonzero(cw[:, best[1]] ^ cw[:, best[2]]), best[1])
    return _cache[key]


def partial_outside(dims):
    """The positions outside the support that PARTIAL_XOR erases as well."""
    N = dims[1] * dims[2]
    _, _, outside, xseed = RAMP[tuple(dims)]
    return np.random.default_rng(xseed).choice(np.setdiff1d(np.arange(N), xor_support(dims)[0]), size=outside, replace=False)


def ml_input(dims):
    """(bits int32 [N, F_MAX] with 0 at the erased positions, erased int32 [N, F_MAX], the words sent).  The frames of a smaller batch
    are its first columns."""
    dims = tuple(dims)
    key = ("in", dims)
    if key not in _cache:
        N = dims[1] * dims[2]
        step, seed = RAMP[dims][:2]
        cw = _codewords(dims).copy()
        rng = np.random.default_rng(seed)
        er = np.zeros((N, F_MAX), np.int32)
        for f in range(F_MAX):
            er[rng.choice(N, size=min(int(f * step), N), replace=False), f] = 1
        er[:, ALL_ERASED] = 1
        rk = np.random.default_rng(11)
        for f in RANDOM_KNOWN:
            cw[:, f] = rk.integers(0, 2, size=N)
            er[:, f] = 0
            er[rk.choice(N, size=min(N // 4, 12 + f), replace=False), f] = 1
        er[:, X_COL0] = 0
        if dims == EXTREME:
            er[X_COL0_VAR, X_COL0] = 1
        sup, first = xor_support(dims)
        cw[:, PARTIAL_XOR] = cw[:, first]
        er[:, PARTIAL_XOR] = 0
        er[sup, PARTIAL_XOR] = 1
        er[partial_outside(dims), PARTIAL_XOR] = 1
        counted = {**COUNTED, **(HEAVY if dims == WORKSPACE_DIMS else {})}
        for f, k in counted.items():
            er[:, f] = 0
            er[rng.choice(N, size=k, replace=False), f] = 1
        bits = cw * (1 - er)
        for a in (bits, er, cw):
            a.setflags(write=False)
        _cache[key] = (bits, er, cw)
    return _cache[key]


def ml_dirty_input(dims, F):
    """The packed words of the first F frames with garbage in the padding of both arrays and in the value bits of the erased positions."""
    bits, er, _ = ml_input(dims)
    g = np.random.default_rng(5).integers(0, 2, size=(bits.shape[0], F)).astype(np.int32)
    return garbage_padding(np_pack(bits[:, :F] | (g & er[:, :F])), F, seed=9), garbage_padding(np_pack(er[:, :F]), F, seed=10)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def row_variables(H, Z):
    """[M] arrays: the variables of check row j*Z + t are l*Z + (t + H[j, l]) % Z over the blocks of block row j."""
    H = np.asarray(H)
    J, L = H.shape
    t = np.arange(Z)
    rows = []
    for j in range(J):
        cols = [l * Z + (t + int(H[j, l])) % Z for l in range(L) if H[j, l] != -1]
        block = np.stack(cols, 1) if cols else np.zeros((Z, 0), np.int64)
        rows += [block[i] for i in range(Z)]
    return rows


def solve_frame(rows_v, x, er):
    """One frame on Python integers.  Returns (status without the bound, rank, determined positions, their values)."""
    cols = np.flatnonzero(er)
    e = len(cols)
    if e == 0:
        return ML_NONE, 0, cols, []
    idx = {int(v): i for i, v in enumerate(cols)}
    mask = (1 << e) - 1
    basis = {}  # lowest unknown of a row -> the row, right-hand side in bit e
    inconsistent = False
    for vs in rows_v:
        row = 0
        for v in vs.tolist():
            row ^= (1 << idx[v]) if er[v] else (int(x[v]) << e)
        while True:
            coef = row & mask
            if not coef:
                inconsistent |= bool(row >> e)
                break
            low = (coef & -coef).bit_length() - 1
            if low not in basis:
                basis[low] = row
                break
            row ^= basis[low]
    rank = len(basis)
    if inconsistent:
        return ML_INCONSISTENT, rank, cols[:0], []
    pivots = sorted(basis, reverse=True)
    pivot_mask = sum(1 << p for p in pivots)
    for p in pivots:  # back substitution, highest pivot first: every row loses the other pivots
        row = basis[p]
        other = row & pivot_mask & ~(1 << p)
        while other:
            q = (other & -other).bit_length() - 1
            row ^= basis[q]
            other = row & pivot_mask & ~(1 << p) & ~((1 << (q + 1)) - 1)
        basis[p] = row
    # a basis of the null space: one vector per free unknown j, itself and every pivot unknown whose row has j
    free = [j for j in range(e) if j not in basis]
    in_some_vector = 0
    for j in free:
        vec = 1 << j
        for p in pivots:
            if (basis[p] >> j) & 1:
                vec |= 1 << p
        in_some_vector |= vec
    det = [p for p in sorted(basis) if not (in_some_vector >> p) & 1]
    vals = [(basis[p] >> e) & 1 for p in det]  # the solution with every free unknown 0
    status = ML_SOLVED if rank == e else ML_PARTIAL if det else ML_STUCK
    return status, rank, cols[det], vals


def np_ml_all(dims):
    """The restatement on ml_input(dims) with no bound on e: dict(x [N, F_MAX], er [N, F_MAX], status, rank, e [F_MAX]), computed once."""
    dims = tuple(dims)
    key = ("ml", dims)
    if key not in _cache:
        H, Z = matrix(dims), dims[2]
        bits, er_in, _ = ml_input(dims)
        rows_v = row_variables(H, Z)
        x, er = bits.astype(np.int64), er_in.astype(np.int64)
        status, rank = np.zeros(F_MAX, np.int32), np.zeros(F_MAX, np.int32)
        for f in range(F_MAX):
            st, rk, pos, vals = solve_frame(rows_v, x[:, f].copy(), er[:, f].copy())
            status[f], rank[f] = st, rk
            x[pos, f] = vals
            er[pos, f] = 0
        _cache[key] = dict(x=x, er=er, status=status, rank=rank, e=er_in.sum(0))
    return _cache[key]


def np_outputs(dims, F, max_erased):
    """(D [N+1, F], E [N, F], status [F], rank [F]) of the first F frames at this max_erased (0: M): a frame above the bound is as it came."""
    H, Z = matrix(dims), dims[2]
    bits, er_in, _ = ml_input(dims)
    a = np_ml_all(dims)
    me = max_erased if max_erased else dims[0] * Z
    skip = a["e"][:F] > me
    x = np.where(skip[None], bits[:, :F], a["x"][:, :F])
    er = np.where(skip[None], er_in[:, :F], a["er"][:, :F])
    flag = ~er.any(0) & ~np_syndrome(np.asarray(H), Z, x.astype(np.int64)).any(0)
    D = np.concatenate([x, flag[None].astype(np.int64)], 0).astype(np.int32)
    return (D, er.astype(np.int32), np.where(skip, ML_SKIPPED, a["status"][:F]).astype(np.int32),
            np.where(skip, -1, a["rank"][:F]).astype(np.int32))
