"""The case tables of tests/test_enc_shapes_cpu.py and tests/test_enc_shapes_gpu.py: generated codes at the shapes the shipped
matrices do not have, for the two encoders and syndrome checks (csrc/bldpc_encode.hip, csrc/nbldpc_encode.hip), and an independent
numpy restatement of the systematic generator both tests compare with.

The reference.  Both host generators search the pivots from the right, which makes the result unique: column c is a parity position
exactly when it is linearly independent of the columns to its right, and P is the fully reduced matrix restricted to the information
columns.  ref_gf2 / ref_gfq restate that on the dense H, one column at a time (for c from N - 1 down to 0: the first unused row with
a nonzero in column c; normalise it; clear column c from every other row), knowing nothing of the product's panels or threads.

Binary cases: seeded random block matrices in which every block column keeps at least one block and no block row more than 26 (the
most a code object takes).  GF(q) cases: the 18 codes of nb_shape_cases.py, a rank-deficient twin of each (last row = a nonzero
multiple of row 0) and four larger codes.  Everything is deterministic in the seeds, files are written once into a temporary
directory, and the reference results are computed once per case and shared; nothing here is written to after it was made."""
import collections
import os
import tempfile

import numpy as np

import nb_shape_cases as S

_TMP = tempfile.TemporaryDirectory(prefix="enc_shape_cases_")
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


# ---- digest (what tests/cpp/encoder_host_test.hip prints) ---------------------------------------------------------------------------
_FNV_OFFSET, _FNV_PRIME, _M64 = 0xCBF29CE484222325, 0x100000001B3, (1 << 64) - 1


def _fnv_rows(a):
    """FNV-1a 64 of every row of a uint8 [R, C] array -> uint64 [R]; the rows side by side, one numpy step per byte column."""
    h = np.full(a.shape[0], _FNV_OFFSET, np.uint64)
    at = np.ascontiguousarray(a.T).astype(np.uint64)
    with np.errstate(over="ignore"):
        for j in range(at.shape[0]):
            h = (h ^ at[j]) * np.uint64(_FNV_PRIME)
    return h


def digest(info_pos, P):
    """FNV-1a 64 over the bytes of info_pos (int32), continued over the 8 bytes of the FNV-1a 64 digest of every row of P in turn."""
    P = np.ascontiguousarray(P)
    rows = _fnv_rows(P.view(np.uint8).reshape(P.shape[0], -1))
    h = _FNV_OFFSET
    for b in np.asarray(info_pos).astype("<i4").tobytes() + rows.astype("<u8").tobytes():
        h = ((h ^ b) * _FNV_PRIME) & _M64
    return h


# ---- GF(2) ---------------------------------------------------------------------------------------------------------------------------
def block_matrix(J, L, Z, seed, density=0.6, dup=False, max_row=26):
    """int32 [J, L] block shifts, -1 = zero block, deterministic in `seed`: each block present with probability `density`, then every
    block column is given a block where it has none (in the lightest row) and every block row at least two and at most `max_row`
    (surplus blocks leave columns that hold another).  dup: the last block row repeats the first."""
    rng = np.random.default_rng(seed)
    on = rng.random((J, L)) < density
    for l in range(L):
        if not on[:, l].any():
            on[int(np.argmin(on.sum(1))), l] = True
    for j in range(J):
        while on[j].sum() > max_row:
            spare = [l for l in np.flatnonzero(on[j]) if on[:, l].sum() > 1]
            on[j, int(rng.choice(spare))] = False
        while on[j].sum() < 2:
            on[j, int(rng.choice(np.flatnonzero(~on[j])))] = True
    H = np.where(on, rng.integers(0, Z, size=(J, L)), -1).astype(np.int32)
    if dup:
        H[J - 1] = H[0]
    return H


def dense_h2(H, J, L, Z):
    """uint8 [M, N]: column c of a block with shift s meets row (c - s) mod Z (the convention of test_encoder_cpu.syndrome_np)."""
    A = np.zeros((J * Z, L * Z), np.uint8)
    c = np.arange(Z)
    for j in range(J):
        for l in range(L):
            s = int(H[j, l])
            if s != -1:
                A[j * Z + (c - s) % Z, l * Z + c] = 1
    return A


def ref_gf2(H, J, L, Z):
    """dict(K_info, rank, info_pos=int32 [K'], P=uint64 [rank, ceil(K'/64)]) in the layout of bldpc.generator_host, by plain
    Gauss-Jordan on byte-packed rows, pivot columns from the right."""
    N, M = L * Z, J * Z
    A = np.packbits(dense_h2(H, J, L, Z), axis=1, bitorder="little")
    used = np.zeros(M, bool)
    row_of = np.full(N, -1)
    for c in range(N - 1, -1, -1):
        col = (A[:, c >> 3] >> (c & 7)) & 1
        cand = np.flatnonzero(col.astype(bool) & ~used)
        if not cand.size:
            continue
        p = int(cand[0])
        used[p] = True
        row_of[c] = p
        rows = np.flatnonzero(col)
        A[rows[rows != p]] ^= A[p]
    info = np.flatnonzero(row_of < 0).astype(np.int32)
    par = np.flatnonzero(row_of >= 0)
    K, rank = len(info), len(par)
    bits = np.unpackbits(A[row_of[par]], axis=1, bitorder="little")[:, :N][:, info]
    padded = np.zeros((rank, (K + 63) // 64 * 64), np.uint8)
    padded[:, :K] = bits
    P = np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(rank, (K + 63) // 64)
    return dict(K_info=K, rank=rank, info_pos=info, P=P)


# id: (J, L, Z, seed, density, dup).  The property each case must have is asserted, from ref_gf2 alone, by
# test_enc_shapes_cpu.py::test_binary_case_has_its_property; a seed that does not give it is replaced, never the assertion.
BCase = collections.namedtuple("BCase", "id J L Z seed density dup")
BCASES = [
    BCase("tiny", 3, 8, 2, 1, 0.6, False),          # N = 16, K' < 16
    BCase("k_lt_64", 3, 5, 13, 2, 0.6, False),      # N = 65, 0 < K' < 64, rank < 64, M = 39: one syndrome slice over three block rows
    BCase("n_500", 2, 5, 100, 3, 1.0, False),       # N mod 64 != 0, K' mod 64 not in {0, 1}, scattered info_pos
    BCase("kw_33", 2, 35, 64, 4, 0.6, False),       # ceil(K'/64) = 33: one live word in the second register tile
    BCase("kw_34_odd", 2, 36, 63, 7, 0.7, False),   # ceil(K'/64) = 34, rank mod 4 != 0, N mod 64 != 0, scattered info_pos
    BCase("dup_row", 3, 5, 17, 6, 0.8, True),       # rank <= M - Z
    BCase("lds_full", 2, 42, 512, 7, 0.3, False),   # K' = 20 480 exactly: 160 KiB of slices (a block row holds at most 26 blocks: J = 2)
    BCase("lds_over", 2, 43, 512, 8, 0.3, False),   # lds_full and one block column more: 20 480 < K', refused by the encoder
]
B_BY_ID = {c.id: c for c in BCASES}
B_IDS = [c.id for c in BCASES]
LDS_MAX_INFO_BITS = 20480  # 160 KiB / (64 frames x 8 bytes per 64 information bits) x 64


def bin_h(cid):
    """int32 [J, L] of the case, made once (read-only)."""
    def make():
        c = B_BY_ID[cid]
        if cid == "lds_over":  # lds_full with one more block column: one block, in the lighter block row, at a seeded shift
            base = bin_h("lds_full")
            col = np.full((c.J, 1), -1, np.int32)
            col[int(np.argmin((base >= 0).sum(1))), 0] = np.random.default_rng(c.seed).integers(0, c.Z)
            H = np.hstack([base, col])
        else:
            H = block_matrix(c.J, c.L, c.Z, c.seed, c.density, c.dup)
        H.setflags(write=False)
        return H
    return _memo(("bin_h", cid), make)


def bin_file(cid):
    """Path of the case's block file (tab-separated shifts, one block row per line), written once."""
    def make():
        path = os.path.join(_TMP.name, "bin_%s.txt" % cid)
        with open(path, "w") as f:
            for row in bin_h(cid):
                f.write("\t".join(str(int(x)) for x in row) + "\n")
        return path
    return _memo(("bin_file", cid), make)


def bin_ref(cid):
    c = B_BY_ID[cid]
    return _memo(("bin_ref", cid), lambda: ref_gf2(bin_h(cid), c.J, c.L, c.Z))


# ---- GF(q) ---------------------------------------------------------------------------------------------------------------------------
def dense_hq(N, M, edges):
    """int64 [M, N]: entry (r, v) = XOR of the coefficients of the edges (r, v), as the decoders see H."""
    A = np.zeros((M, N), np.int64)
    for r, c, h in edges:
        A[r, c] ^= h
    return A


def ref_gfq(N, M, edges, q):
    """dict(K_info, rank, info_pos=int32 [K'], P=uint8 [rank, K']) in the layout of nbldpc.generator_host, by plain Gauss-Jordan
    over the tables of nb_shape_cases.gf_tables, pivot columns from the right, every pivot row normalised to 1."""
    mul, _, inv = S.gf_tables(q)
    A = dense_hq(N, M, edges)
    used = np.zeros(M, bool)
    row_of = np.full(N, -1)
    for c in range(N - 1, -1, -1):
        cand = np.flatnonzero((A[:, c] != 0) & ~used)
        if not cand.size:
            continue
        p = int(cand[0])
        used[p] = True
        row_of[c] = p
        A[p] = mul[inv[A[p, c]], A[p]]
        rows = np.flatnonzero(A[:, c])
        rows = rows[rows != p]
        A[rows] ^= mul[A[rows, c][:, None], A[p][None, :]]
    info = np.flatnonzero(row_of < 0).astype(np.int32)
    par = np.flatnonzero(row_of >= 0)
    P = A[row_of[par]][:, info].astype(np.uint8).reshape(len(par), len(info))
    return dict(K_info=len(info), rank=len(par), info_pos=info, P=P)


# the four larger codes: id: (q, N, dv, dc, drop, seed), and the (K', rank) the reference must give
NEW = {
    "q8_chunk4": (8, 390, 2, 6, 7, 31),    # K' = 260: a last LDS chunk of 4 symbols
    "q4_pad": (4, 777, 2, 7, 5, 32),       # K' = 555: Kp = 556, three chunks, rank mod 8 = 6
    "q128_rank1": (128, 301, 3, 7, 4, 33),  # rank 129: rank mod 8 = 1, 17 row groups, the last workgroup with one active wave
    "q32_half": (32, 268, 2, 4, 3, 34),    # K' = rank = 134
}
NEW_WANT = {"q8_chunk4": (260, 130), "q4_pad": (555, 222), "q128_rank1": (172, 129), "q32_half": (134, 134)}
TWIN = "_def"  # suffix of a rank-deficient twin
NB_IDS = S.IDS + [i + TWIN for i in S.IDS] + list(NEW)
NbCode = collections.namedtuple("NbCode", "q N M dv dc edges")


def twin_factor(q, seed):
    """The nonzero, non-unit multiple a twin's last row is of its row 0."""
    return 2 + seed % (q - 2)


def nb_code(cid):
    """NbCode of the case, made once: (q, N, M, dv, dc, edges in row-major slot order)."""
    def make():
        if cid in NEW:
            q, N, dv, dc, drop, seed = NEW[cid]
            M, edges = S.random_graph(N, dv, dc, drop, q, seed)
            return NbCode(q, N, M, dv, dc, tuple(edges))
        twin = cid.endswith(TWIN)
        case = S.BY_ID[cid[:-len(TWIN)] if twin else cid]
        M, edges = S.graph(case)
        dv = case.dv
        if twin:
            mul = S.gf_tables(case.q)[0]
            a = twin_factor(case.q, case.seed)
            edges = [e for e in edges if e[0] != M - 1] + [(M - 1, c, int(mul[a, h])) for r, c, h in edges if r == 0]
            dv = int(np.bincount([c for _, c, _ in edges], minlength=case.N).max())
        return NbCode(case.q, case.N, M, dv, case.dc, tuple(edges))
    return _memo(("nb_code", cid), make)


def nb_files(cid):
    """(matrix path, GF table path) of the case, written once; the codes of nb_shape_cases.py keep the files that module writes."""
    def make():
        if cid in S.BY_ID:
            return S.files(S.BY_ID[cid])
        c = nb_code(cid)
        mpath = os.path.join(_TMP.name, "nb_%s.txt" % cid)
        gpath = os.path.join(_TMP.name, "gf%d.txt" % c.q)
        S.write_matrix(mpath, c.N, c.M, c.q, c.dv, c.dc, list(c.edges))
        if not os.path.exists(gpath):
            S.write_gf(gpath, c.q)
        return mpath, gpath
    return _memo(("nb_files", cid), make)


def nb_ref(cid):
    c = nb_code(cid)
    return _memo(("nb_ref", cid), lambda: ref_gfq(c.N, c.M, list(c.edges), c.q))
