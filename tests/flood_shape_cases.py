"""The shape table of tests/test_flood_shapes_cpu.py and tests/test_flood_shapes_gpu.py: seeded generated codes at the edges of the
flooding decoders (bldpc_decode, bldpc_decode_per_frame, bldpc_decode_normalised, bldpc_decode_statistic, bldpc_statistic) that
neither the shipped matrices nor qc_variant_cases.random_block_matrix reach.

Table kernels: Z = 1, Z below 32, Z no multiple of 32, N no multiple of 4, a lifting size without an entry of the variant table, a
block column of weight 16, 1 and 0, a block row of weight 26 and 2, M and N above the grid cap of 65 535, an as-written table
with colliding slots.  Generic compressed-state tier: both sides of L = CPT * G, of J = 62, of the row weight WCS = 24 and of the
LDS bound, a partly filled last group, the Z = 96 entry at its full width, an empty block column, two blocks of one row with the same shift.

Matrices come from random_blockh of test_layered_shapes_cpu.py (seed J + L + Z) and are edited afterwards where the table says
so; they are written into a temporary directory for the oracle, never committed.  `landing` is where KERNEL_AUTO must send the
code: the tag of a variant-table entry, or None for the table kernels.  `gb` holds, for the batches of 5 and of 8 frames, the width
W of the ramp whose leading columns ramp_input(N, W)[:, :F] the batch-global rule stops strictly between iteration 1 and MAXIT
(the smallest such W, found with the oracle alone; test_flood_shapes_cpu.py checks it).  None: no width does (Z = 1 with 8 frames;
the mode then runs on ramp_input(N, F), which never stops), or the shape does not run that mode (the large one)."""
import collections
import os
import tempfile

import numpy as np

from qc_variant_cases import write_blockh
from test_layered_shapes_cpu import ramp_input, random_blockh

MAXIT = 20          # the early-exit modes
FIXED_ITS = (1, 2, 7)
BATCHES = (5, 8)    # VEC 1 and VEC 4 of the table kernels
GRID_CAP = 65535

Shape = collections.namedtuple("Shape", "J L Z weights edit landing gb")

W6 = (24, 24, 22, 22, 21, 21)  # six rows of at most WCS = 24 blocks that cover up to 134 columns
W17 = (26, 14, 9, 20, 5, 17, 11, 23, 8, 13, 19, 6, 25, 10, 16, 12, 2)  # J = 17: weights 26 and 2 (row 16 is the one that loses column 3)

SHAPES = [
    # ---- the table kernels alone ---------------------------------------------------------------------------------------------
    Shape(2, 4, 1, None, None, None, (7, None)),           # Z = 1: N = 4
    Shape(4, 10, 7, None, None, None, (8, 11)),            # Z below 32, N = 70: N % 4 = 2
    Shape(3, 5, 13, None, None, None, (6, 12)),            # N = 65, odd
    Shape(3, 7, 33, None, None, None, (8, 14)),            # Z just above 32, odd
    Shape(3, 9, 50, None, None, None, (11, 17)),           # N = 450
    Shape(6, 12, 500, None, None, None, (8, 13)),          # N = 6000
    Shape(4, 12, 32, None, None, None, (10, 17)),          # Z a multiple of 32 without an entry
    Shape(3, 8, 2048, None, None, None, (15, 25)),         # the same above every entry
    Shape(17, 40, 33, W17, "wv16", None, (10, 15)),        # column 3 of weight 16 (kMaxWv), column 7 of weight 1, rows of weight 26 (kMaxWc) and 2
    Shape(4, 10, 50, None, "empty", None, (15, 21)),       # a block column of weight 0
    Shape(32, 33, 2053, None, None, None, None),           # M = 65 696, N = 67 749: both stride loops take a second trip
    Shape(3, 9, 50, None, "literal", None, (13, 23)),      # the as-written table: colliding slots, levels > 1
    # ---- the generic compressed-state tier: Z = 64 entry (G 16, CPT 8, WCS 24) ------------------------------------------------
    Shape(6, 128, 64, W6, None, "compressed", (18, 29)),   # L = CPT * G
    Shape(6, 129, 64, W6, None, None, (18, 29)),           # one more
    Shape(6, 121, 64, W6, "twin", "compressed", (17, 29)),  # L % G = 9: a partly filled last group; two blocks of one row share a shift
    Shape(62, 64, 64, None, None, "compressed", (8, 13)),  # the last J
    Shape(63, 64, 64, None, None, None, (7, 12)),          # one more
    Shape(3, 26, 64, (24, 24, 3), None, "compressed", (13, 21)),  # WCS
    Shape(3, 26, 64, (24, 25, 3), None, None, (13, 21)),   # one more
    # an empty block column: only the register-state builder refuses one (qc_tables_regstate); qc_tables_compressed takes it, the
    # column's sum is then the channel value alone
    Shape(5, 12, 64, None, "empty", "compressed", (15, 21)),
    # ---- Z = 96 entry (U 128: 32 idle lanes per group, G 8, CPT 12) -----------------------------------------------------------
    Shape(4, 96, 96, (24,) * 4, None, "compressed", (16, 29)),  # L = CPT * G at full width; 4 rows of WCS blocks: every column has weight 1
    Shape(8, 96, 96, (24,) * 8, None, "compressed", (15, 26)),   # the same width with columns of more than one block
    Shape(4, 97, 96, (24,) * 4, "wide", None, (18, 29)),   # one more: the same rows over 96 columns and an empty 97th, so that L alone decides
    # ---- Z = 1024 entry: 12 (J + 1) Z + 4 (L + 1) Z + 16 <= 160 KiB ---------------------------------------------------------------
    Shape(3, 26, 1024, (24, 12, 7), None, "compressed", (17, 27)),  # 159 760 bytes
    Shape(3, 27, 1024, (24, 12, 7), None, None, (17, 29)),          # 163 856 bytes, 16 over
]
LARGE = (32, 33, 2053)  # at most 8 frames, 7 fixed iterations and one per-frame call
F_RAMP = 37             # the ramp on which the conditions of the per-frame exit hold on every shape (the CPU test checks them)
# (4, 10, 7) alone: one, two (261: of VEC 1 and of k_flags; 1028: of VEC 4, the second nearly empty) workgroups in x, and the
# ramp width of the batch-global rule as in `gb` (a batch of one frame is the noiseless frame 0: it stops at iteration 1)
BATCH_SIZES = {1: None, 4: 6, 37: 81, 260: 571, 261: 573, 1028: 2936, 1030: 2936}
STAT_BATCHES = (1028, 1030)  # the statistics kernels: F above 1024, a multiple of 4 and not
WV16_COL, WV1_COL = 3, 7  # of the "wv16" edit


def shape_id(s):
    return "J%d_L%d_Z%d" % s[:3] + ("_wc%d" % max(s.weights) if s.weights else "") + ("_" + s.edit if s.edit else "")


def by_id(ident):
    hits = [s for s in SHAPES if shape_id(s) == ident]
    assert len(hits) == 1, ident
    return hits[0]


def _move(H, j, src, banned):
    """Moves block (j, src) to the lightest column that row j does not meet (the leftmost of them; none of `banned`, none of
    weight 16): the row weights stay."""
    wv = (H != -1).sum(0)
    free = [c for c in range(H.shape[1]) if H[j, c] == -1 and c not in banned and c != src and wv[c] < 16]
    dst = min(free, key=lambda c: (wv[c], c))
    H[j, dst], H[j, src] = H[j, src], -1


def edited(s, H):
    """The post-edit of the table.  Row weights are kept ("wv16": blocks are moved, not added) or fall by at most one ("empty").
    wv16   column 3 meets block rows 0 .. J-2 and not the last one (weight 16 for J = 17): a row that lacks it moves the block of its
           heaviest other column there; column 7 keeps its topmost block only.
    empty  the leftmost block column whose removal leaves every block row at least two blocks is cleared.
    wide   an empty block column is appended.
    twin   the second block of block row 1 takes the shift of its first.
    Shifts 0 and Z - 1 are put back on the first and the last block."""
    H = H.copy()
    J, L = H.shape
    if s.edit == "wv16":
        c3, c1 = WV16_COL, WV1_COL
        for j in range(J - 1):
            if H[j, c3] == -1:
                wv = (H != -1).sum(0)
                src = max((c for c in range(L) if H[j, c] != -1 and c != c1), key=lambda c: (wv[c], -c))
                H[j, c3], H[j, src] = H[j, src], -1
        if H[J - 1, c3] != -1:
            _move(H, J - 1, c3, (c3, c1))
        rows = np.flatnonzero(H[:, c1] != -1)
        if len(rows) == 0:
            _move(H, 1, int(np.flatnonzero(H[1] != -1)[-1]), ())  # (not met by the seeds of the table)
        for j in rows[1:]:
            _move(H, int(j), c1, (c3, c1))
    elif s.edit == "empty":
        c = min(c for c in range(L) if ((H != -1).sum(1) - (H[:, c] != -1)).min() >= 2)
        H[:, c] = -1
    elif s.edit == "wide":
        H = np.concatenate([H, np.full((J, 1), -1, np.int32)], 1)
    elif s.edit == "twin":
        a, b = np.flatnonzero(H[1] != -1)[:2]
        H[1, b] = H[1, a]
    nz = np.flatnonzero(H.reshape(-1) != -1)
    H.reshape(-1)[nz[0]] = 0
    H.reshape(-1)[nz[-1]] = s.Z - 1
    return H


def generate(s):
    """The shape's block matrix, int32 [J, L]: deterministic in the table."""
    Lg = s.L - 1 if s.edit == "wide" else s.L
    return edited(s, random_blockh(s.J, Lg, s.Z, s.J + s.L + s.Z, s.weights))


_TMP = tempfile.TemporaryDirectory(prefix="flood_shape_cases_")
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def matrix_of(s):
    """The shape's matrix: made once, shared by both test files, never written to."""
    def make():
        H = generate(s)
        H.setflags(write=False)
        return H
    return _memo(("H", s), make)


def path_of(s):
    """The matrix as a BlockH file in a temporary directory, for the oracle."""
    def make():
        path = os.path.join(_TMP.name, shape_id(s) + ".txt")
        write_blockh(path, matrix_of(s))
        return path
    return _memo(("path", s), make)


def ocode(orc, s):
    """The oracle's code object; the "literal" shape with the reference's Transform_H as written."""
    return _memo(("ocode", s), lambda: orc.BinaryCode(path_of(s), s.J, s.L, s.Z, literal=s.edit == "literal"))


def make_code(C, s):
    """A fresh device code object: from the block shifts, the "literal" shape from its as-written address table."""
    H = matrix_of(s)
    if s.edit != "literal":
        return C.BinaryCode.from_shifts(H, s.J, s.L, s.Z)
    wc, wv = row_col_weights(H)
    return C.BinaryCode.from_table(s.J, s.L, s.Z, wc, wv, C.Transform_H(H, s.J, s.L, s.Z, wc, wv, as_written=True))


def row_col_weights(H):
    """Weight_Checknode [J+1] and Weight_Variablenode [L+1] as Get_H makes them: the maximum in the last place."""
    wc, wv = (H != -1).sum(1), (H != -1).sum(0)
    return np.append(wc, wc.max()).astype(np.int32), np.append(wv, wv.max()).astype(np.int32)


def lengths_of(s):
    N, K = s.L * s.Z, (s.L - s.J) * s.Z
    return tuple(dict.fromkeys((0, 1, K - 1, N)))  # Z = 1: K - 1 = 1


# ---- inputs: float32 [N, F] host arrays, made once, never written to ------------------------------------------------------------
def ramp(s, F, width=None):
    """The leading F columns of ramp_input(N, width or F)."""
    def make():
        y = np.ascontiguousarray(ramp_input(s.L * s.Z, width or F)[:, :F])
        y.setflags(write=False)
        return y
    return _memo(("ramp", s[:3], F, width or F), make)


def global_width(s, F):
    """The recorded ramp width of the batch-global rule for this shape and batch, or None."""
    if s.gb is not None and F in BATCHES:
        return s.gb[BATCHES.index(F)]
    return BATCH_SIZES.get(F) if s[:3] == (4, 10, 7) else None


def global_ramp(s, F):
    """(key, input) of the batch-global mode: the leading F columns of the ramp of the recorded width, or of ramp_input(N, F)."""
    W = global_width(s, F) or F
    return ("ramp", W), ramp(s, F, W)


# The special-values input holds +-3e38.  A block row of weight 2 hands one neighbour's value to the other unchanged, so two of them
# that meet through such a row add up to inf, and inf - inf = NaN one iteration later.  The kernels are defined for sums that stay
# finite (bldpc_math.hpp: "q is never -0.0f or NaN here"): what the reference's comparisons make of a NaN is no property of min-sum,
# and bldpc_decode_normalised_host departs from the oracle there as the kernels do.  On (3, 8, 2048) the draw for 5 frames has such a
# pair (positions 2744 and 14469 of frame 4, block row 2); the odd batch there has 9 frames.  The CPU test holds every batch used to
# finite sums by the oracle alone, and the overflow of the batch left out.
SPECIAL_BATCHES = {(3, 8, 2048): (9, 8)}


def special_batches(s):
    return SPECIAL_BATCHES.get(s[:3], BATCHES)


def special(s, F):
    def make():
        from qc_variant_cases import special_values
        y = special_values(s.L * s.Z, F).reshape(s.L * s.Z, F)
        y.setflags(write=False)
        return y
    return _memo(("special", s[:3], F), make)


def slow_batch(s, F):
    """Noise the decoder does not get through: the batch-global rule runs past 64 iterations (the CPU test checks that it does)."""
    def make():
        y = (1.0 + 1.5 * np.random.default_rng(9).standard_normal((s.L * s.Z, F))).astype(np.float32)
        y.setflags(write=False)
        return y
    return _memo(("slow", s[:3], F), make)


# ---- oracle results, once per (shape, input, mode): dict(D int32 [N+1, F], app float32 [N, F], it or iters, flag_hist) ----------
def _olen(length):
    return None if length == 0 else length  # the product's 0 is "K"; the oracle takes the number


def want_fixed(orc, s, key, y, its, length=0):
    def run():
        N, F = y.shape
        w = orc.bldpc_decode(ocode(orc, s), y, F, its, early_exit=0, length=_olen(length), want_app=True)
        return dict(D=w["D"].reshape(N + 1, F), app=w["app"].reshape(N, F), it=w["it"], flag_hist=w["flag_hist"])
    return _memo(("fixed", s, key, y.shape[1], its, length), run)


def want_global(orc, s, key, y, max_iter=MAXIT, length=0):
    def run():
        N, F = y.shape
        w = orc.bldpc_decode(ocode(orc, s), y, F, max_iter, early_exit=1, length=_olen(length), want_app=True)
        return dict(D=w["D"].reshape(N + 1, F), app=w["app"].reshape(N, F), it=w["it"], flag_hist=w["flag_hist"])
    return _memo(("global", s, key, y.shape[1], max_iter, length), run)


def want_per_frame(orc, s, key, y, max_iter=MAXIT, length=0):
    def run():
        from qc_variant_cases import oracle_per_frame
        D, app, iters = oracle_per_frame(orc, ocode(orc, s), y, y.shape[1], max_iter, _olen(length))
        return dict(D=D, app=app, iters=iters)
    return _memo(("pf", s, key, y.shape[1], max_iter, length), run)
