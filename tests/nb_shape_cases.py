"""The case table of tests/test_nb_shapes_cpu.py and tests/test_nb_shapes_gpu.py: random GF(q) codes at the shapes the shipped
matrices and the synthetic (2, 4) codes of test_nbldpc_gpu.py do not have -- column weights 3 and 4 on the fused kernels, more
than 96 columns (the tail loop of phase A), rows of weight 2, GF(128), idle groups and dv 3 on the wide kernel, GF(4) / GF(8)
and explicit-stack rows of weight 7 ... 12 on the workspace kernel, trellis rows of 7 and 8 edges and the 63 / 64 level boundary.

Every code is generated from the case's seed (numpy only), written in the reference's matrix and GF-table formats into a temporary
directory, and read from there by the oracle, the product and tests/cpp/nb_plan_host_test.hip alike.  The inputs and the oracle
results the tests compare with are computed once per case and shared; nothing here is written to after it was made."""
import collections
import os
import tempfile

import numpy as np

POLY = {4: 7, 8: 11, 16: 19, 32: 37, 64: 67, 128: 137, 256: 285}  # primitive polynomials, as tests/test_host_cpu.py
MAX_ITER = 8
SEED = (173, 173, 173)


def gf_tables(q):
    """(mul [q, q], add [q, q], inv [q]) of GF(q) = GF(2)[x] / POLY[q], int64."""
    poly, m = POLY[q], q.bit_length() - 1
    a = np.arange(q)[:, None] * np.ones((1, q), np.int64)
    b = np.arange(q)[None, :] * np.ones((q, 1), np.int64)
    r = np.zeros((q, q), np.int64)
    x = a.copy()
    for i in range(m):  # carry-less multiply, reduced on the fly
        r ^= np.where((b >> i) & 1, x, 0)
        x <<= 1
        x = np.where(x & q, x ^ poly, x)
    inv = np.zeros(q, np.int64)
    for e in range(1, q):
        inv[e] = int(np.flatnonzero(r[e] == 1)[0])
    return r, a ^ b, inv


def write_gf(path, q):
    mul, add, inv = gf_tables(q)
    with open(path, "w") as f:
        f.write("GF(%d) with Primitive Polynomial: %d.\nMultiply Table:\n" % (q, POLY[q]))
        for row in mul:
            f.write(" ".join(str(int(x)) for x in row) + "\n")
        f.write("Add Table:\n")
        for row in add:
            f.write(" ".join(str(int(x)) for x in row) + "\n")
        f.write("Inverse Table:\n" + " ".join(str(int(x)) for x in inv) + "\n")


def random_graph(N, dv, dc, drop, q, seed):
    """A (dv, dc)-regular bipartite graph of the configuration model with `drop` edges taken out: (M, edges), edges = list of
    (row, column, coefficient) in row-major slot order.  Parallel edges of the draw are repaired by swapping the second stub of a
    pair with a random stub of another row (accepted when neither row gets a pair from it), never by drawing again.  Every row and
    every column loses at most one edge, so no column is left empty (dv >= 2) and every row keeps dc - 1 >= 2."""
    assert (N * dv) % dc == 0 and dv >= 2 and dc >= 3 and dc <= N
    rng = np.random.default_rng(seed)
    M = N * dv // dc
    stubs = np.repeat(np.arange(N), dv)
    rng.shuffle(stubs)
    rows = stubs.reshape(M, dc)

    def first_pair():
        for r in range(M):
            seen = set()
            for t in range(dc):
                if int(rows[r, t]) in seen:
                    return r, t
                seen.add(int(rows[r, t]))
        return None
    while True:
        bad = first_pair()
        if bad is None:
            break
        r, t = bad
        while True:
            r2, t2 = int(rng.integers(M)), int(rng.integers(dc))
            a, b = int(rows[r, t]), int(rows[r2, t2])
            if r2 != r and a not in rows[r2] and b not in rows[r]:
                rows[r, t], rows[r2, t2] = b, a
                break
    gf = rng.integers(1, q, size=(M, dc))
    edges = [(r, int(rows[r, t]), int(gf[r, t])) for r in range(M) for t in range(dc)]
    colw, roww = np.full(N, dv), np.full(M, dc)
    for k in rng.permutation(len(edges)):
        if drop == 0:
            break
        r, c, _ = edges[k]
        if colw[c] == dv and roww[r] == dc:  # at most one edge out of any row or column
            colw[c] -= 1
            roww[r] -= 1
            edges[k] = None
            drop -= 1
    assert drop == 0, "the graph has no room for that many dropped edges"
    return M, [e for e in edges if e is not None]


def ladder_graph(M, q, seed):
    """Row r joins variables r and r + 1: M rows of weight 2, N = M + 1, end columns of weight 1.  Every row shares a variable with
    the row before it, so the layered schedule has exactly M levels."""
    rng = np.random.default_rng(seed)
    gf = rng.integers(1, q, size=(M, 2))
    return M, [(r, r + t, int(gf[r, t])) for r in range(M) for t in range(2)]


def write_matrix(path, N, M, q, dv, dc, edges):
    """The reference's matrix format (Get_H): header, column weights, row weights, the columns' (row, coefficient) lists with rows
    ascending, the rows' (column, coefficient) lists in slot order; indices from 1."""
    colw, roww = np.zeros(N, np.int64), np.zeros(M, np.int64)
    for r, c, _ in edges:
        colw[c] += 1
        roww[r] += 1
    with open(path, "w") as f:
        f.write("%d %d %d\n%d %d\n" % (N, M, q, dv, dc))
        f.write(" ".join(str(int(w)) for w in colw) + "\n" + " ".join(str(int(w)) for w in roww) + "\n")
        by_col = [[] for _ in range(N)]
        by_row = [[] for _ in range(M)]
        for r, c, h in edges:
            by_col[c].append((r, h))
            by_row[r].append((c, h))
        for c in range(N):
            f.write(" ".join("%d %d" % (r + 1, h) for r, h in by_col[c]) + "\n")
        for r in range(M):
            f.write(" ".join("%d %d" % (c + 1, h) for c, h in by_row[r]) + "\n")


def levels_of(M, edges):
    """The layered schedule's level count restated: level of a row = 1 + the highest level among the EARLIER rows that share a
    variable with it."""
    last, top = {}, 0
    for r in range(M):
        cols = [c for rr, c, _ in edges if rr == r]
        lv = max([last.get(c, -1) for c in cols]) + 1
        for c in cols:
            last[c] = lv
        top = max(top, lv + 1)
    return top


# ---- the case table --------------------------------------------------------------------------------------------------------------
# kernel: what Decoding_EMS must report in code.last_kernel; tmm: the trellis decoders are offered; snr: Eb/N0 of the noisy frames,
# FRAMES_PER_SNR of each, chosen with the oracle alone such that the frames stop at three or more different iterations, one at
# least decodes after >= 2 iterations and one never does (test_nb_shapes_cpu.py checks this, for every decoder the code offers).
# (The ladders are rate-1/N codes: their frames spread over the iterations at Eb/N0 of 10 ... 16 dB only.)
Case = collections.namedtuple("Case", "id q N dv dc drop kernel tmm snr seed")
FRAMES_PER_SNR = 4
CASES = [
    Case("dv3_q16", 16, 48, 3, 6, 5, "k_nb_ems", True, (2.0, 4.0, 6.0), 1),         # k_nb_ems<16, 8>: columns 2 / 3, rows 5 / 6
    Case("dv3_q64", 64, 24, 3, 6, 3, "k_nb_ems", True, (2.0, 4.0, 6.0), 2),         # k_nb_ems<64, 8>; no pipeline (dv > 2)
    Case("dv4_q32", 32, 30, 4, 6, 6, "k_nb_ems", True, (2.0, 4.0, 6.0), 3),         # k_nb_ems<32, 8>: columns 3 / 4
    Case("tail_q16", 16, 130, 2, 4, 9, "k_nb_ems", True, (2.0, 4.0, 6.0), 4),       # tail loop: columns 96 ... 129, waves 0-1 one trip more
    Case("tail_q32", 32, 130, 2, 4, 0, "k_nb_ems", True, (2.0, 4.0, 6.0), 5),
    Case("tail_q64", 64, 100, 2, 4, 7, "k_nb_ems", True, (2.0, 4.0, 6.0), 6),       # 163 016 B of LDS; tail in waves 0-3 only
    Case("wide128", 128, 26, 2, 4, 3, "k_nb_ems_wide", False, (2.0, 4.0, 6.0), 7),  # GW 2; idle groups in the last rounds
    Case("wide128_dv3", 128, 16, 3, 6, 2, "k_nb_ems_wide", False, (2.0, 4.0, 6.0), 8),
    Case("wide256_dv3", 256, 8, 3, 6, 0, "k_nb_ems_wide", False, (4.0, 5.0, 6.0), 9),
    Case("hbm_q4", 4, 24, 2, 4, 3, "k_nb_ems_hbm", False, (2.0, 4.0, 6.0), 10),     # q not fused: explicit stack
    Case("hbm_q8", 8, 24, 2, 4, 3, "k_nb_ems_hbm", False, (0.0, 2.0, 4.0), 11),
    Case("dc8_q16", 16, 48, 2, 8, 5, "k_nb_ems_hbm", True, (2.0, 4.0, 6.0), 12),    # EMS: explicit stack w 7 / 8; trellis rows of 7 / 8
    Case("dc8_q32_dv3", 32, 48, 3, 8, 6, "k_nb_ems_hbm", True, (2.0, 4.0, 6.0), 13),
    Case("dc12_q64", 64, 48, 2, 12, 4, "k_nb_ems_hbm", False, (2.0, 4.0, 6.0), 14),  # explicit stack w 11 / 12 at q = 64
    Case("hbm256_mixed", 256, 48, 2, 12, 3, "k_nb_ems_hbm", False, (4.5, 5.0, 5.5), 15),  # w 12 straight-line, w 11 explicit stack
    Case("big_q16", 16, 600, 2, 4, 20, "k_nb_ems_hbm", False, (2.0, 4.0, 6.0), 16),  # M dc = 1 200 > 1 024: three chunk passes
    Case("ladder63", 16, 64, 2, 2, None, "k_nb_ems", True, (10.0, 13.0, 16.0), 17),    # rows of weight 2; exactly 63 levels
    Case("ladder64", 16, 65, 2, 2, None, "k_nb_ems", False, (10.0, 13.0, 16.0), 18),   # 64 levels: trellis refused
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]

_TMP = tempfile.TemporaryDirectory(prefix="nb_shape_cases_")
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def graph(case):
    """(M, edges) of the case, made once."""
    def make():
        if case.drop is None:
            return ladder_graph(case.N - 1, case.q, case.seed)
        return random_graph(case.N, case.dv, case.dc, case.drop, case.q, case.seed)
    return _memo(("graph", case.id), make)


def files(case):
    """(matrix path, GF table path), written once."""
    def make():
        M, edges = graph(case)
        mpath = os.path.join(_TMP.name, case.id + ".txt")
        gpath = os.path.join(_TMP.name, "gf%d.txt" % case.q)
        write_matrix(mpath, case.N, M, case.q, case.dv, case.dc, edges)
        if not os.path.exists(gpath):
            write_gf(gpath, case.q)
        return mpath, gpath
    return _memo(("files", case.id), make)


def ocode(orc, case):
    return _memo(("ocode", case.id), lambda: orc.NBCode(*files(case)))


def n_noisy(case):
    return FRAMES_PER_SNR * len(case.snr)


def inputs(orc, case):
    """float32 [B, N, q - 1], B = 4 per Eb/N0 + 4 <= 16: the all-zero codeword through the oracle's channel (BPSK, one stream from
    the seed (173, 173, 173) across the Eb/N0 values), then the special frames of test_ties_zeros_and_extremes: integers in
    [-3, 3] (ties everywhere: first-maximum, first-minimum and stable-sort rules, within a wave and across the waves of a wide
    vector) -- one with -0.0 entries, one scaled by 1e30, one scaled by 1e-40 (denormals), one as it is."""
    def make():
        oc = ocode(orc, case)
        seed = np.array(SEED, np.int32)
        cw = np.zeros(case.N, np.int32)
        L = []
        for snr in case.snr:
            sigma = orc.nb_sigma(snr, oc.rate)
            L += [orc.nb_channel(oc, cw, seed, sigma)[1] for _ in range(FRAMES_PER_SNR)]
        sp = np.random.default_rng(1000 + case.seed).integers(-3, 4, size=(4, case.N, case.q - 1)).astype(np.float32)
        sp[0, :, ::5] = -0.0
        sp[1] *= np.float32(1e30)
        sp[2] *= np.float32(1e-40)
        sp = list(sp)
        Lch = np.ascontiguousarray(np.stack(L + sp), np.float32)
        Lch.setflags(write=False)
        return Lch
    return _memo(("inputs", case.id), make)


def want_ems(orc, case, Nm=2, Nc=2, dcmax_cfg=None):
    """The oracle's Decoding_EMS on every frame of the batch: list of dict(out, it, ok, LLR, c2v)."""
    Lch = inputs(orc, case)
    return _memo(("ems", case.id, Nm, Nc, dcmax_cfg),
                 lambda: [orc.nb_ems_decode(ocode(orc, case), Lch[b], Nm, Nc, MAX_ITER, dcmax_cfg=dcmax_cfg, want_state=True)
                          for b in range(Lch.shape[0])])


def want_tmm(orc, case, layered):
    Lch = inputs(orc, case)
    return _memo(("tmm", case.id, layered),
                 lambda: [orc.nb_tmm_decode(ocode(orc, case), Lch[b], MAX_ITER, layered=layered, want_state=True) for b in range(Lch.shape[0])])


def spread_ok(case, want):
    """The condition on the inputs that makes a comparison worth something, on the noisy frames: three or more different iteration
    counts, a frame that decodes after >= 2 iterations and a frame that never does.  -> (verdict, what was seen)."""
    w = want[:n_noisy(case)]
    its = sorted(set(r["it"] for r in w))
    late = any(r["ok"] == 1 and r["it"] >= 2 for r in w)
    never = any(r["ok"] == 0 for r in w)
    return len(its) >= 3 and late and never, "%s: iterations %s, ok %s" % (case.id, [r["it"] for r in w], [r["ok"] for r in w])
