"""The case table of tests/test_nb_qspa_layered_cpu.py and tests/test_nb_qspa_layered_gpu.py: the shapes of tests/nb_qspa_cases.py plus
the graphs at which the level sweep of k_nb_qspa_layered can go wrong (a level wider than one pass of the workgroup, a level whose
row count is no multiple of the vectors per wave, single-row levels next to wide ones, a column of weight 1 beside one of weight dvmax,
a column of weight 0), their inputs, the results of the host statement nbldpc_qspa_layered_decode_host on them, and the fp32 numpy
restatement of the layered decoder written from the text of include/nbldpc.h ("FHT sum-product, layered schedule").

Inputs and host results are computed once per case and shared; nothing here is written to after it was made."""
import collections
import os

import numpy as np

import nb_qspa_cases as Q
from nb_shape_cases import random_graph, write_gf, write_matrix

MAX_ITER = Q.MAX_ITER
FRAMES_PER_SNR = Q.FRAMES_PER_SNR
f32 = np.float32
THREAD_SET = (256, 512, 1024)


# ---- graphs the flooding table does not have: -> (N, M, dv, dc, edges), edges (row, column, coefficient) in row-major slot order ----
def two_partitions(N, q, seed):
    """Two random partitions of the N columns into rows of 4: rows 0 ... N/4-1 are pairwise disjoint (level 0, N/4 rows wide), and so
    are rows N/4 ... N/2-1 (level 1).  A (2, 4)-regular code."""
    assert N % 4 == 0
    rng = np.random.default_rng(seed)
    rows = np.concatenate([rng.permutation(N).reshape(N // 4, 4), rng.permutation(N).reshape(N // 4, 4)])
    gf = rng.integers(1, q, size=rows.shape)
    return N, N // 2, 2, 4, [(r, int(rows[r, t]), int(gf[r, t])) for r in range(N // 2) for t in range(4)]


def random_plus_ladder(N0, steps, q, seed):
    """A random (2, 4) graph on columns 0 ... N0-1 and, after its rows, a ladder of `steps` rows of weight 2 on columns N0 ... N0+steps:
    ladder row k sits alone in level k once the random part's levels are used up."""
    M0, edges = random_graph(N0, 2, 4, 0, q, seed)
    rng = np.random.default_rng(seed + 100)
    gf = rng.integers(1, q, size=(steps, 2))
    edges = list(edges) + [(M0 + k, N0 + k + t, int(gf[k, t])) for k in range(steps) for t in range(2)]
    return N0 + steps + 1, M0 + steps, 2, 4, edges


def thinned_columns(N, q, seed):
    """A random (3, 6) graph with column 0 emptied (weight 0) and a later column c cut down to one edge whose row keeps a column of
    weight 3 = dvmax: weights 0, 1 and dvmax in one code, 1 and dvmax in one row."""
    M, edges = random_graph(N, 3, 6, 0, q, seed)
    rows0 = {r for r, c, _ in edges if c == 0}
    c1 = next(c for c in range(1, N) if not rows0 & {r for r, cc, _ in edges if cc == c})  # no row loses two edges
    keep = min(k for k, (r, c, _) in enumerate(edges) if c == c1)
    edges = [e for k, e in enumerate(edges) if e[1] != 0 and (e[1] != c1 or k == keep)]
    return N, M, 3, 6, edges


def _of_q(cid):
    c = Q.BY_ID[cid]
    M, edges = Q.graph(c)
    return c.N, M, c.dv, c.dc, edges


# snr: Eb/N0 of the noisy frames over BPSK, FRAMES_PER_SNR of each, chosen with the LAYERED host statement alone such that the frames of
# the case stop at three or more different iteration counts and one at least fails (test_nb_qspa_layered_cpu.py asserts it).
Case = collections.namedtuple("Case", "id q snr seed make")
_SNR = {"q8": (-1.0, 1.0, 3.0), "q32": (0.0, 2.0, 4.0)}  # where the flooding table's values leave the layered decoder no failing frame
CASES = [Case(c.id, c.q, _SNR.get(c.id, c.snr), c.seed, (lambda cid=c.id: _of_q(cid))) for c in Q.CASES] + [
    Case("wide_q64", 64, (1.0, 2.0, 3.0), 21, lambda: two_partitions(84, 64, 21)),     # 21 rows per level: two passes even at 1024 threads
    Case("wide_q16", 16, (1.0, 2.5, 4.0), 22, lambda: two_partitions(84, 16, 22)),     # 21 = 5 waves of 4 vectors + 1
    Case("mix_q16", 16, (2.0, 4.0, 6.0), 23, lambda: random_plus_ladder(24, 9, 16, 23)),  # single-row levels after wide ones
    Case("thin_q32", 32, (2.0, 4.0, 6.0), 24, lambda: thinned_columns(24, 32, 24)),    # column weights 0, 1 and 3
]
LDS_OVER = Case(Q.LDS_OVER.id, Q.LDS_OVER.q, (), Q.LDS_OVER.seed, lambda: _of_q(Q.LDS_OVER.id))
BY_ID = {c.id: c for c in CASES + [LDS_OVER]}
IDS = [c.id for c in CASES]
PINNED = "wide_q16"  # a code run under every workgroup size of THREAD_SET: 2 passes per level at 256 threads, 1 at 512 and 1024

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def graph(case):
    return _memo(("graph", case.id), case.make)


def files(case):
    """(matrix path, GF table path), written once."""
    def make():
        N, M, dv, dc, edges = graph(case)
        mpath = os.path.join(Q._TMP.name, "layered_" + case.id + ".txt")
        gpath = os.path.join(Q._TMP.name, "gf%d.txt" % case.q)
        write_matrix(mpath, N, M, case.q, dv, dc, edges)
        if not os.path.exists(gpath):
            write_gf(gpath, case.q)
        return mpath, gpath
    return _memo(("files", case.id), make)


def matrix(nb, case):
    def make():
        m = nb.NBMatrix(files(case)[0])
        m.TableMultiply = Q.mul_table(case.q)
        return m
    return _memo(("matrix", case.id), make)


def inputs(nb, case):
    """float32 [3 * FRAMES_PER_SNR, N, q-1], read-only."""
    def make():
        N, M, _, _, _ = graph(case)
        rng = np.random.default_rng(7000 + case.seed)
        rate = max((N - M) / N, 1.0 / N)
        L = np.ascontiguousarray(np.concatenate([Q.bpsk_llr(nb, N, case.q, s, rate, rng, FRAMES_PER_SNR) for s in case.snr]), np.float32)
        L.setflags(write=False)
        return L
    return _memo(("inputs", case.id), make)


def want(nb, case, maxIT=MAX_ITER):
    """The layered host statement on the case's inputs, with state."""
    return _memo(("want", case.id, maxIT),
                 lambda: nb.Decoding_QSPA_host(matrix(nb, case), inputs(nb, case), maxIT, want_state=True, layered=True))


# ---- the dependency levels and the workgroup-size rule, restated --------------------------------------------------------------------
def level_tables(M, edges):
    """-> (level of every row, row_order, level_begin): a row's level is 1 + the highest level among the EARLIER rows that share a
    variable with it; row_order lists the rows by level, ascending within one."""
    last, level = {}, []
    for r in range(M):
        cols = [c for rr, c, _ in edges if rr == r]
        lv = max(last.get(c, -1) for c in cols) + 1
        for c in cols:
            last[c] = lv
        level.append(lv)
    order = sorted(range(M), key=lambda r: (level[r], r))
    begin = [0] * (max(level) + 2)
    for lv in level:
        begin[lv + 1] += 1
    return level, order, np.cumsum(begin).tolist()


def level_widths(case):
    _, M, _, _, edges = graph(case)
    begin = level_tables(M, edges)[2]
    return np.diff(begin).tolist()


def threads_rule(q, widest):
    """include/nbldpc.h: 256 where its waves hold the widest level in one pass, else 512; 1024 only by the switch."""
    return 256 if 256 // 64 * max(64 // q, 1) >= widest else 512


# ---- the layered decoder restated in numpy float32, from the text of include/nbldpc.h -------------------------------------------------
def np_decode_layered(m, mul, L, maxIT, levels=None):
    """One frame: m an NBMatrix, L float32 [N, q-1] -> dict(out, it, ok, APP [N,q], c2v [M,dc,q]).  levels None: rows 0 ... M-1 in
    that order, each on the messages as they stand.  levels a list of row lists: one level at a time, every row of a level from the
    messages as they stood when the level began (what rows run side by side see), stored together when the level ends."""
    N, M, q, dc = m.N, m.M, m.q, m.dc
    mul = np.asarray(mul, np.int64)
    x = np.concatenate([np.zeros((N, 1), f32), np.asarray(L, f32)], axis=1)
    with np.errstate(over="ignore"):
        p = np.maximum(Q.np_exp(x - x.max(axis=1, keepdims=True)), Q.FLOOR)
    c2v = np.ones((M, dc, q), f32)
    slot = {}  # (variable, edge) -> (row, slot): first match
    for i in range(N):
        for d in range(m.vn_weight[i]):
            r = int(m.vn_linkCNs[i, d])
            slot[(i, d)] = (r, [int(v) for v in m.cn_linkVNs[r, :m.cn_weight[r]]].index(i))

    def row_messages(r, state):
        w, vs = m.cn_weight[r], []
        for t in range(w):
            i = int(m.cn_linkVNs[r, t])
            v = p[i]
            for d2 in range(m.vn_weight[i]):
                if slot[(i, d2)] != (r, t):
                    v = Q.np_norm(v * state[slot[(i, d2)]])
            vs.append(v)
        return Q.np_check_node(vs, [int(m.cn_linkVNs_GF[r, t]) for t in range(w)], mul)

    out, app = np.zeros(N, np.int32), np.zeros((N, q), f32)
    it, ok = 0, 0
    while it < maxIT:
        it += 1
        for i in range(N):
            a = p[i]
            for d in range(m.vn_weight[i]):
                a = Q.np_norm(a * c2v[slot[(i, d)]])
            app[i] = a
            out[i] = int(np.argmax(a))
        synd = [np.bitwise_xor.reduce([mul[out[m.cn_linkVNs[r, t]], m.cn_linkVNs_GF[r, t]] for t in range(m.cn_weight[r])]) for r in range(M)]
        if not any(synd):
            ok, it = 1, it - 1
            break
        for rows in ([[r] for r in range(M)] if levels is None else levels):
            res = [row_messages(r, c2v) for r in rows]
            for r, rr in zip(rows, res):
                for t in range(m.cn_weight[r]):
                    c2v[r, t] = rr[t]
    return dict(out=out, it=it, ok=ok, APP=app, c2v=c2v)
