"""The case table of tests/test_nb_qspa_ws_cpu.py and tests/test_nb_qspa_ws_gpu.py, the workspace tier of the FHT sum-product
decoders: the flooding cases of tests/nb_qspa_cases.py and the layered ones of tests/nb_qspa_layered_cases.py as they are, and what
the tier adds -- the code just over the LDS bound with inputs of its own, a GF(256) code with rows of 12 (two row passes under the
plan's 256 threads), the two shipped matrices the LDS tier refuses, and the plan restated from the text of include/nbldpc.h.

Inputs and host results are computed once and shared; nothing here is written to after it was made."""
import collections
import os

import numpy as np

import nb_qspa_cases as Q
import nb_qspa_layered_cases as LQ
from conftest import DATA

NB = os.path.join(DATA, "nb")
MAX_ITER = Q.MAX_ITER
LDS_LIMIT = Q.LDS_LIMIT
SIZES = (1024, 512, 256, 128, 64)

# ---- cases of the two tables' kind: (flooding case, layered case) under one id -------------------------------------------------------
# lds_over: the graph of Q.LDS_OVER (163 144 bytes of frame state: refused by the LDS tier), with the inputs that table has no use for.
LDS_OVER = Q.LDS_OVER._replace(snr=(1.0, 2.0, 3.0))
LDS_OVER_L = LQ.LDS_OVER._replace(snr=(1.0, 2.0, 3.0))
# q256_dc12: N 48, (2, 12)-regular, M = 8: fixed LDS 65 744 + 12 288 per wave -> 256 threads = 4 row slabs for 8 rows, two passes
Q256_DC12 = Q.Case("q256_dc12", 256, 48, 2, 12, 0, (3.0, 5.0, 7.0), 31)
Q256_DC12_L = LQ.Case("q256_dc12", 256, (3.0, 5.0, 7.0), 31,
                      lambda: (Q256_DC12.N,) + (Q.graph(Q256_DC12)[0], Q256_DC12.dv, Q256_DC12.dc, Q.graph(Q256_DC12)[1]))
EXTRA = {"lds_over": (LDS_OVER, LDS_OVER_L), "q256_dc12": (Q256_DC12, Q256_DC12_L)}


def flooding_case(cid):
    return EXTRA[cid][0] if cid in EXTRA else Q.BY_ID[cid]


def layered_case(cid):
    return EXTRA[cid][1] if cid in EXTRA else LQ.BY_ID[cid]


def case_of(cid, layered):
    return layered_case(cid) if layered else flooding_case(cid)


def mod_of(layered):
    """The module whose files / matrix / inputs / want serve the schedule."""
    return LQ if layered else Q


def dims(cid, layered):
    """(N, M, q, dv, dc) of a case."""
    if layered:
        c = layered_case(cid)
        N, M, dv, dc, _ = LQ.graph(c)
        return N, M, c.q, dv, dc
    c = flooding_case(cid)
    return c.N, Q.graph(c)[0], c.q, c.dv, c.dc


def widest_level(cid):
    return max(LQ.level_widths(layered_case(cid)))


# ---- the shipped matrices the LDS tier refuses ------------------------------------------------------------------------------------------
# Eb/N0 over BPSK chosen with the host statements alone (test_nb_qspa_ws_cpu.py asserts what they are chosen for).
Shipped = collections.namedtuple("Shipped", "id file q snr frames_per_snr maxIT seed")
N576 = Shipped("n576_k480_gf256", "LDPC_N576_K480_GF256_exp.txt", 256, (3.0, 4.0), 4, 8, 41)
TANNER = Shipped("tanner_gf16", "Tanner_74_9_Z128_GF16.txt", 16, (3.0,), 2, 3, 42)
SHIPPED = {s.id: s for s in (N576, TANNER)}

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def shipped_path(s):
    return os.path.join(NB, s.file)


def shipped_mul(nb, s):
    return _memo(("mul", s.q), lambda: nb.GFInitial(s.q, os.path.join(NB, "GF", "Arith.Table.GF.%d.txt" % s.q))[0])


def shipped_matrix(nb, s):
    def make():
        m = nb.NBMatrix(shipped_path(s))
        m.TableMultiply = shipped_mul(nb, s)
        return m
    return _memo(("matrix", s.id), make)


def shipped_inputs(nb, s):
    def make():
        m = shipped_matrix(nb, s)
        rng = np.random.default_rng(9000 + s.seed)
        L = np.ascontiguousarray(np.concatenate([Q.bpsk_llr(nb, m.N, s.q, x, float(m.rate), rng, s.frames_per_snr) for x in s.snr]), np.float32)
        L.setflags(write=False)
        return L
    return _memo(("inputs", s.id), make)


def shipped_want(nb, s, layered):
    return _memo(("want", s.id, layered),
                 lambda: nb.Decoding_QSPA_host(shipped_matrix(nb, s), shipped_inputs(nb, s), s.maxIT, want_state=True, layered=layered))


def matrix_levels(m):
    """Widths of the dependency levels of an NBMatrix (a row's level is 1 + the highest level among the earlier rows that share a
    variable with it)."""
    last, widths = {}, {}
    for r in range(m.M):
        cols = [int(c) for c in m.cn_linkVNs[r, :m.cn_weight[r]]]
        lv = max(last.get(c, -1) for c in cols) + 1
        for c in cols:
            last[c] = lv
        widths[lv] = widths.get(lv, 0) + 1
    return [widths[k] for k in sorted(widths)]


# ---- the plan, restated from include/nbldpc.h ("FHT sum-product, workspace tier") ------------------------------------------------------
def vectors(threads, q):
    return threads // 64 * max(64 // q, 1)


def ws_lds_bytes(N, q, dc, threads):
    return 4 * (N + 4) + q * q + 4 * vectors(threads, q) * dc * q


def slot_bytes(N, M, q, dc):
    return 4 * (N * q + M * dc * q)


def plan(N, M, q, dc, widest=0, layered=False):
    """dict(threads, lds_bytes, slot_bytes, vectors), or None where even 64 threads miss the bound."""
    fit = [t for t in SIZES if ws_lds_bytes(N, q, dc, t) <= LDS_LIMIT]
    if not fit:
        return None
    t = fit[0]
    if layered:
        hold = [x for x in fit if vectors(x, q) >= widest]
        if hold:
            t = min(hold)
    return dict(threads=t, lds_bytes=ws_lds_bytes(N, q, dc, t), slot_bytes=slot_bytes(N, M, q, dc), vectors=vectors(t, q))
