"""The case table of tests/test_nb_qspa_cpu.py and tests/test_nb_qspa_gpu.py: random GF(q) codes at the smallest shapes at which each
mechanism of the FHT sum-product kernel can go wrong, their inputs, the results of the host statement on them, and the fp32 numpy
restatement of the decoder written from the text of include/nbldpc.h ("FHT sum-product").

Every code is generated from the case's seed with the generators of tests/nb_shape_cases.py and written in the reference's matrix
format into a temporary directory.  Inputs and host results are computed once per case and shared; nothing here is written to after it
was made."""
import collections
import os
import tempfile

import numpy as np

from nb_shape_cases import gf_tables, ladder_graph, random_graph, write_gf, write_matrix

MAX_ITER = 8
FRAMES_PER_SNR = 4
LDS_LIMIT = 159 * 1024
f32 = np.float32


def lds_bytes(N, M, q, dc):
    """The bound of include/nbldpc.h."""
    return 4 * (N * q + M * dc * q) + 4 * (N + 4) + q * q


# snr: Eb/N0 of the noisy frames over BPSK, FRAMES_PER_SNR of each, chosen with the host statement alone such that the frames of the
# case stop at three or more different iteration counts and one at least fails (test_nb_qspa_cpu.py asserts it).  drop None: a ladder.
Case = collections.namedtuple("Case", "id q N dv dc drop snr seed")
CASES = [
    Case("q4", 4, 24, 2, 4, 0, (1.0, 3.0, 5.0), 1),        # 16 vectors per wave
    Case("q8", 8, 16, 2, 4, 2, (1.0, 3.0, 5.0), 2),        # 8 per wave, rows of 3 and 4
    Case("q16_part", 16, 22, 2, 4, 0, (1.0, 3.0, 5.0), 3),  # 4 per wave; 22 variables and 11 rows: the last wave partly empty
    Case("q32", 32, 20, 2, 4, 3, (1.0, 3.0, 5.0), 4),      # 2 per wave, an odd number of rows in the last wave
    Case("q64", 64, 24, 2, 4, 0, (1.0, 3.0, 5.0), 5),
    Case("q64_tail", 64, 100, 2, 4, 7, (1.0, 2.0, 3.0), 6),  # past 96 columns: more than one trip of every vector loop
    Case("q64_dv3", 64, 24, 3, 6, 3, (2.0, 4.0, 6.0), 7),  # columns 2 / 3, rows 5 / 6
    Case("q64_dv4", 64, 24, 4, 6, 4, (2.0, 4.0, 6.0), 8),  # columns 3 / 4
    Case("q128", 128, 12, 2, 4, 0, (1.0, 3.0, 5.0), 9),    # two entries per lane
    Case("q256", 256, 12, 2, 4, 2, (1.0, 3.0, 5.0), 10),   # four entries per lane
    Case("ladder", 16, 16, 2, 2, None, (2.0, 5.0, 8.0), 11),  # rows of weight 2, end columns of weight 1
    Case("dc12_q8", 8, 48, 2, 12, 2, (2.0, 3.0, 4.0), 12),  # rows of 11 / 12: the longest forward / backward run
    Case("lds_under", 64, 204, 2, 4, 0, (1.0, 2.0, 3.0), 13),  # 161 600 bytes of the 162 816
]
LDS_OVER = Case("lds_over", 64, 206, 2, 4, 0, (), 14)       # 163 144 bytes: refused
BY_ID = {c.id: c for c in CASES + [LDS_OVER]}
IDS = [c.id for c in CASES]

_TMP = tempfile.TemporaryDirectory(prefix="nb_qspa_cases_")
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def graph(case):
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


def mul_table(q):
    return _memo(("mul", q), lambda: np.ascontiguousarray(gf_tables(q)[0], np.uint32))


def matrix(nb, case):
    """The host-side code (nb.NBMatrix with its TableMultiply): no device."""
    def make():
        m = nb.NBMatrix(files(case)[0])
        m.TableMultiply = mul_table(case.q)
        return m
    return _memo(("matrix", case.id), make)


def bpsk_llr(nb, N, q, snr_db, rate, rng, frames):
    """The all-zero codeword over BPSK at Eb/N0 = snr_db: float32 [frames, N, q-1] through the library's host demodulator."""
    sigma = float(np.sqrt(1.0 / (2.0 * rate * 10.0 ** (snr_db / 10.0))))
    m = q.bit_length() - 1
    rx = (1.0 + sigma * rng.standard_normal((frames, N * m))).astype(np.float32)
    return nb.Demodulate_NQ_host(N, q, rx, sigma)


def inputs(nb, case):
    """float32 [3 * FRAMES_PER_SNR, N, q-1], read-only."""
    def make():
        M, _ = graph(case)
        rng = np.random.default_rng(5000 + case.seed)
        rate = max((case.N - M) / case.N, 1.0 / case.N)
        L = np.concatenate([bpsk_llr(nb, case.N, case.q, s, rate, rng, FRAMES_PER_SNR) for s in case.snr])
        L = np.ascontiguousarray(L, np.float32)
        L.setflags(write=False)
        return L
    return _memo(("inputs", case.id), make)


def want(nb, case, maxIT=MAX_ITER):
    """The host statement on the case's inputs, with state."""
    return _memo(("want", case.id, maxIT), lambda: nb.Decoding_QSPA_host(matrix(nb, case), inputs(nb, case), maxIT, want_state=True))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the decoder restated in numpy float32, from the text of include/nbldpc.h ---------------------------------------------------------
FLOOR = f32(2.0 ** -40)


def np_exp(x):
    """qspa_exp: every step one float32 operation."""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        live = x >= f32(-87.0)
        xs = np.where(live, x, f32(0.0)).astype(f32)
        n = np.rint(xs * f32(float.fromhex("0x1.715476p+0")))
        r = (xs - n * f32(float.fromhex("0x1.62e4p-1"))) - n * f32(float.fromhex("0x1.7f7d1cp-20"))
        p = np.full_like(xs, f32(float.fromhex("0x1.6d4932p-10")))
        for c in ("0x1.12107cp-7", "0x1.5554e4p-5", "0x1.5554d8p-3", "0x1p-1", "0x1p+0", "0x1p+0"):
            p = p * r + f32(float.fromhex(c))
        y = p * np.ldexp(f32(1.0), n.astype(np.int32))
    assert y.dtype == f32
    return np.where(live, y, f32(0.0)).astype(f32)


def np_norm(v):
    return np.maximum(v / v.max(), FLOOR)


def np_fht(v):
    q = v.shape[0]
    s = 1
    while s < q:
        w = v.reshape(q // (2 * s), 2, s)
        lo, hi = w[:, 0, :], w[:, 1, :]
        v = np.stack([lo + hi, lo - hi], axis=1).reshape(q)
        s *= 2
    return v


def np_check_node(vs, hs, mul):
    """The check-node rule on one row: vs list of v2c float32 [q], hs the coefficients -> list of c2v."""
    w = len(vs)
    U = []
    for v, h in zip(vs, hs):
        u = np.empty_like(v)
        u[mul[h]] = v
        W = np_fht(u)
        U.append(W / W[0])
    F, B = [U[0]], [None] * w
    for t in range(1, w):
        F.append(F[t - 1] * U[t])
    B[w - 1] = U[w - 1]
    for t in range(w - 2, -1, -1):
        B[t] = U[t] * B[t + 1]
    res = []
    for t, h in enumerate(hs):
        o = B[1] if t == 0 else F[w - 2] if t == w - 1 else F[t - 1] * B[t + 1]
        wv = np.maximum(np_fht(o), f32(0.0))
        c = wv[mul[h]]
        res.append(np.ones_like(c) if c.max() == 0 else np_norm(c))
    return res


def np_decode(m, mul, L, maxIT):
    """One frame: m an NBMatrix, L float32 [N, q-1] -> dict(out, it, ok, APP [N,q], c2v [M,dc,q])."""
    N, M, q, dc = m.N, m.M, m.q, m.dc
    mul = np.asarray(mul, np.int64)
    x = np.concatenate([np.zeros((N, 1), f32), np.asarray(L, f32)], axis=1)
    with np.errstate(over="ignore"):
        p = np.maximum(np_exp(x - x.max(axis=1, keepdims=True)), FLOOR)
    c2v = np.ones((M, dc, q), f32)
    slot = {}  # (variable, edge) -> (row, slot): first match
    for i in range(N):
        for d in range(m.vn_weight[i]):
            r = int(m.vn_linkCNs[i, d])
            slot[(i, d)] = (r, [int(v) for v in m.cn_linkVNs[r, :m.cn_weight[r]]].index(i))
    out, app = np.zeros(N, np.int32), np.zeros((N, q), f32)
    it, ok = 0, 0
    while it < maxIT:
        it += 1
        for i in range(N):
            a = p[i]
            for d in range(m.vn_weight[i]):
                a = np_norm(a * c2v[slot[(i, d)]])
            app[i] = a
            out[i] = int(np.argmax(a))
        synd = [np.bitwise_xor.reduce([mul[out[m.cn_linkVNs[r, t]], m.cn_linkVNs_GF[r, t]] for t in range(m.cn_weight[r])]) for r in range(M)]
        if not any(synd):
            ok, it = 1, it - 1
            break
        v2c = np.ones((M, dc, q), f32)
        for i in range(N):
            w = m.vn_weight[i]
            for d in range(w):
                v = p[i]
                for d2 in range(w):
                    if d2 != d:
                        v = np_norm(v * c2v[slot[(i, d2)]])
                v2c[slot[(i, d)]] = v
        for r in range(M):
            w = m.cn_weight[r]
            res = np_check_node([v2c[r, t] for t in range(w)], [int(m.cn_linkVNs_GF[r, t]) for t in range(w)], mul)
            for t in range(w):
                c2v[r, t] = res[t]
    return dict(out=out, it=it, ok=ok, APP=app, c2v=c2v)
