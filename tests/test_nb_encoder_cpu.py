"""CPU tests of the GF(q) encoder's host half (nbldpc_generator_host) and of the random-message rule.

The generator is checked against numpy restatements built from the CN lists and the tables of GFInitial: H * c = 0 over GF(q) for
codewords encoded through P, the rank of H from an independent elimination (with the file's own inverse table), and the refusal of a
multiply table that is not a field.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import DATA, ROOT

NB = os.path.join(DATA, "nb")
FILES = ["BDS.576.288.GF.64.txt", "LDPC_N576_K288_GF64_d1_exp.txt", "LDPC_N96_K48_GF256_d1_exp.txt", "LDPC_N576_K480_GF256_exp.txt",
         "Tanner_74_9_Z128_GF16.txt"]


@pytest.fixture(scope="module")
def nb():
    from cuda_ldpc_amd import nbldpc
    return nbldpc


_cache = {}


def load(nb, name):
    """(host matrix, TableMultiply, TableInverse) of a shipped NB matrix."""
    if name not in _cache:
        H = nb.NBMatrix(os.path.join(NB, name))
        mul, _, inv = nb.GFInitial(H.q, os.path.join(NB, "GF", "Arith.Table.GF.%d.txt" % H.q))
        _cache[name] = (H, mul.astype(np.int64), inv.astype(np.int64))
    return _cache[name]


def dense_h(H):
    """M x N symbol matrix as the decoders see it: entry (r, v) = XOR of the coefficients of all edges (r, v)."""
    A = np.zeros((H.M, H.N), np.int64)
    for r in range(H.M):
        for t in range(H.cn_weight[r]):
            A[r, H.cn_linkVNs[r, t]] ^= H.cn_linkVNs_GF[r, t]
    return A


def syndrome_np(H, mul, words):
    """Per-check sums over GF(q) of words [B, N] (low log2 q bits): [B, M], the decoders' check restated."""
    w = np.asarray(words, np.int64) & (H.q - 1)
    s = np.zeros((w.shape[0], H.M), np.int64)
    for t in range(H.dc):
        live = t < H.cn_weight
        v = np.where(live, H.cn_linkVNs[:, t], 0)
        h = np.where(live, H.cn_linkVNs_GF[:, t], 0)  # coefficient 0 adds nothing
        s ^= mul[w[:, v], h[None, :]]
    return s


def encode_np(gen, N, mul, msg):
    """Codewords [B, N] of messages [B, K'] through the host generator: systematic on info_pos, parity r = XOR_j mul[msg_j][P[r, j]]."""
    q = mul.shape[0]
    msg = np.asarray(msg, np.int64) & (q - 1)
    B, K = msg.shape
    P = gen["P"].astype(np.int64)
    cw = np.zeros((B, N), np.int64)
    cw[:, gen["info_pos"]] = msg
    par = np.zeros((B, gen["rank"]), np.int64)
    for j0 in range(0, K, 64):
        prod = mul[msg[:, None, j0:j0 + 64], P[None, :, j0:j0 + 64]]  # [B, rank, 64]
        par ^= np.bitwise_xor.reduce(prod, axis=2)
    cw[:, np.setdiff1d(np.arange(N), gen["info_pos"])] = par
    return cw


def rank_np(A, mul, inv):
    """Rank over GF(q) by plain Gaussian elimination (left to right, the file's inverse table)."""
    A = A.copy()
    M, N = A.shape
    r = 0
    for c in range(N):
        rows = np.nonzero(A[r:, c])[0]
        if not len(rows):
            continue
        p = r + rows[0]
        A[[r, p]] = A[[p, r]]
        A[r] = mul[inv[A[r, c]], A[r]]
        for i in np.nonzero(A[:, c])[0]:
            if i != r:
                A[i] ^= mul[A[i, c], A[r]]
        r += 1
        if r == M:
            break
    return r


@pytest.mark.parametrize("name", FILES)
def test_generator_rank_information_set_and_codewords(nb, name):
    H, mul, inv = load(nb, name)
    t = time.time()
    gen = nb.generator_host(H, mul)
    dt = time.time() - t
    K, rank, pos, P = gen["K_info"], gen["rank"], gen["info_pos"], gen["P"]
    assert K + rank == H.N and P.shape == (rank, K) and P.max(initial=0) < H.q
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < H.N
    if H.N <= 96:
        assert rank == rank_np(dense_h(H), mul, inv), "rank differs from an independent elimination"
    assert dt < 120, "generator of %s took %.1f s" % (name, dt)
    rng = np.random.default_rng(len(name))
    B = 6
    msg = rng.integers(0, 1 << 20, (B, K))
    msg[0] = rng.integers(1, H.q, K)  # every information symbol nonzero
    cw = encode_np(gen, H.N, mul, msg)
    assert np.array_equal(cw[:, pos], msg & (H.q - 1)), "not systematic on info_pos"
    assert not syndrome_np(H, mul, cw).any(), "H * c != 0 over GF(%d)" % H.q
    assert cw[:, np.setdiff1d(np.arange(H.N), pos)].any(), "parity symbols all zero"
    # the numpy check itself sees a corrupted word
    bad = cw.copy()
    bad[:, pos[0]] ^= 1
    assert syndrome_np(H, mul, bad).any(axis=1).all()


def test_generator_refuses_a_table_that_is_not_a_field(nb):
    from cuda_ldpc_amd._lib import LdpcError
    H, mul, _ = load(nb, "BDS.576.288.GF.64.txt")
    bad = mul.copy()
    bad[5, 9] ^= 1  # still symmetric: distributivity breaks
    bad[9, 5] ^= 1
    with pytest.raises(LdpcError, match=r"\(-5\).*TableMultiply does not distribute"):
        nb.generator_host(H, bad)
    bad = mul.copy()
    bad[2, 3], bad[2, 4] = mul[2, 4], mul[2, 3]
    with pytest.raises(LdpcError, match=r"\(-5\).*TableMultiply"):
        nb.generator_host(H, bad)
    bad = mul.copy()
    bad[7, 7] = 0  # a zero divisor: still symmetric, no longer a field
    with pytest.raises(LdpcError, match=r"\(-5\).*TableMultiply"):
        nb.generator_host(H, bad)


def test_pn_messages_rule(nb):
    from cuda_ldpc_amd.bldpc import splitmix64
    assert int(splitmix64(0)) == 0xE220A8397B1DCDAF  # SplitMix64 seeded with 0: its well-known first output
    seed, K, B, first = 0xDEADBEEF, 25, 5, 7
    for q, m in ((16, 4), (64, 6), (256, 8)):
        s = 64 // m
        W = -(-K // s)
        got = nb.pn_messages(seed, K, q, B, first_frame=first)
        assert got.shape == (B, K) and got.dtype == np.int32 and got.max() < q
        for b in range(B):
            for k in (0, s - 1, s, K - 1):
                w = int(splitmix64((seed + (first + b) * W + k // s) % (1 << 64)))
                assert got[b, k] == (w >> (m * (k % s))) & (q - 1)
        assert np.array_equal(nb.pn_messages(seed, K, q, 3, first_frame=first + 2), got[2:])
        assert not np.array_equal(nb.pn_messages(seed + 1, K, q, B, first_frame=first), got)


def test_sweep_nb_refuses_a_constellation_of_another_field():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sweep.py"), "nb", "--nb-matrix", "Tanner_74_9_Z128_GF16.txt", "--qam", "64"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "GF(16)" in r.stderr
