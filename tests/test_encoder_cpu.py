"""CPU tests of the systematic encoder's host half (bldpc_generator_host) and of the PN_Message plumbing.

The generator is checked against a numpy restatement of H built from the block shifts (column c of a block with shift s
meets row (c - s) mod Z): rank, K' and the information set of every shipped matrix, H * c = 0 for random messages.
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import DATA, ROOT

BL = os.path.join(DATA, "bldpc")


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def _dims(name):
    if name == "PON_LDPC.txt":
        return 12, 69, 256
    return tuple(int(x) for x in re.match(r"J(\d+)_L(\d+)_Z(\d+)_BlockH\.txt$", name).groups())


FILES = sorted(f for f in os.listdir(BL) if f.endswith("_BlockH.txt")) + ["PON_LDPC.txt"]

# matrices whose last M columns are singular: pivots found among the last M columns (of M)
SINGULAR_TAIL = {"J12_L60_Z160": 1919, "J15_L60_Z160": 2396, "J20_L60_Z160": 2879, "J24_L60_Z160": 3520, "J30_L60_Z160": 4640}
RANK_DEFICIENT = {"J40_L60_Z160": 6399, "J48_L60_Z160": 7679}


def syndrome_np(H, J, L, Z, cw):
    """H * cw over GF(2) from the shifts: cw uint8 [N, F] -> [M, F]."""
    s = np.zeros((J * Z, cw.shape[1]), np.uint8)
    for j in range(J):
        for l in range(L):
            sh = int(H[j * L + l])
            if sh != -1:
                s[j * Z + (np.arange(Z) - sh) % Z] ^= cw[l * Z:(l + 1) * Z]
    return s


def encode_np(gen, N, msg):
    """Codewords [N, F] uint8 of messages [K', F] from the host generator: systematic on info_pos, parity = P * msg."""
    K, P = gen["K_info"], gen["P"]
    msg = (np.asarray(msg) & 1).astype(np.uint8)
    par = np.setdiff1d(np.arange(N), gen["info_pos"])
    cw = np.zeros((N, msg.shape[1]), np.uint8)
    cw[gen["info_pos"]] = msg
    mf = msg.astype(np.float32)
    for r0 in range(0, gen["rank"], 1024):  # counts stay below 2^24: exact in float32
        bits = np.unpackbits(P[r0:r0 + 1024].view(np.uint8), axis=1, bitorder="little")[:, :K].astype(np.float32)
        cw[par[r0:r0 + 1024]] = (bits @ mf).astype(np.int64) & 1
    return cw


@pytest.mark.parametrize("name", FILES)
def test_generator_rank_information_set_and_codewords(C, name):
    J, L, Z = _dims(name)
    N, M = L * Z, J * Z
    H, _, _ = C.Get_H(os.path.join(BL, name), J, L)
    t = time.time()
    gen = C.generator_host(H, J, L, Z)
    dt = time.time() - t
    tag = name.split("_BlockH")[0]
    rank, K, pos = gen["rank"], gen["K_info"], gen["info_pos"]
    assert rank + K == N and gen["P"].shape == (rank, (K + 63) // 64)
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < N
    assert rank == RANK_DEFICIENT.get(tag, M)
    tail_pivots = M - int(np.sum(pos >= N - M))
    if tag in SINGULAR_TAIL:
        assert tail_pivots == SINGULAR_TAIL[tag]
    elif tag in RANK_DEFICIENT:
        assert K == N - M + 1
    else:  # full rank, invertible parity part: the information set is exactly 0 .. K-1
        assert np.array_equal(pos, np.arange(N - M))
    if tag == "J15_L30_Z1280":
        assert dt < 30, "generator of J15_L30_Z1280 took %.1f s" % dt
    rng = np.random.default_rng(7)
    msg = rng.integers(0, 2, (K, 64), dtype=np.int32)
    cw = encode_np(gen, N, msg)
    assert np.array_equal(cw[pos], msg), "not systematic on info_pos"
    assert not syndrome_np(H, J, L, Z, cw).any(), "H * c != 0"
    assert cw[np.setdiff1d(np.arange(N), pos)].any(), "parity bits all zero"


def test_generator_refuses_bad_shifts(C):
    from cuda_ldpc_amd._lib import LdpcError
    with pytest.raises(LdpcError):
        C.generator_host(np.array([0, 5, -1, 1], np.int32), 2, 2, 4)  # J >= L and a shift past Z


def test_splitmix64_and_message_rule(C):
    from cuda_ldpc_amd.bldpc import pn_messages, splitmix64
    assert int(splitmix64(0)) == 0xE220A8397B1DCDAF  # SplitMix64 seeded with 0: its well-known first output
    K, F = 130, 5  # three words per frame
    m = pn_messages(12345, K, F, first_frame=7)
    assert m.shape == (K, F) and set(np.unique(m)) <= {0, 1}
    for f in range(F):
        for k in (0, 63, 64, 129):
            w = int(splitmix64((12345 + (7 + f) * 3 + k // 64) % (1 << 64)))
            assert m[k, f] == (w >> (k % 64)) & 1
    assert np.array_equal(pn_messages(12345, K, 3, first_frame=9), m[:, 2:])


def test_pn_message_needs_fixed_exit(C):
    from cuda_ldpc_amd.simulation import Simulation_GPU
    with pytest.raises(ValueError, match="EXIT_FIXED"):
        Simulation_GPU(None, np.array([173] * 3, np.int32), 1.0, C.SimCounters(), exit_mode=C.EXIT_BATCH_GLOBAL, PN_Message=1)
    with pytest.raises(ValueError):
        Simulation_GPU(None, np.array([173] * 3, np.int32), 1.0, C.SimCounters(), exit_mode=C.EXIT_FIXED, PN_Message=2)


def test_sweep_pn_message_requires_fixed():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sweep.py"), "binary", "--pn-message"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--fixed" in r.stderr
