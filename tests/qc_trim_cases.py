"""Inputs shared by test_qc2_valu_trim_gpu.py and test_select_network_cpu.py: exact channel values and the frame that makes a
variable-node sum of -0.0f only (see test_qc2_valu_trim_gpu.py)."""
import os

import numpy as np

from conftest import DATA

BL = os.path.join(DATA, "bldpc")
MATRIX_SHAPES = [(4, 24, 96), (8, 24, 96), (6, 24, 96), (12, 24, 96), (32, 64, 64)]


def path(J, L, Z):
    return os.path.join(BL, "J%d_L%d_Z%d_BlockH.txt" % (J, L, Z))


def _odd_cover(B):
    """Block columns with an odd number of their blocks in every block row: a full-weight column if there is one, else a solution
    of B x = 1 over GF(2) (Gauss-Jordan, free variables 0)."""
    J, L = B.shape
    if B.all(0).any():
        return [int(np.argmax(B.all(0)))]
    A = np.concatenate([B.astype(np.uint8), np.ones((J, 1), np.uint8)], axis=1)
    piv, r = [], 0
    for c in range(L):
        rows = [i for i in range(r, J) if A[i, c]]
        if not rows:
            continue
        A[[r, rows[0]]] = A[[rows[0], r]]
        for i in range(J):
            if i != r and A[i, c]:
                A[i] ^= A[r]
        piv.append(c)
        r += 1
        if r == J:
            break
    assert not A[r:, L].any(), "no column set with an odd count in every block row"
    return [c for i, c in enumerate(piv) if A[i, L]]


def corner_frame(J, L, Z):
    """(y of input (b), the block columns whose variables sum -0.0f only from iteration 2 on)."""
    B = np.loadtxt(path(J, L, Z), dtype=np.int64).reshape(J, L) >= 0
    cols = _odd_cover(B)
    inside = B[:, cols].sum(1)
    assert (inside % 2 == 1).all() and (B.sum(1) - inside >= 2).all()
    corner = [l for l in range(L) if l not in cols and B[:, l].sum() == B.sum(0).max()]
    assert corner
    y = np.full((L, Z), -0.0, np.float32)
    y[cols] = -1.0
    return y.reshape(-1), corner


def _random_frames(J, L, Z, n):
    vals = np.array([-0.0, 0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0], np.float32)
    rng = np.random.default_rng(9000 + J)
    return vals[rng.integers(0, len(vals), size=(n, L * Z))]


def batches(J, L, Z):
    """name -> (y as [N][F], index of the corner frame or None)"""
    a = _random_frames(J, L, Z, 2)
    b, _ = corner_frame(J, L, Z)
    return {"F1-random": (a[0][:, None], None), "F1-corner": (b[:, None], 0), "F3": (np.stack([a[0], b, a[1]], axis=1), 1)}
