"""What test_harq_qam_cpu.py and test_harq_qam_gpu.py share: the profiles of test_harq_gpu.py, the constellations of
test_modem_gpu.py, the small modem shapes, and numpy restatements of the index rules and of the modem (include/bldpc.h, "binary codes
over QAM")."""
import numpy as np

from test_harq_gpu import CASE_IDS, CASES, CH_PUNCT, CH_SHORT, DONES, N1, NCB, SHORT_LLR, make_done  # noqa: F401
from test_modem_gpu import constellation as _named

IL_NONE, IL_ROWCOL = 0, 1
RULES = [IL_NONE, IL_ROWCOL]
LAPS = [1, 1, 2, 3, 8]  # of CASES
# q -> the name test_modem_gpu.constellation knows it by: the shipped Gray files where they exist
CON_NAMES = {2: "bpsk", 4: "qpsk", 8: "rand8", 64: "gray64", 128: "rand128", 256: "gray256"}
# (N, m): one bit (one symbol with seven pads); pads in two symbols under ROWCOL; a short word with a pad; Ns = 64 with a pad, a
# multiple of both tiles; Ns = 329, a multiple of neither, with two pads; no pad at all
MODEM_SHAPES = [(1, 8), (7, 3), (5, 6), (383, 6), (2301, 7), (2304, 8)]
_cons = {}


def constellation(C, q):
    """float32 [q, 2], made once."""
    if q not in _cons:
        _cons[q] = np.ascontiguousarray(_named(C, CON_NAMES[q]), np.float32)
    return _cons[q]


def n_sym(N, m):
    return (N + m - 1) // m


def bit_index(N, m, il):
    """int [Ns, m]: the bit e behind bit b of symbol s; e >= N is a pad."""
    Ns = n_sym(N, m)
    s, b = np.meshgrid(np.arange(Ns), np.arange(m), indexing="ij")
    return b * Ns + s if il == IL_ROWCOL else s * m + b


def np_map(cw, N, m, il):
    """sym int32 [F, Ns] of cw int32 [N, F]: pad bits 0, only bit 0 of an entry is read."""
    e = bit_index(N, m, il)
    bits = np.where((e < N)[:, :, None], cw[np.minimum(e, N - 1)] & 1, 0)  # [Ns, m, F]
    return (bits << np.arange(m)[None, :, None]).sum(1).T.astype(np.int32)


def np_demap(rx, con, scale, N, il):
    """float32 [N, F] of rx float32 [F, Ns, 2]: every step of the header in np.float32, one rounding per operation."""
    q = con.shape[0]
    m = q.bit_length() - 1
    dx = rx[:, :, None, 0] - con[None, None, :, 0]
    dy = rx[:, :, None, 1] - con[None, None, :, 1]
    d = dx * dx + dy * dy  # float32 [F, Ns, q]: two products, each rounded, then their sum
    assert d.dtype == np.float32
    out = np.zeros((N, rx.shape[0]), np.float32)
    e = bit_index(N, m, il)
    p = np.arange(q)
    for b in range(m):
        one = (p >> b) & 1 == 1
        v = (d[:, :, one].min(2) - d[:, :, ~one].min(2)) * np.float32(scale)  # [F, Ns]
        keep = e[:, b] < N
        out[e[keep, b]] = v.T[keep]
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
