"""What test_fading_cpu.py and test_fading_gpu.py share: the shapes at which the fading kernels can still go wrong, and float32 numpy
restatements of the two demappers with receiver CSI (include/bldpc.h "block fading", include/nbldpc.h)."""
import numpy as np

from harq_qam_cases import CON_NAMES, IL_NONE, IL_ROWCOL, MODEM_SHAPES, RULES, bit_index, bits, constellation, n_sym, np_demap  # noqa: F401

# (S, Lc, F): fast fading; blocks that end inside a run of 32 uses; one block exactly; Lc above S; the smallest call; a codeword of
# J4_L24_Z96 over BPSK with more than one workgroup of runs and F no multiple of anything
GAIN_SHAPES = [(77, 1, 70), (77, 5, 70), (77, 77, 70), (77, 100, 70), (1, 1, 1), (2304, 16, 257)]
# (N, F): a run of 32 that ends inside a word; the shipped length; more than one block of 256 frames with a short last one
BPSK_SHAPES = [(77, 70), (2304, 64), (33, 257)]
# (Ns, q, F)
QAM_SHAPES = [(33, 64, 70), (1, 256, 1), (384, 64, 257), (329, 128, 65)]
# (N, m, F) of the demapper: the modem shapes (N % m != 0 among them, Ns = 1, 3, 1, 64, 329, 288: both sides of 32 and of 64) with
# F on both sides of the 64-frame tile, and the constellation sizes the shapes do not reach (m = 2, 4, 5) at a small ragged shape
DEMAP_SHAPES = [(1, 8, 1), (7, 3, 63), (5, 6, 65), (383, 6, 65), (2301, 7, 63), (2304, 8, 257), (383, 1, 65), (131, 2, 63), (131, 4, 65),
                (131, 5, 257)]
# (q, N, B) of the GF(q) demodulator
NB_SHAPES = [(4, 12, 1), (4, 96, 70), (64, 12, 70), (64, 96, 1), (64, 576, 70), (256, 12, 1), (256, 96, 70), (256, 576, 1)]
FADE_SEED = (4711, 4712, 4713)

_extra = {}


def con_of(C, m):
    """float32 [2^m, 2]: the table of harq_qam_cases where it has the size, else rand16 / rand32 made as test_modem_gpu makes them."""
    q = 1 << m
    if q in CON_NAMES:
        return constellation(C, q)
    if q not in _extra:
        from test_modem_gpu import constellation as named
        _extra[q] = np.ascontiguousarray(named(C, "rand%d" % q), np.float32)
    return _extra[q]


def np_demap_fading(rx, gain, con, scale, N, il):
    """bldpc_qam_demap_fading in np.float32, one rounding per operation: np_demap with the points a * c, each product rounded to float32
    before the subtraction.  rx [F, Ns, 2], gain [F, Ns] -> [N, F]."""
    q = con.shape[0]
    m = q.bit_length() - 1
    a = np.ascontiguousarray(gain, np.float32)[:, :, None]
    ax = a * con[None, None, :, 0]
    ay = a * con[None, None, :, 1]
    assert ax.dtype == np.float32
    dx = rx[:, :, None, 0] - ax
    dy = rx[:, :, None, 1] - ay
    d = dx * dx + dy * dy  # float32 [F, Ns, q]
    assert d.dtype == np.float32
    out = np.zeros((N, rx.shape[0]), np.float32)
    e = bit_index(N, m, il)
    p = np.arange(q)
    for b in range(m):
        one = (p >> b) & 1 == 1
        v = (d[:, :, one].min(2) - d[:, :, ~one].min(2)) * np.float32(scale)
        keep = e[:, b] < N
        out[e[keep, b]] = v.T[keep]
    return out


def np_nb_demod(rx, con, sigma, gain=None):
    """k_nb_demod_qam (gain None) and nbldpc_demodulate_qam_fading in np.float32: rx [B, N, 2], con [q, 2], gain [B, N] -> [B, N, q-1].
    The four products a*c0r, a*c0i, a*ckr, a*cki first, then the expression in its order."""
    rx = np.ascontiguousarray(rx, np.float32)
    con = np.ascontiguousarray(con, np.float32)
    two, s = np.float32(2), np.float32(sigma)
    yr, yi = rx[:, :, None, 0], rx[:, :, None, 1]
    c0r, c0i, ckr, cki = con[0, 0], con[0, 1], con[None, None, 1:, 0], con[None, None, 1:, 1]
    if gain is not None:
        a = np.ascontiguousarray(gain, np.float32)[:, :, None]
        c0r, c0i, ckr, cki = a * c0r, a * c0i, a * ckr, a * cki
    out = ((two * yr - c0r - ckr) * (ckr - c0r) + (two * yi - c0i - cki) * (cki - c0i)) / (two * s * s)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def demap_inputs(C, N, m, F, seed):
    """(rx [F, Ns, 2], gain [F, Ns], con) for the demapper tests: points of random symbols under gains of Lc = 5 from the host
    generator, a few of them 0.0 and 1.0, plus noise."""
    rng = np.random.default_rng(seed)
    con = con_of(C, m)
    Ns = n_sym(N, m)
    gain = C.Fading_Gains_host(np.array(FADE_SEED, np.int32), 5, Ns, F)
    flat = gain.reshape(-1)
    k = max(1, flat.size // 9)
    flat[rng.integers(0, flat.size, k)] = 0.0
    flat[rng.integers(0, flat.size, k)] = 1.0
    flat[0] = 0.0
    sym = rng.integers(0, 1 << m, (F, Ns))
    rx = (gain[:, :, None] * con[sym] + rng.normal(0.0, 0.2, (F, Ns, 2))).astype(np.float32)
    return rx, gain, con
