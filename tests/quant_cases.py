"""What tests/test_quant_cpu.py and tests/test_quant_gpu.py share: the parameter sets, the inputs, the expected kernel tier of every
shape, and a numpy restatement of the quantised layered min-sum decoder's specification (include/bldpc.h) in int64 that also counts
how often each clamp acts.  Nothing here touches a device."""
import numpy as np

from test_layered_shapes_cpu import SHAPES, matrix_of, ramp_input

f32 = np.float32

# (bits_ch, bits_app, bits_msg, norm8, offset, llr_scale)
P0 = (6, 8, 6, 8, 0, 8.0)     # plain
P1 = (6, 8, 6, 6, 0, 16.0)    # normalised
P2 = (5, 7, 5, 8, 1, 8.0)     # offset
P3 = (4, 6, 4, 7, 1, 4.0)     # narrow: every clamp fires
P4 = (8, 15, 8, 5, 0, 32.0)   # widest words: m * norm8 and Q + R' are largest
PARAMS = {"P0": P0, "P1": P1, "P2": P2, "P3": P3, "P4": P4}

FIXED_ITER, MAX_ITER = 5, 10
F_PAIR = 37

ACCEPTED = [s for s in SHAPES if s[5] is not None]  # all but the weight-27 matrix, of which no code object is made
BY_DIMS = {s[:3]: s for s in SHAPES}
LDS_BYTES = 160 * 1024 - 1024  # what a workgroup may ask for


def tier_by_rule(J, L, Z):
    """The documented rule (include/bldpc.h): on-chip when Z <= 1024 and one frame pair's 4 N + 16 J Z + 16 bytes fit."""
    return "k_lq" if Z <= 1024 and 4 * L * Z + 16 * J * Z + 16 <= LDS_BYTES else "k_lq_ws"


# The tier bldpc_decode_layered_quant must pick, written out (test_quant_cpu.py holds the table to tier_by_rule).
TIER = {
    (3, 5, 13): "k_lq",         # N = 65: one bit in the last word, 4 pairs in a wave with idle lanes
    (4, 10, 7): "k_lq",         # N = 70, odd Z: 9 pairs in a wave
    (3, 7, 33): "k_lq",         # odd Z just above 32: pairs straddle the wave boundaries
    (3, 9, 50): "k_lq",
    (3, 9, 96): "k_lq",
    (6, 12, 500): "k_lq",       # 72 000 bytes a pair: two pairs of 500 rows in one workgroup
    (3, 8, 1056): "k_lq_ws",    # Z above 1024
    (4, 24, 8): "k_lq",         # 8 pairs in one wave; weights 2 and 23
    (32, 36, 16): "k_lq",       # 4 pairs in one wave, 32 layers
    (4, 10, 640): "k_lq",       # 640-thread workgroups
    (4, 12, 1024): "k_lq",      # 1024-thread workgroups, 114 688 bytes
    (8, 16, 1000): "k_lq_ws",   # 64 000 + 128 000 bytes; Z no multiple of 256: uneven t loop
    (3, 16, 4): "k_lq",         # 16 pairs in one wave
    (5, 8, 24): "k_lq",         # pairs straddle the wave boundaries
    (5, 12, 32): "k_lq",        # two pairs in one wave
    (5, 12, 96): "k_lq",
    (3, 8, 1024): "k_lq",       # 1024 threads
    (32, 34, 288): "k_lq_ws",   # 39 168 + 147 456 bytes
    (2, 27, 64): "k_lq",        # weights 26 and 25
    (4, 27, 64): "k_lq",        # weights 26, 2, 3, 25
}


def limits(P):
    return (1 << (P[0] - 1)) - 1, (1 << (P[1] - 1)) - 1, (1 << (P[2] - 1)) - 1  # C, A, Mx


def pair_input(N, F, seed=0, sigma=None, gain=1.0):
    """ramp_input with its columns permuted by a seeded permutation: the two frames of a pair have unrelated noise levels.
    sigma=(lo, hi) and gain: the same noise, y[:, f] = gain * (1 + sigma_f * g) with sigma_f from lo to hi instead of 0 to 1.3, for the
    shapes on which ramp_input's frames either stop at once or never (INPUT below)."""
    if sigma is None and gain == 1.0:
        y = ramp_input(N, F)
    else:
        g = np.random.default_rng(5).standard_normal((N, F))  # ramp_input's noise
        y = np.ascontiguousarray((gain * (1.0 + np.linspace(sigma[0], sigma[1], F)[None, :] * g)).astype(np.float32))
    return np.ascontiguousarray(y[:, np.random.default_rng(1000 + seed).permutation(F)])


# Shapes whose pair_input differs from the default, found by trying sigma ranges 0.3 wide from 0 up and gains 2 and 1 until the
# restatement says that the conditions of test_quant_cpu.test_gpu_inputs_meet_their_conditions hold under P0 and P3 alike.  With the
# default these matrices (high rate, or 64 variables) leave only frames that stop after one iteration and frames that never stop.
INPUT = {
    (4, 24, 8): dict(gain=2.0, sigma=(0.3, 0.6)),
    (4, 12, 1024): dict(gain=2.0, sigma=(0.3, 0.6)),
    (3, 16, 4): dict(gain=2.0, sigma=(0.4, 0.7)),
    (2, 27, 64): dict(gain=2.0, sigma=(0.2, 0.5)),
    (4, 27, 64): dict(gain=2.0, sigma=(0.2, 0.5)),
}
_in = {}


def input_for(s):
    """The shape's pair input, float32 [N, F_PAIR]: made once, shared by both test files, never written to."""
    if s[:3] not in _in:
        y = pair_input(s[1] * s[2], F_PAIR, **INPUT.get(s[:3], {}))
        y.setflags(write=False)
        _in[s[:3]] = y
    return _in[s[:3]]


def corrected_max(P):
    """g(Mx): the largest magnitude a check message can have."""
    _, _, Mx = limits(P)
    return max(0, ((Mx * P[3] + 4) >> 3) - P[4])


def app_clamp_possible(H, P):
    """Whether min(A, max(-A, .)) can act at all: |S| <= C + (column weight) * g(Mx), so it cannot where that stays within A.  Under P0
    (31 + 31 wc against 127) it takes a column of weight 4, under P3 (7 + 5 wc against 31) one of weight 5."""
    C, A, _ = limits(P)
    return C + int((np.asarray(H) != -1).sum(0).max()) * corrected_max(P) > A


def special_input(N, F, P, seed=7):
    """float32 [N, F], F >= 8, for the parameter set P (its llr_scale is a power of two, so the products below are exact): products
    that land exactly on k + 0.5 for even and odd k of both signs, zeros of both signs, denormals, values at and one ulp beyond
    +-C / llr_scale, 2^100, ordinary values; frame 0 has every magnitude tied, frame 1 holds only zeros of both signs, frame 2 only
    half-way products."""
    assert F >= 8
    C, _, _ = limits(P)
    sc = f32(P[5])
    rng = np.random.default_rng(seed)
    halves = np.array([k + 0.5 for k in (0, 1, 2, 3, 4, 5, -1, -2, -3, -4, -5, -6)], np.float32) / sc
    edge = f32(C) / sc
    edges = np.array([edge, np.nextafter(edge, f32(np.inf)), np.nextafter(edge, f32(0)), -edge, np.nextafter(-edge, f32(-np.inf)),
                      np.nextafter(-edge, f32(0))], np.float32)
    other = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.1754944e-38, -1.1754944e-38, 2.0 ** 100, -2.0 ** 100, 1.0, -1.0, 0.5, -0.25,
                      0.3, -0.7, 1.9, 2.6], np.float32)
    pool = np.concatenate([halves, edges, other])
    y = pool[rng.integers(0, pool.size, (N, F))]
    y[:, 0] = 1.0
    y[:, 1] = np.where(rng.random(N) < 0.5, f32(0.0), f32(-0.0))
    y[:, 2] = halves[rng.integers(0, halves.size, N)]
    assert np.array_equal((sc * halves) * 2 % 2, np.ones(halves.size)), "the products must land on k + 0.5 exactly"
    return np.ascontiguousarray(y.astype(np.float32))


# ---- the numpy restatement of the specification -------------------------------------------------------------------------------------------
CLAMPS = ("channel", "message", "app", "offset")


def np_quantise(y, P, counts=None):
    """int64 of the shape of y; one float32 product, np.rint (ties to even), saturation at +-C."""
    C, _, _ = limits(P)
    with np.errstate(all="ignore"):
        x = (f32(P[5]) * y.astype(np.float32)).astype(np.float32)
    sat = np.clip(np.rint(np.clip(x, -f32(C) - 1, f32(C) + 1)), -C - 1, C + 1).astype(np.int64)  # the clip keeps 2^100 castable
    q = np.where(x >= f32(C), C, np.where(x <= -f32(C), -C, sat)).astype(np.int64)
    if counts is not None:
        counts["channel"] += int((np.abs(sat) > C).sum())
    return q


def np_corrected(m, P):
    return ((m * P[3] + 4) >> 3) - P[4]  # before the max(0, .)


def np_quant_pass(H, Z, S, R, P, counts):
    """One iteration over S int64 [N, F] and R {(j, l): int64 [Z, F]} in place."""
    _, A, Mx = limits(P)
    J, L = H.shape
    t = np.arange(Z)
    for j in range(J):
        cols = [l for l in range(L) if H[j, l] != -1]
        v = [l * Z + (t + H[j, l]) % Z for l in cols]
        Q = np.stack([S[v[i]] - R[(j, cols[i])] for i in range(len(cols))])  # [w, Z, F]
        sg = Q < 0
        Par = np.logical_xor.reduce(sg, axis=0)
        a = np.minimum(np.abs(Q), Mx)
        counts["message"] += int((np.abs(Q) > Mx).sum())
        srt = np.sort(a, axis=0)
        m1, m2 = srt[0], srt[1]
        first = np.argmax(a == m1[None], axis=0)
        r1, r2 = np_corrected(m1, P), np_corrected(m2, P)
        counts["offset"] += int((r1 < 0).sum() + (r2 < 0).sum())
        g1, g2 = np.maximum(r1, 0), np.maximum(r2, 0)
        for i in range(len(cols)):
            mag = np.where(first == i, g2, g1)
            r = np.where(Par ^ sg[i], -mag, mag)
            new = Q[i] + r
            counts["app"] += int((np.abs(new) > A).sum())
            S[v[i]] = np.clip(new, -A, A)
            R[(j, cols[i])] = r


def np_quant_history(H, Z, y, iters, P):
    """S after every iteration, int64 [iters, N, F], and how often each clamp acted.  The layer passes do not depend on the stop rule,
    so one run serves every rule, every `length` and both exit modes (np_outputs of test_layered_shapes_cpu.py turns it into what
    each call must return)."""
    H = np.asarray(H).reshape(-1, y.shape[0] // Z)
    J, L = H.shape
    counts = dict.fromkeys(CLAMPS, 0)
    S = np_quantise(y, P, counts)
    R = {(j, l): np.zeros((Z, y.shape[1]), np.int64) for j in range(J) for l in range(L) if H[j, l] != -1}
    hist = np.empty((iters,) + y.shape, np.int64)
    for it in range(iters):
        np_quant_pass(H, Z, S, R, P, counts)
        hist[it] = S
    hist.setflags(write=False)
    return hist, counts


_hist = {}


def pair_history(s, name):
    """(history, clamp counts) of the shape's input_for under PARAMS[name], 10 iterations: computed once, never written to."""
    key = (s[:3], name)
    if key not in _hist:
        _hist[key] = np_quant_history(matrix_of(s), s[2], input_for(s), MAX_ITER, PARAMS[name])
    return _hist[key]
