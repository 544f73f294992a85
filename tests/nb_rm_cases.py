"""The shared table of the GF(q) rate-matching tests (tests/test_nb_rm_cpu.py, tests/test_nb_rm_gpu.py) and the numpy restatement of
include/nbldpc.h, "rate matching", written from its words: profiles over N code symbols, frame-outer arrays, V = q - 1."""
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBD = os.path.join(ROOT, "data", "nb")

NS = (7, 96)
QS = (2, 4, 16, 64, 256)
BS = (1, 3, 257)
SIGMA = 0.7
SHORT_LLR = 1.0e4
PUNCT, SHORT = -1, -2

# the two lists of the profiles that shorten and puncture, per N: position 0 and position N - 1 are among them
LISTS = {7: ((0, 2), (6,)), 96: ((0, 5, 17), (95, 40, 41, 60))}


def profiles(N):
    """name -> dict(shorten, puncture, k0, E); E None: a linear profile (bldpc_rm_create)."""
    sh, pu = LISTS[N]
    ncb = N - len(sh) - len(pu)
    return {
        "identity": dict(shorten=(), puncture=(), k0=0, E=None),
        "linear": dict(shorten=sh, puncture=pu, k0=0, E=None),
        "circ_wrap": dict(shorten=sh, puncture=pu, k0=ncb - 2, E=ncb),        # k0 > 0, wraps, every position once
        "circ_short": dict(shorten=sh, puncture=pu, k0=1, E=ncb - 2),         # E < Ncb: some positions are not reached
        "circ_one": dict(shorten=sh, puncture=pu, k0=ncb - 1, E=1),           # E = 1
        "circ_twice": dict(shorten=sh, puncture=pu, k0=2, E=ncb + 1),         # one position is sent twice
        "circ_8laps": dict(shorten=(), puncture=pu, k0=3, E=8 * (N - len(pu))),  # 8 laps
        "circ_3laps_part": dict(shorten=sh, puncture=(), k0=1, E=2 * (N - len(sh)) + 3),  # some positions 3 times, the rest twice
    }


def make_rm(RateMatch, N, spec):
    if spec["E"] is None:
        return RateMatch(N, spec["shorten"], spec["puncture"])
    return RateMatch.circular(N, spec["shorten"], spec["puncture"], spec["k0"], spec["E"])


class Tables:
    """The profile as the words of include/bldpc.h put it: map[n], the buffer, tx_pos[e], and every position's contributions."""

    def __init__(self, N, spec):
        sh, pu = set(spec["shorten"]), set(spec["puncture"])
        self.N = N
        self.buffer = [n for n in range(N) if n not in sh and n not in pu]
        self.Ncb = len(self.buffer)
        self.k0 = spec["k0"]
        self.E = self.Ncb if spec["E"] is None else spec["E"]
        self.tx_pos = np.array([self.buffer[(self.k0 + e) % self.Ncb] for e in range(self.E)], np.int32)
        self.map = np.full(N, PUNCT, np.int32)
        self.map[sorted(sh)] = SHORT
        self.map[self.buffer] = np.arange(self.Ncb)
        self.contrib = [[] for _ in range(N)]
        for e, n in enumerate(self.tx_pos):
            self.contrib[n].append(e)  # ascending e


def np_select(t, cw):
    return np.ascontiguousarray(cw[:, t.tx_pos])


def np_receive(t, V, Lrx, short_llr=SHORT_LLR, acc=None, done=None):
    """recover (acc None) or combine: fp32 additions in ascending e, one contribution a copy of the 32 bits."""
    B = Lrx.shape[0]
    combine = acc is not None
    out = acc.copy() if combine else np.empty((B, t.N, V), np.float32)
    live = np.ones(B, bool) if (done is None or not combine) else (np.asarray(done) == 0)
    for n in range(t.N):
        es = t.contrib[n]
        if t.map[n] == SHORT:
            out[live, n, :] = -np.float32(short_llr)
        elif not es:
            if not combine:
                out.view(np.uint32)[:, n, :] = 0
        else:
            with np.errstate(all="ignore"):
                v = (out[live, n, :] + Lrx[live, es[0], :]) if combine else Lrx[live, es[0], :]
                for e in es[1:]:
                    v = v + Lrx[live, e, :]
            out.view(np.uint32)[live, n, :] = v.view(np.uint32)
    return out


def np_demod_qam(rx, con, sigma):
    """nbldpc_demodulate_qam's expression, operand for operand in fp32: rx [B, N, 2], con [q, 2] -> [B, N, q-1]."""
    f = np.float32
    yr, yi = rx[:, :, 0:1], rx[:, :, 1:2]
    c0r, c0i, ckr, cki = con[0, 0], con[0, 1], con[None, None, 1:, 0], con[None, None, 1:, 1]
    pr = (f(2) * yr - c0r - ckr) * (ckr - c0r)
    pi = (f(2) * yi - c0i - cki) * (cki - c0i)
    return ((pr + pi) / (f(2) * f(sigma) * f(sigma))).astype(np.float32)


def np_demod_bpsk(rx, q, sigma):
    """nbldpc_demodulate_bpsk's expression: rx [B, N*m] -> [B, N, q-1]; acc += (-2 * r[b]) / s2 over the set bits b of k, ascending."""
    f = np.float32
    m = q.bit_length() - 1
    B = rx.shape[0]
    r = rx.reshape(B, -1, m)
    s2 = f(sigma) * f(sigma)
    out = np.zeros((B, r.shape[1], q - 1), np.float32)
    for k in range(1, q):
        for b in range(m):
            if k >> b & 1:
                out[:, :, k - 1] = out[:, :, k - 1] + (f(-2) * r[:, :, b]) / s2
    return out


def np_force(t, info_pos, msg):
    out = msg.copy()
    out[:, t.map[info_pos] == SHORT] = 0
    return out


_CON = {}


def constellation(q):
    """GRAY_64QAM / GRAY_256QAM from data/ for q = 64, 256; a seeded random [q, 2] table for q = 2, 4, 16 (the calls take any table)."""
    if q not in _CON:
        if q in (64, 256):
            from cuda_ldpc_amd import nbldpc as nb
            _CON[q] = nb.Get_CONSTELLATION(os.path.join(NBD, "Constellation", "GRAY_%dQAM.txt" % q), q)
        else:
            _CON[q] = np.random.default_rng(1000 + q).normal(size=(q, 2)).astype(np.float32)
    return _CON[q]


def done_masks(B):
    """name -> int32 [B] or None"""
    alt = (np.arange(B) % 2).astype(np.int32)
    last = np.ones(B, np.int32)
    last[-1] = 0
    return {"null": None, "zero": np.zeros(B, np.int32), "one": np.ones(B, np.int32), "alternating": alt, "last_live": last}


def normal(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


SPECIALS = np.array([0x80000000, 0x7F61B1E6, 0xFF61B1E6, 0x000002CA, 0x80000001, 0x00000001], np.uint32)  # -0.0, +-3e38, denormals
NAN_PAYLOAD = np.uint32(0x7FC0BEEF)


def special_lrx(t, V, B, seed):
    """Seeded normal Lrx [B, E, V] with -0.0f, +-3e38 and denormals sprinkled over the first lap (e < Ncb: at most one per chain of
    contributions, so no sum meets two of them and inf - inf never forms) and, where some position has exactly one contribution, a
    NaN with a payload on it: a copy, whose bits are pinned (the payload of NaN + x is not)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, t.E, V)).astype(np.float32)
    u = x.view(np.uint32)
    lap0 = min(t.E, t.Ncb)
    for i in range(4 * len(SPECIALS)):
        u[rng.integers(B), rng.integers(lap0), rng.integers(V)] = SPECIALS[i % len(SPECIALS)]
    once = [es[0] for es in t.contrib if len(es) == 1]
    if once:
        u[B - 1, once[len(once) // 2], V // 2] = NAN_PAYLOAD
    return x


def channel_output(nb, t, q, B, seed, sigma=SIGMA, qam=True):
    """rx of B frames of E random symbols through the host channel: [B, E, 2] over the constellation, [B, E*m] over BPSK."""
    m = q.bit_length() - 1
    rng = np.random.default_rng(seed)
    tx = rng.integers(0, q, size=(B, t.E)).astype(np.int32)
    s = np.array([173, 173, 173], np.int32)
    length = types.SimpleNamespace(N=t.E, m=m)  # AWGNChannel_CPU reads N and m of its code argument only
    con = constellation(q) if qam else None
    return np.stack([nb.AWGNChannel_CPU(s, sigma, length, tx[b], CONSTELLATION=con) for b in range(B)])
