"""Cases shared by tests/test_osd_w_cpu.py and tests/test_osd_w_gpu.py: reprocessing of order 1 and 2 (bldpc_decode_osd_w,
include/bldpc.h) on the shapes, batch sizes and inputs of tests/osd_cases.py, the (order, lambda) sets, two purpose-built frames more
on the two larger LDS shapes, and a restatement of the definition that shares no code with the host statement: the columns of H as
Python integers, reduced against the basis as osd_frame reduces them, so that every position outside B and the syndrome are known as
sums of basis members by order of joining; np.float32 sums in the stated order; the minimum over the triple.  The metrics of every
single and of every pair among the first `lam_max` positions outside B are computed once a frame, and each parameter set takes its
minimum over the part of them it admits."""
import numpy as np

from osd_cases import (BATCHES, DEFICIENT, DIMS, EXTREME, F_MAX, FIXED, WORKSPACE_DIMS, _codewords, columns, dims_id, kept_input,  # noqa: F401
                       matrix, np_syndrome, osd_input, processed_on_workspace)

PARAMS = ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (2, 12), (2, "N"))  # "N": lambda = N, which the definition clips to N - rank
WORKSPACE_PARAMS = ((0, 0), (1, 0), (2, 12))  # WORKSPACE_DIMS: a frame costs many seconds in the restatement
WORKSPACE_W_PROCESSED = 4                      # and only this many of its frames are restated
PAIR_DIMS = ((3, 9, 96), EXTREME)              # the shapes on whose ramp no pair wins: two fixed frames more
PAIR_FRAMES = 2
PAIR_MAGNITUDE = (0.8, 1.6)                    # of every position of those frames, the two wrong ones included

_cache = {}


def params(dims):
    """[(order, lambda)] with lambda an integer."""
    N = dims[1] * dims[2]
    return [(o, N if lam == "N" else lam) for o, lam in (WORKSPACE_PARAMS if tuple(dims) == WORKSPACE_DIMS else PARAMS)]


def processed_w():
    """The frames of WORKSPACE_DIMS that a call of these tests processes: two fixed frames, a clean and a noisy ramp frame."""
    return [FIXED[0], FIXED[3], 0, 36]


def n_frames(dims):
    return F_MAX + (PAIR_FRAMES if tuple(dims) in PAIR_DIMS else 0)


def batches(dims):
    return tuple(BATCHES) + ((n_frames(dims),) if tuple(dims) in PAIR_DIMS else ())


def frames_of(dims):
    return processed_w() if tuple(dims) == WORKSPACE_DIMS else list(range(n_frames(dims)))


def pair_frame_positions(dims, k):
    """The two positions made wrong in extra frame k."""
    osd_w_input(dims)
    return _cache[("wrong", tuple(dims))][k]


def osd_w_input(dims):
    """(app float32 [N, n_frames], the words sent): osd_input(dims), unaltered, and on PAIR_DIMS two columns more.  Each of those is
    the word sent at magnitudes uniform in PAIR_MAGNITUDE (a position in no check 1.0 higher, so that it comes last and the first places
    outside the basis are positions a check sees) with two positions wrong, both among the first 12 positions outside the basis
    of the frame (which depends on the magnitudes alone): the first pair of them, by place, not yet used, for which the restatement at
    (2, 12) returns the word sent with exactly that pair picked.  (A pair loses to a single wherever one of its columns is the sum of
    one or two basis columns, which is common on EXTREME.)"""
    dims = tuple(dims)
    key = ("in", dims)
    if key not in _cache:
        app, cw = osd_input(dims)
        if dims in PAIR_DIMS:
            J, L, Z = dims
            N = L * Z
            cols = columns(matrix(dims), Z)
            rng = np.random.default_rng(5000 + N)
            extra, words, wrong = [], [], []
            for k in range(PAIR_FRAMES):
                word = cw[:, (7 + 5 * k) % F_MAX]
                mag = rng.uniform(*PAIR_MAGNITUDE, N) + np.asarray([1.0 if col == 0 else 0.0 for col in cols])  # a position in no check: last
                clean = ((1.0 - 2.0 * word) * mag).astype(np.float32)
                fr = Frame(cols, J * Z, clean, 0)
                first, order = fr.outside[:12], fr.order
                for i, j in ((i, j) for i in range(12) for j in range(i + 1, 12)):
                    pos = [order[first[i]], order[first[j]]]
                    if pos in wrong:
                        continue
                    a = clean.copy()
                    a[pos] = -a[pos]
                    c, _, picked, _, _ = Frame(cols, J * Z, a, 12).result(2, 12)
                    if picked == pos and np.array_equal(c, word):
                        break
                else:
                    raise AssertionError("no pair among the first 12 positions outside B wins")
                extra.append(a)
                words.append(word)
                wrong.append(pos)
            app = np.concatenate([app, np.stack(extra, 1)], 1)
            cw = np.concatenate([cw, np.stack(words, 1)], 1)
            _cache[("wrong", dims)] = wrong
        app = np.ascontiguousarray(app)
        app.setflags(write=False)
        _cache[key] = (app, cw)
    return _cache[key]


def kept_w_input(dims, F):
    """D_in for the first F frames: kept_input of osd_cases.py; the extra frames are processed; on WORKSPACE_DIMS only processed_w()."""
    dims = tuple(dims)
    N = dims[1] * dims[2]
    D = kept_input(dims, min(F, F_MAX))
    if F > F_MAX:
        more = np.random.default_rng(78).integers(-5, 6, size=(N + 1, F - F_MAX)).astype(np.int32)
        more[N] = 0
        D = np.concatenate([D, more], 1)
    if dims == WORKSPACE_DIMS:
        keep = np.ones(F, bool)
        keep[[f for f in processed_w() if f < F]] = False
        D[N] = np.where(keep, np.arange(F) + 2, 0)
    return np.ascontiguousarray(D)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _bits(x, n):
    """Python integer -> bool [n], bit k first."""
    return np.unpackbits(np.frombuffer(x.to_bytes((n + 7) // 8 + 1, "little"), np.uint8), bitorder="little")[:n].astype(bool)


def metric_bits(m):
    m = np.asarray(m, np.float32)
    return np.where(np.isnan(m), np.uint32(0x7FFFFFFF), m.view(np.uint32))


def _sums(E, wB):
    """E bool [rank, n]: per column m = +0.0f, then m += wB[k] for k ascending where E[k]: np.float32, no term skipped or reordered."""
    m = np.zeros(E.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for k in range(E.shape[0]):
            m[E[k]] += wB[k]
    return m


class Frame:
    """One frame on Python integers.  order: place -> position; B: the basis in joining order; outside: the places outside B,
    ascending; w: float32 by position; m0, m1 [n_out], m2 [lam_max, lam_max] (above the diagonal): the metrics of the candidates."""

    def __init__(self, cols, M, a, lam_max):
        a = np.ascontiguousarray(a, np.float32)
        N = a.size
        self.y = (a < 0).astype(np.int64)
        keys = (a.view(np.uint32) & np.uint32(0x7FFFFFFF))
        self.w = keys.view(np.float32)
        srt = sorted((k, v) for v, k in enumerate(keys.tolist()))
        self.order = [v for _, v in srt]
        basis, B, self.scanned = {}, [], 0
        combo_of = {}  # position outside B -> the members of B its column is the sum of
        for place, v in enumerate(self.order):
            vec, combo = cols[v], 0
            while vec:
                low = (vec & -vec).bit_length() - 1
                if low not in basis:
                    basis[low] = (vec, combo | (1 << len(B)))
                    B.append(v)
                    self.scanned = place + 1
                    break
                vec ^= basis[low][0]
                combo ^= basis[low][1]
            else:
                combo_of[v] = combo
        self.B, self.rank = B, len(B)
        inB = set(B)
        self.outside = [p for p, v in enumerate(self.order) if v not in inB]
        s = 0
        for v in np.flatnonzero(self.y).tolist():
            s ^= cols[v]
        combo = 0
        while s:
            low = (s & -s).bit_length() - 1
            s ^= basis[low][0]
            combo ^= basis[low][1]
        rank, n_out = self.rank, len(self.outside)
        self.e0 = _bits(combo, rank)
        self.C = np.zeros((rank, n_out), bool)
        for q, p in enumerate(self.outside):
            self.C[:, q] = _bits(combo_of[self.order[p]], rank)
        self.wB = self.w[np.asarray(B, np.int64)] if rank else np.zeros(0, np.float32)
        self.wS = self.w[np.asarray([self.order[p] for p in self.outside], np.int64)] if n_out else np.zeros(0, np.float32)
        self.m0 = _sums(self.e0[:, None], self.wB)[0]
        with np.errstate(all="ignore"):
            self.m1 = _sums(self.e0[:, None] ^ self.C, self.wB) + self.wS
            lam = min(lam_max, n_out)
            self.m2 = np.full((lam, lam), np.float32(np.nan), np.float32)
            i, j = np.triu_indices(lam, 1)
            for lo in range(0, i.size, 8192):
                ii, jj = i[lo:lo + 8192], j[lo:lo + 8192]
                self.m2[ii, jj] = (_sums(self.e0[:, None] ^ self.C[:, ii] ^ self.C[:, jj], self.wB) + self.wS[ii]) + self.wS[jj]
        self.lam_max = lam_max

    def select(self, order, lam):
        """The least triple (metric bits, place + 1, place + 1) and how many admitted candidates have its metric bits."""
        n_out = len(self.outside)
        cands = [(int(metric_bits(self.m0)), 0, 0)]
        least = [cands[0][0]]
        counts = [np.asarray([cands[0][0]], np.int64)]
        if order >= 1 and n_out:
            b = metric_bits(self.m1).astype(np.int64)
            q = int(np.argmin(b))  # the first of the least: the lowest place
            cands.append((int(b[q]), self.outside[q] + 1, 0))
            counts.append(b)
        lam = min(lam, n_out) if order >= 2 else 0
        assert lam <= min(self.lam_max, n_out), "the restatement was made for a smaller lambda"
        if lam >= 2:
            b = metric_bits(self.m2[:lam, :lam]).astype(np.int64)
            b[np.tril_indices(lam)] = 1 << 40
            q1, q2 = divmod(int(np.argmin(b)), lam)  # row-major: the lowest first place, then the lowest second
            cands.append((int(b[q1, q2]), self.outside[q1] + 1, self.outside[q2] + 1))
            counts.append(b.ravel())
        best = min(cands)
        return best, int(sum((c == best[0]).sum() for c in counts))

    def result(self, order, lam):
        """(c int64 [N], flips, picked [2], metric float32, ties) of the selection."""
        (_, p1, p2), ties = self.select(order, lam)
        e = self.e0.copy()
        pos = [self.order[p - 1] for p in (p1, p2) if p]
        m = self.m0
        if p1:
            q1 = self.outside.index(p1 - 1)
            e ^= self.C[:, q1]
            m = self.m1[q1]
            if p2:
                q2 = self.outside.index(p2 - 1)
                e ^= self.C[:, q2]
                m = self.m2[q1, q2]
        c = self.y.copy()
        c[np.asarray(self.B, np.int64)[e]] ^= 1
        c[pos] ^= 1
        return c, int(e.sum()) + len(pos), pos + [-1] * (2 - len(pos)), np.float32(m), ties


def np_frames(dims):
    """frame -> Frame of osd_w_input(dims), for frames_of(dims), computed once."""
    dims = tuple(dims)
    key = ("frames", dims)
    if key not in _cache:
        J, L, Z = dims
        app, _ = osd_w_input(dims)
        cols = columns(matrix(dims), Z)
        lam_max = max(lam for _, lam in params(dims))
        _cache[key] = {f: Frame(cols, J * Z, app[:, f], lam_max) for f in frames_of(dims)}
    return _cache[key]


def np_w_all(dims, order, lam):
    """The restatement at one parameter set: dict(c [N, n], flips, scanned [n], picked [2, n], metric [n], ties [n]); -99 / NaN on the
    frames of WORKSPACE_DIMS that are not restated."""
    dims = tuple(dims)
    key = ("all", dims, order, lam)
    if key not in _cache:
        N, n = dims[1] * dims[2], n_frames(dims)
        r = dict(c=np.full((N, n), -99, np.int32), flips=np.full(n, -99, np.int32), scanned=np.full(n, -99, np.int32),
                 picked=np.full((2, n), -99, np.int32), metric=np.full(n, np.nan, np.float32), ties=np.zeros(n, np.int32))
        for f, fr in np_frames(dims).items():
            r["c"][:, f], r["flips"][f], r["picked"][:, f], r["metric"][f], r["ties"][f] = fr.result(order, lam)
            r["scanned"][f] = fr.scanned
        _cache[key] = r
    return _cache[key]


def np_w_outputs(dims, F, order, lam, D_in=None):
    """(D [N+1, F], flips, scanned [F], picked [2, F], metric bits uint32 [F], processed bool [F]) of the first F frames."""
    a = np_w_all(dims, order, lam)
    N = dims[1] * dims[2]
    D = np.concatenate([a["c"][:, :F], np.ones((1, F), np.int32)], 0).astype(np.int32)
    flips, scanned, picked = a["flips"][:F].copy(), a["scanned"][:F].copy(), a["picked"][:, :F].copy()
    done = np.ones(F, bool)
    if D_in is not None:
        kept = D_in[N] != 0
        D[:, kept] = D_in[:, kept]
        flips[kept], scanned[kept], picked[:, kept] = -1, 0, -1
        done = ~kept
    assert (D[:N] != -99).all() and (flips != -99).all(), "a frame of WORKSPACE_DIMS outside processed_w() is processed"
    return D, flips, scanned, picked, metric_bits(a["metric"][:F]), done
