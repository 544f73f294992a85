"""The case table of tests/test_qc_variants_gpu.py and tests/test_qc_variants_cpu.py: for every entry of the fused binary kernels'
variant table (qc_variants() in csrc/bldpc_qc_kernel.hpp, read through cuda_ldpc_amd.qc_variants()) at least one matrix, the
switches or the pin under which a code object lands on that entry, and the Es/N0 at which its early exits are exercised.

No index is written down here: every case finds its entry in the table by what the entry is (tag, shape, NG), so removing or
adding an entry moves the indices without touching the cases -- and an entry without a case fails the CPU test.

Matrices are the shipped ones, seeded random block matrices (the generator of test_other_lifting_sizes_random_matrices) or a
shipped block pattern with seeded random shifts.  The oracle results the tests compare with are computed once per (matrix, Es/N0)
and shared by the cases that use the same matrix."""
import collections
import os
import tempfile

import numpy as np

from conftest import DATA

BL = os.path.join(DATA, "bldpc")

SHIPPED = {"PON_LDPC": (12, 69, 256)}
for _f in sorted(os.listdir(BL)):
    if _f.endswith("_BlockH.txt"):
        _J, _L, _Z = (int(x[1:]) for x in _f[:-len("_BlockH.txt")].split("_"))
        SHIPPED["J%d_L%d_Z%d" % (_J, _L, _Z)] = (_J, _L, _Z)


def shipped_path(name):
    return os.path.join(BL, "PON_LDPC.txt" if name == "PON_LDPC" else name + "_BlockH.txt")


def random_block_matrix(Z, J, L):
    """A seeded random block matrix: about 55 % of the blocks, every column keeps at least two blocks, every row at least three."""
    rng = np.random.default_rng(Z + J)
    H = rng.integers(0, Z, size=(J, L)).astype(np.int32)
    H[rng.random((J, L)) < 0.45] = -1
    for l in range(L):
        rows = rng.permutation(J)[:2]
        for r in rows:
            if H[r, l] < 0:
                H[r, l] = rng.integers(0, Z)
    for j in range(J):
        cols = rng.permutation(L)[:3]
        for c in cols:
            if H[j, c] < 0:
                H[j, c] = rng.integers(0, Z)
    return H


def random_shifts(name, seed):
    """The block pattern of a shipped matrix with seeded random shifts."""
    J, L, Z = SHIPPED[name]
    base = np.loadtxt(shipped_path(name), dtype=np.int64).reshape(J, L)
    rng = np.random.default_rng(seed)
    return np.where(base >= 0, rng.integers(0, Z, size=(J, L)), -1).astype(np.int32)


def write_blockh(path, H):
    with open(path, "w") as f:
        for row in H:
            f.write("\t".join(str(int(x)) for x in row) + "\r\n")


def max_wrapped(H, Z):
    """The halo kernels' wrap count restated: shifts are taken relative to the first block column that meets every block row;
    a block wraps in tile t when its 64 rotated positions starting at 64 t run past Z.  Returns the largest number of wrapped
    blocks of one (block row, tile); an entry with NG slots takes the matrix when this is <= NG.  None: no full column."""
    J, L = H.shape
    full = np.flatnonzero((H >= 0).sum(0) == J)
    if len(full) == 0 or Z % 64:
        return None
    lc = int(full[0])
    worst = 0
    for j in range(J):
        rot = int(H[j, lc])
        rel = [(int(H[j, l]) - rot) % Z for l in range(L) if l != lc and H[j, l] >= 0]
        for t in range(Z // 64):
            worst = max(worst, sum(1 for s in rel if (64 * t + s) % Z > Z - 64))
    return worst


# ---- matrices: ("shipped", name) | ("random", Z, J, L) | ("shifts", name, seed) ------------------------------------------------
_TMP = tempfile.TemporaryDirectory(prefix="qc_variant_cases_")
_MAT = {}


def matrix(spec):
    """-> (path of a BlockH file, H int32 [J, L], J, L, Z); generated matrices are written once into a temporary directory."""
    if spec not in _MAT:
        if spec[0] == "shipped":
            J, L, Z = SHIPPED[spec[1]]
            path = shipped_path(spec[1])
            H = np.loadtxt(path, dtype=np.int64).reshape(J, L).astype(np.int32)
        else:
            if spec[0] == "random":
                _, Z, J, L = spec
                H = random_block_matrix(Z, J, L)
            else:
                J, L, Z = SHIPPED[spec[1]]
                H = random_shifts(spec[1], spec[2])
            path = os.path.join(_TMP.name, "_".join(str(x) for x in spec) + ".txt")
            write_blockh(path, H)
        _MAT[spec] = (path, H, J, L, Z)
    return _MAT[spec]


# Es/N0 per matrix, found with the oracle alone (test_qc_variants_cpu.py checks what the GPU tests rely on): the batch of
# 5 frames of the seed (173, 173, 173) stops, under the reference's batch-global rule, strictly between iteration 1 and
# MAXIT_GLOBAL, and its frames, each on its own flag, stop at different iterations.
SNR = {
    ("shipped", "J4_L24_Z96"): 2.7,
    ("shipped", "J8_L24_Z96"): 1.0,
    ("shipped", "J12_L24_Z96"): 0.0,
    ("shipped", "J6_L24_Z96"): 2.0,
    ("shipped", "J32_L64_Z64"): -0.9,
    ("shipped", "J4_L24_Z256"): 2.8,
    ("shipped", "PON_LDPC"): 2.5,
    ("shipped", "J4_L24_Z512"): 3.6,
    ("shifts", "J4_L24_Z512", 2): 3.6,
    ("random", 256, 5, 14): 1.0,
    ("random", 512, 3, 10): 1.0,
    ("shipped", "J10_L60_Z160"): 3.0,
    ("shipped", "J48_L60_Z160"): -3.0,
    ("random", 64, 5, 12): 1.0,
    ("random", 96, 3, 9): 1.0,
    ("random", 128, 6, 20): 1.8,
    ("random", 192, 4, 16): 1.8,
    ("random", 320, 5, 11): 1.0,
    ("random", 384, 3, 24): 3.5,
    ("random", 640, 4, 10): 0.9,
    ("random", 1024, 3, 8): 1.0,
    ("shipped", "J15_L30_Z1280"): 0.3,
    ("shifts", "J15_L30_Z1280", 3): 0.3,
}
MAXIT_GLOBAL = 40   # batch-global and per-frame exits
MAXIT_PERSIST = 50  # the persistent form, as PERSIST_CODES of test_bldpc_gpu.py
F_EXIT = 5          # the ragged batch of the early-exit modes
F_FIXED = 6         # fixed iterations: F = 1, 5 and 6 are the leading columns of this batch
F_BLOCK = 64        # the block the persistent form's batch is tiled from
OTHER_LIFTING_SIZES = [(64, 5, 12), (96, 3, 9), (128, 6, 20), (192, 4, 16), (320, 5, 11), (384, 3, 24), (640, 4, 10), (1024, 3, 8)]

Case = collections.namedtuple("Case", "id variant matrix env snr")


def find_variant(variants, tag, **want):
    """The index of THE entry with this tag and these fields (CPT carries NG on the halo entries)."""
    hits = [v["index"] for v in variants if v["tag"] == tag and all(v[k] == x for k, x in want.items())]
    assert len(hits) == 1, "variant table: %d entries match %s %s" % (len(hits), tag, want)
    return hits[0]


def build_cases(variants):
    """The case table from cuda_ldpc_amd.qc_variants()."""
    cases = []

    def add(ident, vi, spec, env=None, pin=False):
        env = dict(env or {})
        if pin:
            env["BLDPC_QC_VARIANT"] = str(vi)
        cases.append(Case(ident, vi, spec, env, SNR[spec]))

    def fv(tag, **kw):
        return find_variant(variants, tag, **kw)

    no_local, no_halo = {"BLDPC_NO_LOCAL": "1"}, {"BLDPC_NO_HALO": "1"}
    # the half-row kernels
    add("halfrow-local-J4", fv("halfrow-local", J=4, Z=96), ("shipped", "J4_L24_Z96"))
    add("halfrow-J4-nolocal", fv("halfrow", J=4, Z=96), ("shipped", "J4_L24_Z96"), no_local)
    for J in (8, 12, 6):
        add("halfrow-J%d" % J, fv("halfrow", J=J, Z=96), ("shipped", "J%d_L24_Z96" % J))
    # the row kernels
    add("row-local-J32", fv("row-local", J=32, Z=64), ("shipped", "J32_L64_Z64"))
    add("row-J32-nolocal", fv("row", J=32, Z=64), ("shipped", "J32_L64_Z64"), no_local)
    for J in (4, 8, 12, 6):  # behind the half-row entries: reachable by pin only
        add("row-J%d-pinned" % J, fv("row", J=J, Z=96), ("shipped", "J%d_L24_Z96" % J), pin=True)
    add("row-nf1-Z256", fv("row", NF=1, J=4, Z=256), ("shipped", "J4_L24_Z256"))
    # check states in registers
    add("regstate-PON", fv("regstate", J=12, Z=256), ("shipped", "PON_LDPC"))
    add("halo-Z512", fv("regstate-halo", J=4, Z=512), ("shipped", "J4_L24_Z512"))
    add("regstate-Z512-nohalo", fv("regstate", J=4, Z=512), ("shipped", "J4_L24_Z512"), no_halo)
    add("regstate-Z512-shifts", fv("regstate", J=4, Z=512), ("shifts", "J4_L24_Z512", 2))
    add("halo-J15-ng2", fv("regstate-halo", J=15, Z=1280, CPT=2), ("shipped", "J15_L30_Z1280"))
    add("halo-J15-ng3-pinned", fv("regstate-halo", J=15, Z=1280, CPT=3), ("shipped", "J15_L30_Z1280"), pin=True)
    add("halo-J15-ng3-shifts", fv("regstate-halo", J=15, Z=1280, CPT=3), ("shifts", "J15_L30_Z1280", 3))
    add("regstate-J15-nohalo", fv("regstate", J=15, Z=1280), ("shipped", "J15_L30_Z1280"), no_halo)
    # compressed check states
    add("compressed-Z256-random", fv("compressed", Z=256), ("random", 256, 5, 14))
    add("compressed-Z256-PON-pinned", fv("compressed", Z=256), ("shipped", "PON_LDPC"), pin=True)
    add("compressed-Z512-random", fv("compressed", Z=512), ("random", 512, 3, 10))
    add("compressed-Z512-J4-pinned", fv("compressed", Z=512), ("shipped", "J4_L24_Z512"), pin=True)
    add("compressed-Z160-J10", fv("compressed", Z=160), ("shipped", "J10_L60_Z160"))
    add("compressed-Z160-J48", fv("compressed", Z=160), ("shipped", "J48_L60_Z160"))
    for Z, J, L in OTHER_LIFTING_SIZES:
        add("compressed-Z%d-random" % Z, fv("compressed", Z=Z), ("random", Z, J, L))
    return cases


def cases():
    import cuda_ldpc_amd
    return build_cases(cuda_ldpc_amd.qc_variants())


# ---- inputs and oracle results, once per (matrix, Es/N0) -----------------------------------------------------------------------
_ORC = {}


def _memo(key, fn):
    if key not in _ORC:
        _ORC[key] = fn()
    return _ORC[key]


def channel(orc, spec, snr, F):
    """float32 [N * F], frame-fastest: the reference's channel from the seed (173, 173, 173)."""
    _, _, _, L, Z = matrix(spec)
    return _memo(("y", spec, snr, F), lambda: orc.bldpc_awgn(np.array((173, 173, 173), np.int32), orc.bldpc_sigma(snr), L * Z, F))


def ocode(orc, spec):
    path, _, J, L, Z = matrix(spec)
    return _memo(("code", spec), lambda: orc.BinaryCode(path, J, L, Z))


def oracle_per_frame(orc, oc, y, F, max_iter, length=None):
    """The reference's early-exit rule on every frame alone: D [N+1, F], app [N, F], iterations [F]."""
    N = oc.N
    yy = np.ascontiguousarray(y, np.float32).reshape(N, F)
    D = np.zeros((N + 1, F), np.int32)
    app = np.zeros((N, F), np.float32)
    iters = np.zeros(F, np.int32)
    for f in range(F):
        w = orc.bldpc_decode(oc, np.ascontiguousarray(yy[:, f]), 1, max_iter, early_exit=1, length=length, want_app=True)
        D[:, f] = w["D"]
        app[:, f] = w["app"]
        iters[f] = w["it"]
    return D, app, iters


def want_fixed(orc, spec, snr, its):
    """Fixed iterations on the batch of F_FIXED frames; frames do not interact, so its leading columns are smaller batches."""
    return _memo(("fixed", spec, snr, its),
                 lambda: orc.bldpc_decode(ocode(orc, spec), channel(orc, spec, snr, F_FIXED), F_FIXED, its, early_exit=0, want_app=True))


def want_global(orc, spec, snr, length=None):
    return _memo(("global", spec, snr, length),
                 lambda: orc.bldpc_decode(ocode(orc, spec), channel(orc, spec, snr, F_EXIT), F_EXIT, MAXIT_GLOBAL, early_exit=1, length=length,
                                          want_app=True))


def want_per_frame(orc, spec, snr, length=None):
    return _memo(("pf", spec, snr, length),
                 lambda: oracle_per_frame(orc, ocode(orc, spec), channel(orc, spec, snr, F_EXIT), F_EXIT, MAXIT_GLOBAL, length))


def want_block(orc, spec, snr, maxit):
    return _memo(("block", spec, snr, maxit),
                 lambda: oracle_per_frame(orc, ocode(orc, spec), channel(orc, spec, snr, F_BLOCK), F_BLOCK, maxit))


def special_values(N, F):
    """The input of test_tier_kernels_special_values: +-0, denormals, +-3e38 and tied +-0.5 among normal draws."""
    rng = np.random.default_rng(11)
    y = rng.standard_normal(N * F).astype(np.float32)
    for val, cnt in ((0.0, N // 8), (-0.0, N // 8), (1e-41, N // 16), (-3e-42, N // 16), (3e38, N // 64), (-3e38, N // 64), (0.5, N // 2),
                     (-0.5, N // 2)):
        y[rng.integers(0, N * F, cnt)] = val
    return y
