"""The half-row kernel's local edges after their rescheduling (csrc/bldpc_qc2_body.inc: the local edges' outputs in front of the drain
wait, the local first triple of the selection network ahead of the variable-node barrier, the leftover single's |x| as a source
modifier): hard bits, flag row, iteraTime / iterations per frame and the a-posteriori sums as uint32 bit patterns, against the CPU
oracle and against KERNEL_TABLE.

Codes.  Through the library: the shipped J4_L24_Z96 and a generated J = 4, L = 24, Z = 96 matrix with full rows of 20 from
random_blockh (the generator of the flooding shape tests): other shifts, another matching of columns to half-rows, the same
half-row width of 10.  The variant table has this one half-row entry with local edges, so a code object cannot reach the local form
at another width.  test_local_form_other_widths therefore runs the same kernel body, instantiated for full rows of 16 and of 18
(half-rows of 8 and 9: five and six values behind the local first triple, an odd and an even tail of the sign words, two leftover
singles and none) by tests/cpp/qc2_local_width_test.hip, on generated matrices of those row weights.  That program builds its
tables with the host side's own builders and launches k_qc2 / k_qc2p directly; build() compiles it (a minute per width).

max_iter 1 and 2 run no loop iteration (first phase / first iteration and the final phase), 3 runs one, 4 two, 50 is the benchmark's.
The early work meets the first-iteration path at 2, the last loop iteration and the final variable-node phase at 3 and 4.

Inputs.  (i) the seed-173 AWGN block at 3 dB, F = 2 and F = 6.  (ii) 64 frames drawn with a fixed seed from {+-0.0f, +-1 (ties), a
denormal, 3e38, ordinary values}: across the frames the two smallest magnitudes of a row fall on local edges, on stored edges, and one
on each.  test_local_form_other_widths counts the three cases over the 64 x 384 rows of the first iteration with the matching the
program reports and asserts that each occurs.  The oracle's sums stay finite on it (checked here: the kernels are defined for finite
sums)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from qc_trim_cases import path as _path
from qc_variant_cases import oracle_per_frame, write_blockh
from test_layered_shapes_cpu import random_blockh

pytestmark = pytest.mark.gpu

J, L, Z = 4, 24, 96
N = L * Z
ITERS = (1, 2, 3, 4, 50)
ALPHA = 0.8125
_MEMO = {}


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    assert torch.cuda.is_available()
    return cuda_ldpc_amd


def _matrix(which, tmp):
    """(path of the BlockH file, block shifts [J, L])"""
    if which == "shipped":
        p = _path(J, L, Z)
        return p, np.loadtxt(p, dtype=np.int32).reshape(J, L)
    H = random_blockh(J, L, Z, 4 + 24 + 96 + 20, (20,) * J)
    p = str(tmp / "generated_J4_L24_Z96_wc20.txt")
    write_blockh(p, H)
    return p, H


def _awgn(orc, F):
    return np.ascontiguousarray(orc.bldpc_awgn(np.array([173, 173, 173], np.int32), orc.bldpc_sigma(3.0), N, F).reshape(N, F))


def _special():
    """input (ii): [N, 64]"""
    if "special" not in _MEMO:
        rng = np.random.default_rng(8)
        F = 64
        y = (1.0 + 0.8 * rng.standard_normal((N, F))).astype(np.float32)
        pick = rng.random((N, F))
        for k, val in enumerate((0.0, -0.0, 1.0, -1.0, 1e-41)):
            y[(pick >= 0.08 * k) & (pick < 0.08 * (k + 1))] = val
        y[(pick >= 0.40) & (pick < 0.404)] = 3e38
        y.setflags(write=False)
        _MEMO["special"] = y
    return _MEMO["special"]


def _inputs(orc):
    return {"awgn-F2": _awgn(orc, 2), "awgn-F6": _awgn(orc, 6), "special-F64": _special()}


def _u32(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _run(C, code, y, **kw):
    r = C.LDPC_Decoder_GPU(code, torch.from_numpy(np.ascontiguousarray(y)).cuda(), want_app=True, **kw)
    torch.cuda.synchronize()
    return r


def _same(r, D, app, it, what):
    got = r["D"].cpu().numpy().reshape(-1)
    F = got.size // (N + 1)
    assert np.array_equal(got[: N * F], D.reshape(-1)[: N * F]), "hard bits differ: " + what
    assert np.array_equal(got[N * F:], D.reshape(-1)[N * F:]), "flag row differs: " + what
    assert r["iteraTime"] == it, "iteraTime differs: " + what
    assert np.array_equal(_u32(r["app"].cpu().numpy()), _u32(app)), "a-posteriori sums differ bitwise: " + what


def _cases(C, orc, which, tmp, monkeypatch, no_local):
    p, H = _matrix(which, tmp)
    ocode = orc.BinaryCode(p, J, L, Z)
    if no_local:
        monkeypatch.setenv("BLDPC_NO_LOCAL", "1")
    code = C.BinaryCode.from_shifts(H, J, L, Z)
    if no_local:
        monkeypatch.delenv("BLDPC_NO_LOCAL")
    tag = "qc_lds_halfrow<" if no_local else "qc_lds_halfrow-local<"
    for name, y in _inputs(orc).items():
        F = y.shape[1]
        yflat = np.ascontiguousarray(y).reshape(-1)
        for its in ITERS:
            what = "%s %s max_iter %d" % (which, name, its)
            # fixed iterations
            want = orc.bldpc_decode(ocode, yflat, F, its, early_exit=0, want_app=True)
            assert np.isfinite(want["app"]).all(), "the input leaves finite sums: " + what
            r = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_FIXED)
            assert code.last_kernel.startswith(tag), code.last_kernel
            _same(r, want["D"], want["app"], want["it"], "fixed, " + what)
            t = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_TABLE)
            _same(r, t["D"].cpu().numpy(), t["app"].cpu().numpy(), t["iteraTime"], "fixed against the table kernels, " + what)
            # batch-global exit
            want = orc.bldpc_decode(ocode, yflat, F, its, early_exit=1, want_app=True)
            r = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_BATCH_GLOBAL)
            assert code.last_kernel.startswith(tag), code.last_kernel
            _same(r, want["D"], want["app"], want["it"], "batch-global, " + what)
            t = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_TABLE)
            _same(r, t["D"].cpu().numpy(), t["app"].cpu().numpy(), t["iteraTime"], "batch-global against the table kernels, " + what)
            # per-frame exit
            D, app, iters = oracle_per_frame(orc, ocode, y, F, its)
            r = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_PER_FRAME)
            assert tag[:-1] in code.last_kernel, code.last_kernel
            assert np.array_equal(r["iters"].cpu().numpy(), iters), "iterations per frame differ: " + what
            _same(r, D, app, None, "per-frame, " + what)
            t = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_TABLE)
            assert np.array_equal(r["iters"].cpu().numpy(), t["iters"].cpu().numpy()), "iterations per frame against the table kernels: " + what
            _same(r, t["D"].cpu().numpy(), t["app"].cpu().numpy(), None, "per-frame against the table kernels, " + what)
            # normalised min-sum (bldpc_decode_normalised), fixed and per-frame, against its host statement
            for mode in (C.EXIT_FIXED, C.EXIT_PER_FRAME):
                want = C.normalised_host(H, J, L, Z, y, max_iter=its, alpha=ALPHA, exit_mode=mode)
                r = _run(C, code, y, max_iter=its, exit_mode=mode, alpha=ALPHA)
                assert tag[:-1] in code.last_kernel, code.last_kernel
                w = "normalised mode %d, %s" % (mode, what)
                assert np.array_equal(r["D"].cpu().numpy().reshape(-1), np.asarray(want["D"]).reshape(-1)), "D differs: " + w
                assert np.array_equal(_u32(r["app"].cpu().numpy()), _u32(want["app"])), "a-posteriori sums differ bitwise: " + w
                if mode == C.EXIT_PER_FRAME:
                    assert np.array_equal(r["iters"].cpu().numpy(), np.asarray(want["iters"])), "iterations per frame differ: " + w
    code.close()


@pytest.mark.parametrize("which", ["shipped", "generated"])
def test_local_form_bit_exact(C, orc, which, tmp_path, monkeypatch):
    _cases(C, orc, which, tmp_path, monkeypatch, no_local=False)


@pytest.mark.parametrize("which", ["shipped", "generated"])
def test_plain_form_bit_exact(C, orc, which, tmp_path, monkeypatch):
    """The same cases under BLDPC_NO_LOCAL: the half-row kernel without local edges, which this change leaves as it was."""
    _cases(C, orc, which, tmp_path, monkeypatch, no_local=True)



# ---- other half-row widths: the kernel body instantiated outside the variant table (tests/cpp/qc2_local_width_test.hip) ----------
FORMS = ("fixed", "hist", "pf", "pfp", "norm")


def _program(wch):
    """The test program of this width, from build() (compiled here if the tree was built without it)."""
    import __graft_entry__ as G
    for cmd, _ in G.stale_test_programs():
        subprocess.check_call(cmd)
    return os.path.join(G.TEST_BIN, "qc2_local_width_%d" % wch)


def _read(path, F):
    """flags [F], iters [F], hist [F], D [N, F] unpacked from the packed bits, app [N, F]"""
    raw = np.fromfile(path, np.uint8)
    NW = N // 32
    assert raw.size == F * 4 + F * 4 + F * 8 + F * NW * 4 + N * F * 4, path
    o = 0
    flags = raw[o:o + 4 * F].view(np.int32); o += 4 * F
    iters = raw[o:o + 4 * F].view(np.int32); o += 4 * F
    hist = raw[o:o + 8 * F].view(np.uint64); o += 8 * F
    bits = raw[o:o + 4 * F * NW].view(np.uint32).reshape(F, NW); o += 4 * F * NW
    app = raw[o:].view(np.float32).reshape(N, F)
    D = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(F, N).T.astype(np.int32)
    return flags, iters, hist, D, app


def _minima_cases(H, local_cols, y):
    """Where the two smallest |Q| of a check row sit in the first iteration (Q = y): rows with both on local edges, both on stored
    edges, one on each.  Ties go to the lower column."""
    both, none, one = 0, 0, 0
    t = np.arange(Z)
    for j in range(J):
        cols = np.flatnonzero(H[j] >= 0)
        idx = cols[:, None] * Z + (t[None, :] + H[j, cols][:, None]) % Z         # [w, Z] variable of edge (l, t)
        order = np.argsort(np.abs(y[idx]), axis=0, kind="stable")[:2]              # [2, Z, F]
        nloc = np.isin(cols, local_cols[j])[order].sum(0)
        both, none, one = both + int((nloc == 2).sum()), none + int((nloc == 0).sum()), one + int((nloc == 1).sum())
    return both, none, one


@pytest.mark.parametrize("wch", [8, 9])
def test_local_form_other_widths(C, orc, wch, tmp_path):
    """Half-rows of 8 and 9 edges: every exit form and the normalised one at max_iter 1, 2, 3, 4, 50 on the AWGN block (F = 6) and the
    special-value block (F = 64) in one batch of 70 frames, against the oracle, the normalised host statement and KERNEL_TABLE."""
    H = random_blockh(J, L, Z, 4 + 24 + 96 + 2 * wch, (2 * wch,) * J)
    assert ((H >= 0).sum(1) == 2 * wch).all()
    p = str(tmp_path / ("generated_J4_L24_Z96_wc%d.txt" % (2 * wch)))
    write_blockh(p, H)
    FA, F = 6, 70
    y = np.ascontiguousarray(np.concatenate([_awgn(orc, FA), _special()], axis=1))
    y.tofile(str(tmp_path / "y.bin"))
    ocode = orc.BinaryCode(p, J, L, Z)
    r = subprocess.run([_program(wch), p, str(tmp_path / "y.bin"), str(F), str(ocode.K), repr(ALPHA), str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK 25 half-row %d" % wch, r.stdout + r.stderr
    local_cols = np.loadtxt(str(tmp_path / "local.txt"), dtype=np.int64).reshape(J, 2 * (L // (2 * J)))
    assert sorted(local_cols.reshape(-1).tolist()) == list(range(L)) and all((H[j, local_cols[j]] >= 0).all() for j in range(J))
    both, none, one = _minima_cases(H, local_cols, _special())
    print("rows whose two smallest magnitudes are both local / both stored / one of each: %d / %d / %d" % (both, none, one))
    assert both > 0 and none > 0 and one > 0

    code = C.BinaryCode.from_shifts(H, J, L, Z)
    yflat = y.reshape(-1)
    for its in ITERS:
        got = {f: _read(str(tmp_path / ("%s_%d.bin" % (f, its))), F) for f in FORMS}
        what = "half-rows of %d, max_iter %d" % (wch, its)
        # fixed iterations, and the flag-tracking instantiation run to max_iter
        want = orc.bldpc_decode(ocode, yflat, F, its, early_exit=0, want_app=True)
        assert np.isfinite(want["app"]).all(), "the input leaves finite sums: " + what
        wD = want["D"].reshape(N + 1, F)
        t = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_TABLE)
        for form in ("fixed", "hist"):
            flags, _, _, D, app = got[form]
            assert np.array_equal(D, wD[:N]) and np.array_equal(flags, wD[N]), "%s: D or flag row differs: %s" % (form, what)
            assert np.array_equal(_u32(app), _u32(want["app"])), "%s: a-posteriori sums differ bitwise: %s" % (form, what)
            assert np.array_equal(np.concatenate([D, flags[None]]).reshape(-1), t["D"].cpu().numpy().reshape(-1)), "%s against the table kernels: %s" % (form, what)
            assert np.array_equal(_u32(app), _u32(t["app"].cpu().numpy())), "%s against the table kernels, sums: %s" % (form, what)
        # batch-global exit: the first iteration at which every frame of the AWGN block is flagged, from the flag histories
        wg = orc.bldpc_decode(ocode, np.ascontiguousarray(y[:, :FA]).reshape(-1), FA, its, early_exit=1)
        every = int(np.bitwise_and.reduce(got["hist"][2][:FA])) & ((1 << its) - 1)
        stop = (every & -every).bit_length() if every else its
        assert stop == wg["it"], "batch-global stop %d, the oracle's %d: %s" % (stop, wg["it"], what)
        # per-frame exit: one workgroup per pair, and persistent workgroups
        wD, wapp, witers = oracle_per_frame(orc, ocode, y, F, its)
        t = _run(C, code, y, max_iter=its, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_TABLE)
        first = np.array([(int(h) & -int(h)).bit_length() if int(h) & ((1 << its) - 1) else its for h in got["hist"][2]], np.int32)
        assert np.array_equal(first, witers), "first flag of each frame's history differs: " + what
        for form in ("pf", "pfp"):
            flags, iters, _, D, app = got[form]
            assert np.array_equal(iters, witers), "%s: iterations per frame differ: %s" % (form, what)
            assert np.array_equal(D, wD[:N]) and np.array_equal(flags, wD[N]), "%s: D or flag row differs: %s" % (form, what)
            assert np.array_equal(_u32(app), _u32(wapp)), "%s: a-posteriori sums differ bitwise: %s" % (form, what)
            assert np.array_equal(iters, t["iters"].cpu().numpy()), "%s against the table kernels, iterations: %s" % (form, what)
            assert np.array_equal(_u32(app), _u32(t["app"].cpu().numpy())), "%s against the table kernels, sums: %s" % (form, what)
        # normalised min-sum, fixed iterations, against its host statement
        wn = C.normalised_host(H, J, L, Z, y, max_iter=its, alpha=ALPHA, exit_mode=C.EXIT_FIXED)
        flags, _, _, D, app = got["norm"]
        assert np.array_equal(np.concatenate([D, flags[None]]).reshape(-1), np.asarray(wn["D"]).reshape(-1)), "normalised: D differs: " + what
        assert np.array_equal(_u32(app), _u32(wn["app"])), "normalised: a-posteriori sums differ bitwise: " + what
    code.close()
