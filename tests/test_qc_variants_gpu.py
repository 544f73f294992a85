"""Every ahead-of-time variant of the fused binary kernels (qc_variants(), csrc/bldpc_qc_kernel.hpp) in every exit mode.

qc_plan_build takes the FIRST table entry that accepts a matrix, so tests that create codes and check whatever was picked
cover what the order of the table lets them cover.  Here every case of qc_variant_cases.py names the entry it is meant for and
asserts, through bldpc_code_qc_info, that the code object did land on it (a refused pin is a failure); each case then runs the
entry's kernels -- fn (fixed iterations), fn_hist (flag history, batch-global passes, per-frame exit of small batches) and
fn_pf (the persistent per-frame form) -- and compares hard bits, flag row, a-posteriori sums (as uint32), iteration counts and
flag histories bit for bit with the CPU oracle, with the table kernels as a second witness.

Outside the matrix: BLDPC_REGROUP, BLDPC_LOCAL_PER_FRAME, a pinned row-local variant, and the ran_to_max hint that reorders the
passes of the batch-global rule between calls on one code object.

All switches are set around BinaryCode.from_blockh only: they are read once, when the plan is built."""
import numpy as np
import pytest
import torch

import qc_variant_cases as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def _variants():
    import cuda_ldpc_amd
    return cuda_ldpc_amd.qc_variants()


VARIANTS = _variants()
CASES = Q.build_cases(VARIANTS)
IDS = [c.id for c in CASES]


def _make(C, monkeypatch, spec, env):
    """A code object of the matrix built under the switches of `env` (set for the creation only)."""
    path, _, J, L, Z = Q.matrix(spec)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    for k in env:
        monkeypatch.delenv(k)
    return code


def _case_code(C, monkeypatch, case):
    code = _make(C, monkeypatch, case.matrix, case.env)
    assert code.qc_variant == case.variant, "%s: the plan is variant %d (%s), the case is meant for %d (%s)" % (
        case.id, code.qc_variant, VARIANTS[code.qc_variant]["tag"] if code.qc_variant >= 0 else "none", case.variant, VARIANTS[case.variant]["tag"])
    return code


def _pf_variant(code):
    """The table entry that serves the per-frame passes of this code object."""
    return VARIANTS[code.qc_variant_per_frame if code.qc_variant_per_frame >= 0 else code.qc_variant]


def _named(code, v):
    assert ("qc_lds_%s<" % v["tag"]) in code.last_kernel and ("Z%d," % v["Z"]) in code.last_kernel, (code.last_kernel, v)


def _dev(y, N, F):
    return torch.from_numpy(np.ascontiguousarray(y, np.float32).reshape(N, F)).cuda()


def _misaligned(y, N, F):
    """The same values behind a data pointer 4 bytes off 8-byte alignment."""
    buf = torch.empty(N * F + 1, dtype=torch.float32, device="cuda")
    yt = buf[1:].view(N, F)
    yt.copy_(torch.from_numpy(np.ascontiguousarray(y, np.float32).reshape(N, F)))
    assert yt.is_contiguous() and yt.data_ptr() % 8 == 4
    return yt


def _decode(C, code, yt, **kw):
    r = C.LDPC_Decoder_GPU(code, yt, want_app=True, **kw)
    torch.cuda.synchronize()
    out = dict(D=r["D"].cpu().numpy(), it=r["iteraTime"], app=r["app"].cpu().numpy())
    out["flag_hist"] = None if r["flag_hist"] is None else r["flag_hist"].cpu().numpy().view(np.uint64)
    if r.get("iters") is not None:
        out["iters"] = r["iters"].cpu().numpy()
    return out


def _same(got, D, app, it=None, hist=None, its_run=None, what=""):
    assert np.array_equal(got["D"][:-1], D[:-1]), what + ": hard bits differ"
    assert np.array_equal(got["D"][-1], D[-1]), what + ": flag row differs"
    assert np.array_equal(got["app"].view(np.uint32), app.view(np.uint32)), what + ": a-posteriori sums differ bitwise"
    if it is not None:
        assert got["it"] == it, what + ": iteration count %s, oracle %s" % (got["it"], it)
    if hist is not None:
        mask = np.uint64((1 << min(its_run, 64)) - 1)
        assert np.array_equal(got["flag_hist"] & mask, hist & mask), what + ": flag histories differ"


def _same_pf(got, want, what=""):
    Dw, appw, itw = want
    assert np.array_equal(got["iters"], itw), what + ": iteration counts %s, oracle %s" % (got["iters"], itw)
    assert np.array_equal(got["D"], Dw), what + ": hard bits / flags differ"
    assert np.array_equal(got["app"].view(np.uint32), appw.view(np.uint32)), what + ": a-posteriori sums differ bitwise"


def _cols(w, N, F0, F):
    """The leading F frames of an oracle result on F0 frames: D [N+1, F], app [N, F], hist [F]."""
    return w["D"].reshape(N + 1, F0)[:, :F], w["app"].reshape(N, F0)[:, :F], w["flag_hist"][:F]


def test_code_objects_land_where_the_host_view_says(C, monkeypatch):
    """No kernel runs here: for every case, the code object created under the case's environment reports the variant and the
    nested per-frame variant that qc_plan_host computes, without a device, for the same matrix and switches."""
    for case in CASES:
        code = _make(C, monkeypatch, case.matrix, case.env)
        _, H, _, _, Z = Q.matrix(case.matrix)
        host = C.qc_plan_host(H, Z, pin=int(case.env.get("BLDPC_QC_VARIANT", -1)), no_local="BLDPC_NO_LOCAL" in case.env,
                              no_halo="BLDPC_NO_HALO" in case.env)
        assert (code.qc_variant, code.qc_variant_per_frame) == (host.variant, host.variant_per_frame), case.id
        assert code.frames_per_wg == host.frames_per_wg, case.id


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixed_iterations(C, orc, monkeypatch, case):
    """fn and fn_hist at 1, 2 and 7 iterations, F = 1, 5 and 6 (odd batches take the regrouped input, even ones of the two-frame
    kernels the in-place read), and for the two-frame kernels F = 6 behind a pointer that is not 8-byte aligned."""
    code = _case_code(C, monkeypatch, case)
    v = VARIANTS[case.variant]
    _, _, _, L, Z = Q.matrix(case.matrix)
    N = L * Z
    y6 = Q.channel(orc, case.matrix, case.snr, Q.F_FIXED).reshape(N, Q.F_FIXED)
    for its in (1, 2, 7):
        w = Q.want_fixed(orc, case.matrix, case.snr, its)
        for F in (1, 5, 6):
            D, app, hist = _cols(w, N, Q.F_FIXED, F)
            yt = _dev(y6[:, :F], N, F)
            for want_hist in (False, True):
                got = _decode(C, code, yt, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, want_flag_hist=want_hist)
                _named(code, v)
                _same(got, D, app, its, hist if want_hist else None, its, "%s its=%d F=%d hist=%d" % (case.id, its, F, want_hist))
        if v["NF"] == 2:
            D, app, hist = _cols(w, N, Q.F_FIXED, 6)
            yt = _misaligned(y6, N, 6)
            for want_hist in (False, True):
                got = _decode(C, code, yt, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, want_flag_hist=want_hist)
                _same(got, D, app, its, hist if want_hist else None, its, "%s its=%d F=6 misaligned hist=%d" % (case.id, its, want_hist))
    D, app, hist = _cols(w, N, Q.F_FIXED, 5)  # second witness: the table kernels, 7 iterations
    got = _decode(C, code, _dev(y6[:, :5], N, 5), max_iter=7, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_TABLE, want_flag_hist=True)
    _same(got, D, app, 7, hist, 7, case.id + " table")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_batch_global(C, orc, monkeypatch, case):
    """The reference's rule on a ragged batch that stops strictly inside (1, max_iter): a per-frame pass, then fn_hist."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F = L * Z, Q.F_EXIT
    w = Q.want_global(orc, case.matrix, case.snr)
    assert 1 < w["it"] < Q.MAXIT_GLOBAL, "pick an SNR at which the batch converges before max_iter (it=%d)" % w["it"]
    D, app, hist = _cols(w, N, F, F)
    yt = _dev(Q.channel(orc, case.matrix, case.snr, F), N, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_QC_LDS, want_flag_hist=True)
    _named(code, VARIANTS[case.variant])
    _same(got, D, app, w["it"], hist, w["it"], case.id)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_QC_LDS)  # without the caller's history
    _same(got, D, app, w["it"], what=case.id + " no history")
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_TABLE, want_flag_hist=True)
    _same(got, D, app, w["it"], hist, w["it"], case.id + " table")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_per_frame_exit(C, orc, monkeypatch, case):
    """A ragged batch whose frames stop at different iterations, each equal to the oracle's decode of that frame alone."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F = L * Z, Q.F_EXIT
    want = Q.want_per_frame(orc, case.matrix, case.snr)
    assert len(set(want[2].tolist())) > 1, "pick an SNR at which frames stop at different iterations (%s)" % want[2]
    yt = _dev(Q.channel(orc, case.matrix, case.snr, F), N, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS)
    _named(code, _pf_variant(code))
    _same_pf(got, want, case.id)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_TABLE)
    _same_pf(got, want, case.id + " table")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_partial_length(C, orc, monkeypatch, case):
    """length = Z + 37: not a multiple of 32, ends inside the second block column.  Fixed iterations with the history, and the
    per-frame exit (whose flags it decides)."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F, length = L * Z, Q.F_EXIT, Z + 37
    y = Q.channel(orc, case.matrix, case.snr, F)
    yt = _dev(y, N, F)
    w = orc.bldpc_decode(Q.ocode(orc, case.matrix), y, F, 7, early_exit=0, length=length, want_app=True)
    D, app, hist = _cols(w, N, F, F)
    for kern in (C.KERNEL_QC_LDS, C.KERNEL_TABLE):
        got = _decode(C, code, yt, max_iter=7, length=length, exit_mode=C.EXIT_FIXED, kernel=kern, want_flag_hist=True)
        _same(got, D, app, 7, hist, 7, "%s fixed kernel=%d" % (case.id, kern))
    want = Q.want_per_frame(orc, case.matrix, case.snr, length)
    for kern in (C.KERNEL_QC_LDS, C.KERNEL_TABLE):
        got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, length=length, exit_mode=C.EXIT_PER_FRAME, kernel=kern)
        _same_pf(got, want, "%s per-frame kernel=%d" % (case.id, kern))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_special_values(C, orc, monkeypatch, case):
    """+-0, denormals, +-3e38 and tied +-0.5 (duplicated minima, zero magnitudes), F = 3, 6 iterations."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F = L * Z, 3
    y = Q.special_values(N, F)
    w = orc.bldpc_decode(Q.ocode(orc, case.matrix), y, F, 6, early_exit=0, want_app=True)
    D, app, hist = _cols(w, N, F, F)
    yt = _dev(y, N, F)
    for kern in (C.KERNEL_QC_LDS, C.KERNEL_TABLE):
        got = _decode(C, code, yt, max_iter=6, exit_mode=C.EXIT_FIXED, kernel=kern, want_flag_hist=True)
        _same(got, D, app, 6, hist, 6, "%s kernel=%d" % (case.id, kern))


def _serves_persistent(case):
    """Cases whose per-frame passes run on an entry with a persistent kernel.  The row kernel with local edges hands them to the
    plain row entry it carries (which has one) unless it is pinned."""
    v = VARIANTS[case.variant]
    return v["has_pf"] or (v["loc"] == 2 and "BLDPC_QC_VARIANT" not in case.env)


PERSIST_CASES = [c for c in CASES if _serves_persistent(c)]


@pytest.mark.parametrize("case", PERSIST_CASES, ids=[c.id for c in PERSIST_CASES])
def test_persistent_form(C, orc, monkeypatch, case):
    """fn_pf: a batch just large enough that the dispatched grid exceeds persist_grid, tiled from a block of 64 frames.  Same
    result as a code object built under BLDPC_NO_PERSIST=1; first and last tile and the ragged tail equal the oracle's decodes
    of the block's frames, each alone."""
    code = _case_code(C, monkeypatch, case)
    plain = _make(C, monkeypatch, case.matrix, dict(case.env, BLDPC_NO_PERSIST="1"))
    assert plain.qc_variant == case.variant and plain.qc_info()["no_persist"] and not code.qc_info()["no_persist"]
    assert _pf_variant(code)["has_pf"] and _pf_variant(plain)["index"] == _pf_variant(code)["index"]
    pg, fpw = code.persist_grid, code.qc_info()["frames_per_wg"]
    assert pg > 0 and pg % 8 == 0 and fpw == _pf_variant(code)["NF"]
    F = fpw * pg + fpw * 8 + 3
    assert (-(-F // fpw) + 7) // 8 * 8 > pg  # the dispatched grid would exceed the resident one: the persistent kernel runs
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, B = L * Z, Q.F_BLOCK
    block = _dev(Q.channel(orc, case.matrix, case.snr, B), N, B)
    yt = block.repeat(1, -(-F // B))[:, :F].contiguous()
    a = _decode(C, code, yt, max_iter=Q.MAXIT_PERSIST, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS)
    _named(code, _pf_variant(code))
    b = _decode(C, plain, yt, max_iter=Q.MAXIT_PERSIST, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS)
    _same_pf(a, (b["D"], b["app"], b["iters"]), case.id + " persistent against one workgroup per frame group")
    Dw, appw, itw = Q.want_block(orc, case.matrix, case.snr, Q.MAXIT_PERSIST)
    tail = F % B
    assert 0 < tail < B
    for lo, n in ((0, B), (F - tail - B, B), (F - tail, tail)):  # first tile, last whole tile, ragged tail
        assert np.array_equal(a["iters"][lo:lo + n], itw[:n]), "%s frames %d..: iteration counts differ" % (case.id, lo)
        assert np.array_equal(a["D"][:, lo:lo + n], Dw[:, :n]), "%s frames %d..: hard bits / flags differ" % (case.id, lo)
        assert np.array_equal(a["app"][:, lo:lo + n].view(np.uint32), appw[:, :n].view(np.uint32)), "%s frames %d..: sums differ" % (case.id, lo)


def test_every_variant_has_a_case():
    assert sorted(set(c.variant for c in CASES)) == list(range(len(VARIANTS)))


# ---- host paths of qc_decode outside the matrix ----------------------------------------------------------------------------------
def _three_modes(C, orc, code, spec, snr, F, what, pf_tag=None):
    """Fixed (with and without history), batch-global and per-frame results of `code` on F frames against the oracle."""
    _, _, _, L, Z = Q.matrix(spec)
    N = L * Z
    y = Q.channel(orc, spec, snr, F)
    oc = Q.ocode(orc, spec)
    yt = _dev(y, N, F)
    w = orc.bldpc_decode(oc, y, F, 7, early_exit=0, want_app=True)
    D, app, hist = _cols(w, N, F, F)
    for want_hist in (False, True):
        got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, want_flag_hist=want_hist)
        _same(got, D, app, 7, hist if want_hist else None, 7, what + " fixed")
    w = orc.bldpc_decode(oc, y, F, Q.MAXIT_GLOBAL, early_exit=1, want_app=True)
    assert 1 < w["it"] < Q.MAXIT_GLOBAL
    D, app, hist = _cols(w, N, F, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_QC_LDS, want_flag_hist=True)
    _same(got, D, app, w["it"], hist, w["it"], what + " batch-global")
    want = Q.oracle_per_frame(orc, oc, y, F, Q.MAXIT_GLOBAL)
    assert len(set(want[2].tolist())) > 1
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS)
    _same_pf(got, want, what + " per-frame")
    if pf_tag:
        assert pf_tag in code.last_kernel, code.last_kernel
    return got


@pytest.mark.parametrize("name", ["J4_L24_Z96", "J32_L64_Z64"])
def test_regroup_switch(C, orc, monkeypatch, name):
    """BLDPC_REGROUP=1: k_regroup_y in front of a two-frame kernel on an even batch, where the product reads in place."""
    spec = ("shipped", name)
    code = _make(C, monkeypatch, spec, {"BLDPC_REGROUP": "1"})
    inplace = _make(C, monkeypatch, spec, {})
    assert code.qc_info()["force_regroup"] and not inplace.qc_info()["force_regroup"]
    assert code.qc_variant == inplace.qc_variant >= 0 and VARIANTS[code.qc_variant]["NF"] == 2
    a = _three_modes(C, orc, code, spec, Q.SNR[spec], 6, name + " regrouped")
    b = _three_modes(C, orc, inplace, spec, Q.SNR[spec], 6, name + " in place")
    _same_pf(a, (b["D"], b["app"], b["iters"]), name + " regrouped against in place")


def test_local_per_frame_switch(C, orc, monkeypatch):
    """BLDPC_LOCAL_PER_FRAME=1 on J32_L64_Z64: no nested plan, the row kernel with local edges serves the per-frame exit (its
    retire path) and the pre-pass of the batch-global rule itself."""
    spec = ("shipped", "J32_L64_Z64")
    code = _make(C, monkeypatch, spec, {"BLDPC_LOCAL_PER_FRAME": "1"})
    assert VARIANTS[code.qc_variant]["tag"] == "row-local" and code.qc_variant_per_frame == -1
    assert _make(C, monkeypatch, spec, {}).qc_variant_per_frame == Q.find_variant(VARIANTS, "row", J=32, Z=64)
    for F in (5, 6):
        _three_modes(C, orc, code, spec, Q.SNR[spec], F, "local per-frame F=%d" % F, pf_tag="row-local")


def test_pinned_row_local_variant_has_no_nested_plan(C, orc, monkeypatch):
    """The pin holds for the nested plan too, which the plain row entry then cannot serve: the pinned local-edge plan runs every mode."""
    spec = ("shipped", "J32_L64_Z64")
    vi = Q.find_variant(VARIANTS, "row-local", J=32, Z=64)
    code = _make(C, monkeypatch, spec, {"BLDPC_QC_VARIANT": str(vi)})
    assert code.qc_variant == vi and code.qc_variant_per_frame == -1 and code.persist_grid == 0
    _three_modes(C, orc, code, spec, Q.SNR[spec], 5, "pinned row-local", pf_tag="row-local")


@pytest.mark.parametrize("name", ["J4_L24_Z96", "J8_L24_Z96"])
def test_ran_to_max_hint_never_changes_a_result(C, orc, monkeypatch, name):
    """QcPlan::ran_to_max survives between calls on one code object and decides whether the batch-global rule starts with a
    per-frame pass (then stop == run) or with a full run (then stop < run: a replay).  A batch that never stops sets it, one that
    stops early clears it; both orders on two objects, every result equal to the oracle's and to a fresh object's."""
    spec = ("shipped", name)
    _, _, _, L, Z = Q.matrix(spec)
    N, F, maxit = L * Z, Q.F_EXIT, Q.MAXIT_GLOBAL
    oc = Q.ocode(orc, spec)
    y_early = Q.channel(orc, spec, Q.SNR[spec], F)
    y_never = Q.channel(orc, spec, Q.SNR[spec] - 6.0, F)
    w_early = orc.bldpc_decode(oc, y_early, F, maxit, early_exit=1, want_app=True)
    w_never = orc.bldpc_decode(oc, y_never, F, maxit, early_exit=1, want_app=True)
    # never: runs to max_iter whichever pass comes first, and leaves the hint set.  early: after `never` the full run of max_iter
    # comes first and the stop iteration lies before it (stop < run, replay); on a fresh hint the per-frame pass gives the
    # latest first flag, at which every frame is still flagged (stop == run)
    assert w_never["it"] == maxit and not np.all(w_never["D"].reshape(N + 1, F)[N] == 1)
    assert 1 < w_early["it"] < maxit
    assert int(Q.oracle_per_frame(orc, oc, y_early, F, maxit)[2].max()) == w_early["it"]
    batches = {"early": (_dev(y_early, N, F), w_early), "never": (_dev(y_never, N, F), w_never)}
    for order in (("never", "early", "early"), ("early", "never", "early", "never")):
        code = _make(C, monkeypatch, spec, {})
        for k in order:
            yt, w = batches[k]
            D, app, hist = _cols(w, N, F, F)
            got = _decode(C, code, yt, max_iter=maxit, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_QC_LDS, want_flag_hist=True)
            _same(got, D, app, w["it"], hist, w["it"], "%s %s in %s" % (name, k, "-".join(order)))
            fresh = _decode(C, _make(C, monkeypatch, spec, {}), yt, max_iter=maxit, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=C.KERNEL_QC_LDS,
                            want_flag_hist=True)
            _same(fresh, D, app, w["it"], hist, w["it"], "%s %s on a fresh object" % (name, k))
