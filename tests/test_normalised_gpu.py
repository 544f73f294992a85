"""Normalised min-sum on the flooding decoders (bldpc_decode_normalised) on the GPU: every entry of the fused kernels' variant
table, under the cases of qc_variant_cases.py, through the normalised entry point.

Two references, both bit for bit (hard bits, flag row, a-posteriori sums as uint32, iteration counts):
  alpha = 1.0   the CPU oracle (x * 1.0f is exact), which holds the NORM instantiations to the reference's arithmetic;
  alpha = 0.75  bldpc_decode_normalised_host, the statement of the semantics inside the product (test_normalised_cpu.py holds it
                to the oracle and to a numpy restatement).
Then the table kernels, the persistent form, special values and the -0.0f sums of qc_trim_cases.py, the plain path on a code object
that has served normalised calls, Simulation_GPU(schedule="flooding", alpha=...), and the refusals of the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import qc_trim_cases as T
import qc_variant_cases as Q

pytestmark = pytest.mark.gpu

ALPHA = 0.75
# Es/N0 of the per-frame cases at alpha = 0.75 where the frames of the batch do NOT stop at different iterations at the Es/N0 of
# qc_variant_cases.SNR (found with the host statement alone, see test_per_frame_exit)
SNR_NORM = {("random", 320, 5, 11): 0.8}  # at 1.0 all five frames stop at iteration 5


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
ONE_PER_TAG = list({VARIANTS[c.variant]["tag"]: c for c in reversed(CASES)}.values())  # the first case of every tag
HALFROW = [c for c in CASES if VARIANTS[c.variant]["tag"].startswith("halfrow")]


def _make(C, monkeypatch, spec, env):
    path, _, J, L, Z = Q.matrix(spec)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    for k in env:
        monkeypatch.delenv(k)
    return code


def _case_code(C, monkeypatch, case):
    code = _make(C, monkeypatch, case.matrix, case.env)
    assert code.qc_variant == case.variant, "%s: the plan is variant %d, the case is meant for %d" % (case.id, code.qc_variant, case.variant)
    return code


def _pf_variant(code):
    return VARIANTS[code.qc_variant_per_frame if code.qc_variant_per_frame >= 0 else code.qc_variant]


def _named_norm(code, v):
    k = code.last_kernel
    assert k.endswith("_norm") and ("qc_lds_%s<" % v["tag"]) in k and ("Z%d," % v["Z"]) in k, (k, v)


def _dev(y, N, F):
    return torch.from_numpy(np.ascontiguousarray(y, np.float32).reshape(N, F)).cuda()


def _decode(C, code, yt, **kw):
    r = C.LDPC_Decoder_GPU(code, yt, want_app=True, **kw)
    torch.cuda.synchronize()
    out = dict(D=r["D"].cpu().numpy(), it=r["iteraTime"], app=r["app"].cpu().numpy())
    if r.get("iters") is not None:
        out["iters"] = r["iters"].cpu().numpy()
    return out


def _same(got, D, app, it, what):
    assert np.array_equal(got["D"][:-1], D[:-1]), what + ": hard bits differ"
    assert np.array_equal(got["D"][-1], D[-1]), what + ": flag row differs"
    assert np.array_equal(got["app"].view(np.uint32), np.ascontiguousarray(app).view(np.uint32)), what + ": a-posteriori sums differ bitwise"
    assert got["it"] == it, what + ": iteration count %s, expected %s" % (got["it"], it)


def _same_pf(got, want, what):
    Dw, appw, itw = want
    assert np.array_equal(got["iters"], itw), what + ": iteration counts %s, expected %s" % (got["iters"], itw)
    assert np.array_equal(got["D"], Dw), what + ": hard bits / flags differ"
    assert np.array_equal(got["app"].view(np.uint32), np.ascontiguousarray(appw).view(np.uint32)), what + ": a-posteriori sums differ bitwise"


def _host(C, spec, y, F, its, alpha=ALPHA, **kw):
    """The host statement on y [N * F]; (D, app, iters)."""
    _, H, J, L, Z = Q.matrix(spec)
    r = C.normalised_host(H, J, L, Z, np.ascontiguousarray(y, np.float32).reshape(L * Z, F), max_iter=its, alpha=alpha, **kw)
    return r["D"], r["app"], r["iters"]


def _host_fixed(C, orc, spec, snr, its):
    return Q._memo(("norm-fixed", spec, snr, its), lambda: _host(C, spec, Q.channel(orc, spec, snr, Q.F_FIXED), Q.F_FIXED, its))


def _host_pf(C, orc, spec, snr, length=0):
    return Q._memo(("norm-pf", spec, snr, length),
                   lambda: _host(C, spec, Q.channel(orc, spec, snr, Q.F_EXIT), Q.F_EXIT, Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, length=length))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixed_iterations(C, orc, monkeypatch, case):
    """The entry's fixed-iteration NORM kernel at 1, 2 and 7 iterations, F = 1, 5 and 6 (odd batches take the regrouped input, even
    ones of the two-frame kernels the in-place read)."""
    code = _case_code(C, monkeypatch, case)
    v = VARIANTS[case.variant]
    _, _, _, L, Z = Q.matrix(case.matrix)
    N = L * Z
    y6 = Q.channel(orc, case.matrix, case.snr, Q.F_FIXED).reshape(N, Q.F_FIXED)
    for its in (1, 2, 7):
        w = Q.want_fixed(orc, case.matrix, case.snr, its)
        Dh, apph, _ = _host_fixed(C, orc, case.matrix, case.snr, its)
        for F in (1, 5, 6):
            yt = _dev(y6[:, :F], N, F)
            got = _decode(C, code, yt, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=1.0)
            _named_norm(code, v)
            _same(got, w["D"].reshape(N + 1, Q.F_FIXED)[:, :F], w["app"].reshape(N, Q.F_FIXED)[:, :F], its, "%s alpha=1 its=%d F=%d" % (case.id, its, F))
            got = _decode(C, code, yt, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
            _named_norm(code, v)
            _same(got, Dh[:, :F], apph[:, :F], its, "%s alpha=%g its=%d F=%d" % (case.id, ALPHA, its, F))
    if its > 1:  # the multiplication shows: the two references differ
        assert not np.array_equal(apph.view(np.uint32), w["app"].reshape(N, Q.F_FIXED).view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_per_frame_exit(C, orc, monkeypatch, case):
    """A ragged batch whose frames stop at different iterations: alpha = 1 against the oracle's decode of each frame alone,
    alpha = 0.75 against the host statement's per-frame exit, iteration counts included."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F = L * Z, Q.F_EXIT
    yt = _dev(Q.channel(orc, case.matrix, case.snr, F), N, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=1.0)
    _named_norm(code, _pf_variant(code))
    _same_pf(got, Q.want_per_frame(orc, case.matrix, case.snr), case.id + " alpha=1")
    snr = SNR_NORM.get(case.matrix, case.snr)
    want = _host_pf(C, orc, case.matrix, snr)
    assert len(set(want[2].tolist())) > 1, "pick an Es/N0 at which frames stop at different iterations at alpha %g (%s)" % (ALPHA, want[2])
    yt = _dev(Q.channel(orc, case.matrix, snr, F), N, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
    _named_norm(code, _pf_variant(code))
    _same_pf(got, want, "%s alpha=%g" % (case.id, ALPHA))


@pytest.mark.parametrize("case", ONE_PER_TAG, ids=[c.id for c in ONE_PER_TAG])
def test_partial_length(C, orc, monkeypatch, case):
    """length = Z + 37: not a multiple of 32, ends inside the second block column; fixed iterations and the per-frame exit."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F, length = L * Z, Q.F_EXIT, Z + 37
    snr = SNR_NORM.get(case.matrix, case.snr)
    y = Q.channel(orc, case.matrix, snr, F)
    yt = _dev(y, N, F)
    D, app, _ = _host(C, case.matrix, y, F, 7, length=length)
    got = _decode(C, code, yt, max_iter=7, length=length, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
    _same(got, D, app, 7, case.id + " fixed")
    want = _host_pf(C, orc, case.matrix, snr, length)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, length=length, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
    _same_pf(got, want, case.id + " per-frame")
    w = Q.want_per_frame(orc, case.matrix, case.snr, length)
    got = _decode(C, code, _dev(Q.channel(orc, case.matrix, case.snr, F), N, F), max_iter=Q.MAXIT_GLOBAL, length=length,
                  exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=1.0)
    _same_pf(got, w, case.id + " per-frame alpha=1")


def _serves_persistent(case):
    v = VARIANTS[case.variant]
    return v["has_pf"] or (v["loc"] == 2 and "BLDPC_QC_VARIANT" not in case.env)


PERSIST_CASES = [c for c in CASES if _serves_persistent(c)]


@pytest.mark.parametrize("case", PERSIST_CASES, ids=[c.id for c in PERSIST_CASES])
def test_persistent_form(C, orc, monkeypatch, case):
    """The batch tiling of test_qc_variants_gpu.test_persistent_form (more frame groups than the resident grid, tiled from a block of
    64 frames) at alpha = 1: first and last tile and the ragged tail equal the oracle's decodes of the block's frames, each alone."""
    code = _case_code(C, monkeypatch, case)
    pg, fpw = code.persist_grid, code.qc_info()["frames_per_wg"]
    assert pg > 0 and pg % 8 == 0 and fpw == _pf_variant(code)["NF"]
    F = fpw * pg + fpw * 8 + 3
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, B = L * Z, Q.F_BLOCK
    block = _dev(Q.channel(orc, case.matrix, case.snr, B), N, B)
    yt = block.repeat(1, -(-F // B))[:, :F].contiguous()
    a = _decode(C, code, yt, max_iter=Q.MAXIT_PERSIST, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=1.0)
    _named_norm(code, _pf_variant(code))
    Dw, appw, itw = Q.want_block(orc, case.matrix, case.snr, Q.MAXIT_PERSIST)
    tail = F % B
    assert 0 < tail < B
    for lo, n in ((0, B), (F - tail - B, B), (F - tail, tail)):
        assert np.array_equal(a["iters"][lo:lo + n], itw[:n]), "%s frames %d..: iteration counts differ" % (case.id, lo)
        assert np.array_equal(a["D"][:, lo:lo + n], Dw[:, :n]), "%s frames %d..: hard bits / flags differ" % (case.id, lo)
        assert np.array_equal(a["app"][:, lo:lo + n].view(np.uint32), appw[:, :n].view(np.uint32)), "%s frames %d..: sums differ" % (case.id, lo)


@pytest.mark.parametrize("case", ONE_PER_TAG, ids=[c.id for c in ONE_PER_TAG])
def test_special_values(C, monkeypatch, case):
    """+-0, denormals (alpha times a denormal must not be flushed), +-3e38 and tied +-0.5, F = 3, 6 iterations, alpha = 0.75."""
    code = _case_code(C, monkeypatch, case)
    _, _, _, L, Z = Q.matrix(case.matrix)
    N, F = L * Z, 3
    y = Q.special_values(N, F)
    D, app, _ = _host(C, case.matrix, y, F, 6)
    got = _decode(C, code, _dev(y, N, F), max_iter=6, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
    _same(got, D, app, 6, case.id)
    y = np.full(N * 2, 1e-41, np.float32)  # every product alpha * min is denormal
    y[::7] = -3e-42
    D, app, _ = _host(C, case.matrix, y, 2, 3)
    assert np.all(np.abs(app) < np.float32(1.2e-38)) and np.any(app.reshape(-1) != y)
    got = _decode(C, code, _dev(y, N, 2), max_iter=3, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
    _same(got, D, app, 3, case.id + " denormal products")


@pytest.mark.parametrize("case", HALFROW, ids=[c.id for c in HALFROW])
def test_sums_of_minus_zero_on_the_half_row_entries(C, monkeypatch, case):
    """The inputs of qc_trim_cases.py (exact values; the corner frame drives every sum of some variables through -0.0f only) at
    alpha = 0.75: the loop's sums start at R_0 in the fixed exit and at 0 where the per-frame exit emits from inside the loop."""
    code = _case_code(C, monkeypatch, case)
    _, _, J, L, Z = Q.matrix(case.matrix)
    N = L * Z
    for name, (y, _) in T.batches(J, L, Z).items():
        F = y.shape[1]
        yt = _dev(y, N, F)
        for its in (1, 2, 3, 7):
            D, app, _ = _host(C, case.matrix, y, F, its)
            got = _decode(C, code, yt, max_iter=its, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
            _same(got, D, app, its, "%s %s its=%d" % (case.id, name, its))
        want = _host(C, case.matrix, y, F, 7, exit_mode=C.EXIT_PER_FRAME)
        got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
        _same_pf(got, want, "%s %s per-frame" % (case.id, name))


@pytest.mark.parametrize("name", ["J4_L24_Z96", "J32_L64_Z64"])
def test_table_kernels(C, orc, monkeypatch, name):
    """KERNEL_TABLE: fixed and per-frame, alpha 1.0 against the oracle and 0.75 against the host statement, F = 5 (one frame per
    lane) and the leading 4 frames (four per lane)."""
    spec = ("shipped", name)
    code = _make(C, monkeypatch, spec, {})
    _, _, _, L, Z = Q.matrix(spec)
    N, snr = L * Z, Q.SNR[spec]
    y6 = Q.channel(orc, spec, snr, Q.F_FIXED).reshape(N, Q.F_FIXED)
    w = Q.want_fixed(orc, spec, snr, 7)
    Dh, apph, _ = _host_fixed(C, orc, spec, snr, 7)
    for F, vec in ((5, "table_vec1_norm"), (4, "table_vec4_norm")):
        yt = _dev(y6[:, :F], N, F)
        got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_TABLE, alpha=1.0)
        assert code.last_kernel == vec
        _same(got, w["D"].reshape(N + 1, Q.F_FIXED)[:, :F], w["app"].reshape(N, Q.F_FIXED)[:, :F], 7, "%s alpha=1 F=%d" % (name, F))
        got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_TABLE, alpha=ALPHA)
        _same(got, Dh[:, :F], apph[:, :F], 7, "%s alpha=%g F=%d" % (name, ALPHA, F))
    F = Q.F_EXIT
    yt = _dev(Q.channel(orc, spec, snr, F), N, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_TABLE, alpha=1.0)
    _same_pf(got, Q.want_per_frame(orc, spec, snr), name + " per-frame alpha=1")
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_TABLE, alpha=ALPHA)
    _same_pf(got, _host_pf(C, orc, spec, snr), name + " per-frame alpha=%g" % ALPHA)


def test_as_written_table(C, orc):
    """The reference's Transform_H as written (colliding slots, level-scheduled launches) at alpha = 1 against the oracle; a code built
    from a table is accepted and runs the table kernels."""
    spec = ("shipped", "J4_L24_Z96")
    path, _, J, L, Z = Q.matrix(spec)
    H, wc, wv = C.Get_H(path, J, L)
    code = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv, as_written=True))
    assert code.levels > 1
    N, F = L * Z, Q.F_EXIT
    y = Q.channel(orc, spec, Q.SNR[spec], F)
    ocode = orc.BinaryCode(path, J, L, Z, literal=True)
    w = orc.bldpc_decode(ocode, y, F, 7, early_exit=0, want_app=True)
    got = _decode(C, code, _dev(y, N, F), max_iter=7, exit_mode=C.EXIT_FIXED, alpha=1.0)
    assert code.last_kernel == "table_vec1_norm"
    _same(got, w["D"].reshape(N + 1, F), w["app"].reshape(N, F), 7, "as written")
    got = _decode(C, code, _dev(y, N, F), max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, alpha=1.0)
    _same_pf(got, Q.oracle_per_frame(orc, ocode, y, F, Q.MAXIT_GLOBAL), "as written per-frame")
    from cuda_ldpc_amd._lib import LdpcError
    with pytest.raises(LdpcError):
        _decode(C, code, _dev(y, N, F), max_iter=7, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_QC_LDS, alpha=1.0)


def test_row_local_plan_without_nested_plan_falls_back_to_the_table_kernels(C, orc, monkeypatch):
    """A pinned row-local entry has no nested plain-row plan and no fused NORM kernel for the per-frame exit: AUTO runs the normalised
    table kernels and says so, an explicit KERNEL_QC_LDS is refused; fixed iterations run the entry's own NORM kernel."""
    from cuda_ldpc_amd._lib import LdpcError
    spec = ("shipped", "J32_L64_Z64")
    vi = Q.find_variant(VARIANTS, "row-local", J=32, Z=64)
    code = _make(C, monkeypatch, spec, {"BLDPC_QC_VARIANT": str(vi)})
    assert code.qc_variant == vi and code.qc_variant_per_frame == -1
    _, _, _, L, Z = Q.matrix(spec)
    N, F, snr = L * Z, Q.F_EXIT, Q.SNR[spec]
    yt = _dev(Q.channel(orc, spec, snr, F), N, F)
    got = _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, alpha=ALPHA)
    assert code.last_kernel == "table_vec1_norm"
    _same_pf(got, _host_pf(C, orc, spec, snr), "pinned row-local per-frame")
    with pytest.raises(LdpcError, match="no normalised kernel"):
        _decode(C, code, yt, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, kernel=C.KERNEL_QC_LDS, alpha=ALPHA)
    D, app, _ = _host(C, spec, Q.channel(orc, spec, snr, F), F, 7)
    got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_FIXED, alpha=ALPHA)
    _named_norm(code, VARIANTS[vi])
    _same(got, D, app, 7, "pinned row-local fixed")


@pytest.mark.parametrize("name", ["J4_L24_Z96", "J32_L64_Z64", "PON_LDPC"])
def test_plain_path_is_untouched(C, orc, monkeypatch, name):
    """Scratch and plans are shared: plain and normalised calls alternate on one code object, in both orders, and each reports its own
    kernel name and its own reference's bits."""
    spec = ("shipped", name)
    _, _, _, L, Z = Q.matrix(spec)
    N, snr, F = L * Z, Q.SNR[spec], Q.F_FIXED
    yt = _dev(Q.channel(orc, spec, snr, F), N, F)
    w = Q.want_fixed(orc, spec, snr, 7)
    Dh, apph, _ = _host_fixed(C, orc, spec, snr, 7)

    def plain(code):
        got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_FIXED)
        assert code.last_kernel.startswith("qc_lds_") and not code.last_kernel.endswith("_norm"), code.last_kernel
        _same(got, w["D"].reshape(N + 1, F), w["app"].reshape(N, F), 7, name + " plain")

    def norm(code):
        got = _decode(C, code, yt, max_iter=7, exit_mode=C.EXIT_FIXED, alpha=ALPHA)
        assert code.last_kernel.startswith("qc_lds_") and code.last_kernel.endswith("_norm"), code.last_kernel
        _same(got, Dh, apph, 7, name + " normalised")

    for order in ((norm, plain, norm), (plain, norm, plain)):
        code = _make(C, monkeypatch, spec, {})
        for call in order:
            call(code)
    code = _make(C, monkeypatch, spec, {})  # the per-frame passes too
    y5 = _dev(Q.channel(orc, spec, snr, Q.F_EXIT), N, Q.F_EXIT)
    got = _decode(C, code, y5, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME, alpha=ALPHA)
    _same_pf(got, _host_pf(C, orc, spec, snr), name + " normalised per-frame")
    got = _decode(C, code, y5, max_iter=Q.MAXIT_GLOBAL, exit_mode=C.EXIT_PER_FRAME)
    assert not code.last_kernel.endswith("_norm")
    _same_pf(got, Q.want_per_frame(orc, spec, snr), name + " plain per-frame after a normalised one")


def test_simulation_flooding_with_alpha(C):
    """Simulation_GPU(schedule="flooding", alpha=0.75): one batch of random codewords at EXIT_FIXED and one all-zero batch with
    per-frame exit; the counters equal those of the same steps composed by hand."""
    from cuda_ldpc_amd.simulation import Simulation_GPU
    spec = ("shipped", "J4_L24_Z96")
    path, _, J, L, Z = Q.matrix(spec)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    F, maxIT, pn_seed = 256, 20, 4242
    sigma = C.sigma_of(2.4)
    dev = torch.device("cuda", torch.cuda.current_device())

    def counters(SIM):
        return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]

    # random codewords, fixed iterations, syndrome flag
    SIM = C.SimCounters()
    seed = np.array([173, 173, 173], np.int32)
    Simulation_GPU(code, seed, sigma, SIM, Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_FIXED, max_batches=1, log=None,
                   device_channel=True, PN_Message=1, pn_seed=pn_seed, schedule="flooding", alpha=ALPHA, leastTestFrames=10 ** 9)
    seed2 = np.array([173, 173, 173], np.int32)
    cw = C.PN_CodeWords(code, pn_seed, F, first_frame=0, device=dev)
    y = C.AWGNChannel_GPU(seed2, sigma, code.N, F, device=dev, CodeWord=cw)
    r = C.LDPC_Decoder_GPU(code, y, max_iter=maxIT, length=code.K, exit_mode=C.EXIT_FIXED, alpha=ALPHA)
    assert code.last_kernel.endswith("_norm")
    C.Syndrome(code, r["D"], into_flag_row=True)
    ref = C.SimCounters()
    ref.num_Frames = F
    C.Statistic(ref, code, r["D"], r["iteraTime"], length=code.K, CodeWord=cw)
    assert SIM.num_Frames == F and counters(SIM) == counters(ref), (counters(SIM), counters(ref))
    assert np.array_equal(seed, seed2) and SIM.Total_Iteration == F * maxIT
    # all-zero codeword, per-frame exit
    SIM = C.SimCounters()
    seed = np.array([173, 173, 173], np.int32)
    Simulation_GPU(code, seed, sigma, SIM, Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=1, log=None,
                   device_channel=True, schedule="flooding", alpha=ALPHA, leastTestFrames=10 ** 9)
    seed2 = np.array([173, 173, 173], np.int32)
    y = C.AWGNChannel_GPU(seed2, sigma, code.N, F, device=dev)
    r = C.LDPC_Decoder_GPU(code, y, max_iter=maxIT, length=code.K, exit_mode=C.EXIT_PER_FRAME, alpha=ALPHA)
    ref = C.SimCounters()
    ref.num_Frames = F
    C.Statistic(ref, code, r["D"], r["iters"], length=code.K)
    assert counters(SIM) == counters(ref), (counters(SIM), counters(ref))
    assert F < SIM.Total_Iteration < F * maxIT  # frames stopped on their own flags
    with pytest.raises(ValueError):  # the batch-global rule stays with the plain decoders
        Simulation_GPU(code, seed, sigma, C.SimCounters(), Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_BATCH_GLOBAL, max_batches=1,
                       log=None, schedule="flooding", alpha=ALPHA)
    with pytest.raises(ValueError):  # the prefix rule tests for the zero word
        Simulation_GPU(code, seed, sigma, C.SimCounters(), Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=1,
                       log=None, schedule="flooding", alpha=ALPHA, PN_Message=1, device_channel=True)


def test_refusals_through_the_c_abi(C):
    from cuda_ldpc_amd._lib import lib
    spec = ("shipped", "J4_L24_Z96")
    path, _, J, L, Z = Q.matrix(spec)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N, F = L * Z, 4
    y = torch.ones((N, F), dtype=torch.float32, device="cuda")
    D = torch.zeros((N + 1, F), dtype=torch.int32, device="cuda")
    iters = torch.zeros(F, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    EINVAL = -1

    def call(max_iter=5, alpha=0.75, length=0, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_AUTO, it=iters, yy=y):
        return lib.bldpc_decode_normalised(code._h, p(yy), F, max_iter, ctypes.c_float(alpha), length, exit_mode, kernel, p(D), None, p(it), None)

    assert call() == 0 and call(exit_mode=C.EXIT_PER_FRAME) == 0 and call(alpha=1.0) == 0 and call(it=None) == 0
    for bad in (dict(alpha=0.0), dict(alpha=1.25), dict(alpha=float("nan")), dict(alpha=-0.75), dict(alpha=float("inf")), dict(max_iter=0),
                dict(exit_mode=C.EXIT_BATCH_GLOBAL), dict(exit_mode=9), dict(length=N + 1), dict(length=-1),
                dict(exit_mode=C.EXIT_PER_FRAME, it=None), dict(kernel=7), dict(yy=None)):
        rc = call(**bad)
        assert rc == EINVAL and lib.bldpc_last_error(), (bad, rc)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        C.LDPC_Decoder_GPU(code, y, exit_mode=C.EXIT_BATCH_GLOBAL, alpha=0.75)
    with pytest.raises(ValueError):
        C.LDPC_Decoder_GPU(code, y, exit_mode=C.EXIT_FIXED, alpha=0.75, want_flag_hist=True)
